"""ControlNet on the MI355X: vd_rows_eltwise op 7 bit for bit inside tests/memframe.py frames,
the tiny ControlNet and the UNet with residuals against tests/controlnet_ref.py, and
AnimateDiffControlNetPipeline end to end (graph vs eager, a disabled control, guess mode, LCM,
IP-Adapter) at 2 frames, 8 x 8 latents and 64 x 64 conditioning frames.

Bars (none taken from the device; tests/test_controlnet_host.py asserts that a dropped or swapped
residual moves the output by more than 3 x the largest of them):
  * op 7: equality with bf16(fp32(fp64(s) * z + x)) — |x|, |z| in [2^-6, 2^6] with 8 significant
    bits and s in {0, 0.1f, 1, 1.5f}, so the fp64 evaluation is exact and its rounding to fp32 is
    the fused multiply-add's;
  * the ControlNet's residuals: rel-L2 <= 3 x the bf16-emulating restatement's own deviation from
    the fp32 one (the factor and the 0.1 ceiling of tests/test_gpu_clip.py);
  * everything through the UNet: 1.3 x the bf16-emulating restatement's rel-L2 at that shape and
    on that quantity (test_tiny_unet_matches_oracle's headroom), the hooked module path against
    its own emulation (every module's output rounded).
"""
import pytest
import torch

import controlnet_ref as R
import memframe as mf
from vdiff import (AnimateDiffControlNetPipeline, AnimateDiffPipeline, ControlNetConditioning, DDIMScheduler,
                   DenoiseLoop, LCMScheduler, ops)
from vdiff._lib import lib
from vdiff.pipeline import ControlState, randn_tensor

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
G = 7.5
BAR_FACTOR, BAR_CEILING = 3.0, 0.1
S_VALUES = [0.0, 0.1, 1.0, 1.5]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


# ---------------------------------------------------------------- op 7
def lattice(rows, cols, seed):
    """bf16 values +-2^e * (1 + k / 128), e in -6..5, k in 0..127: |v| in [2^-6, 2^6)."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-6, 6, (rows, cols), generator=g).double()
    k = torch.randint(0, 128, (rows, cols), generator=g).double()
    sign = torch.randint(0, 2, (rows, cols), generator=g).double() * 2 - 1
    v = sign * torch.exp2(e) * (1 + k / 128)
    assert torch.equal(v.to(BF).double(), v)
    return v.to(BF)


def tables():
    """(period, ldy, table): one row and three rows of four columns; every s of S_VALUES sits in
    the first and in the last column of some row."""
    s = torch.tensor(S_VALUES, dtype=F32)
    one = s.roll(1)[None]
    three = torch.stack([s, s.roll(2), s.roll(3)])
    return [one, three]


def ctrl_reference(acc, res, s):
    """bf16(fp32(fp64(s) * z + x)): exact in fp64 on the lattice, then the two roundings."""
    return (float(s) * res.double() + acc.double()).to(F32).to(BF)


@pytest.mark.parametrize("slack", [0, 8])
@pytest.mark.parametrize("C", [8, 320])
@pytest.mark.parametrize("rows", [1, 37, 4096 + 3])
def test_ctrl_add_bit_for_bit_in_frames(cuda, rows, C, slack):
    acc0, res = lattice(rows, C, 10 * rows + C), lattice(rows, C, 10 * rows + C + 1)
    xv, fx = mf.load2d(res.cuda(), col_slack=slack, name="res")
    seen = set()
    for tab in tables():
        period, ldy = tab.shape
        bv, fb = mf.framed_1d(ops.CTRL_HEADER + tab.numel(), F32, cuda, name="block")
        for step in (-1, 0, 2, 99):
            for col in (0, ldy - 1):
                fb.poison()                                  # header words 1..3 stay NaN: they are ignored
                bv[ops.CTRL_HEADER:].copy_(tab.reshape(-1))
                bv[:1].view(torch.int32).fill_(step)
                ov, fo = mf.load2d(acc0.cuda(), col_slack=slack, name="acc")
                s = tab[min(max(step, 0), period - 1), col].item()
                seen.add(s)
                with mf.poisoned_empty():
                    got = ops.ctrl_add_(ov, xv, bv, col, cols=ldy)
                torch.cuda.synchronize()
                mf.assert_all_intact(fx, fb, fo)
                assert got.data_ptr() == ov.data_ptr()
                want = ctrl_reference(acc0, res, s)
                assert torch.equal(bits(ov.cpu()), bits(want)), (period, step, col, s)
                if s == 0.0:
                    assert torch.equal(ov.cpu(), acc0)      # the input under ==
                else:
                    assert not torch.equal(ov.cpu(), acc0)
                assert int(bv[:1].view(torch.int32).item()) == step
    assert seen == {torch.tensor(v, dtype=F32).item() for v in S_VALUES}
    assert torch.equal(bits(xv.cpu()), bits(res))            # the residual is only read


def test_ctrl_add_on_a_row_slice_and_a_column_slice(cuda):
    """The conditional half's rows of a wider buffer (guess mode under CFG), and a column slice."""
    acc0, res = lattice(64, 48, 1), lattice(32, 24, 2)
    block, step = ops.ctrl_block(torch.tensor([[0.1, 1.5], [1.0, 0.0]]), cuda)
    assert step.dtype == torch.int32 and step.data_ptr() == block.data_ptr() and int(step.item()) == 0
    assert torch.equal(ops.ctrl_table(block, 2).cpu(), torch.tensor([[0.1, 1.5], [1.0, 0.0]]))
    acc = acc0.cuda()
    ops.ctrl_add_(acc[32:, 8:32], res.cuda(), block, 1, cols=2)
    want = acc0.clone()
    want[32:, 8:32] = ctrl_reference(acc0[32:, 8:32], res, torch.tensor(1.5, dtype=F32).item())
    assert torch.equal(bits(acc.cpu()), bits(want))
    ops.step_advance(step)                                    # the loop's counter is the block's first word
    ops.ctrl_add_(acc[32:, 8:32], res.cuda(), block, 0, cols=2)
    want[32:, 8:32] = ctrl_reference(want[32:, 8:32], res, 1.0)
    assert torch.equal(bits(acc.cpu()), bits(want))


def test_ctrl_add_refuses_with_device_operands(cuda):
    """tests/test_controlnet_host.py's cases with operands the entry point would otherwise take:
    each differs from a valid call in the one argument named, and returns VD_EINVAL."""
    h = lib()
    x, out = torch.zeros(4, 16, dtype=BF, device=cuda), torch.zeros(4, 16, dtype=BF, device=cuda)
    block, _ = ops.ctrl_block(torch.ones(2, 3), cuda)
    px, po, py = x.data_ptr(), out.data_ptr(), block.data_ptr()
    host = torch.zeros(64, dtype=F32)
    stream = torch.cuda.current_stream().cuda_stream

    def call(op=7 | (1 << 8), x=px, ldx=16, y=py, ldy=3, y_f32=1, period=2, rows=4, C=8, out=po, ldo=16):
        return h.vd_rows_eltwise(op, x, ldx, y, ldy, y_f32, 1, period, rows, C, out, ldo, stream)

    assert call() == 0
    assert call(x=None) == 1000 and call(y=None) == 1000 and call(out=None) == 1000
    assert call(x=px + 2) == 1000 and call(y=py + 4) == 1000 and call(out=po + 8) == 1000
    assert call(y_f32=0) == 1000
    assert call(ldy=0) == 1000 and call(ldy=65) == 1000
    assert call(op=7 | (3 << 8)) == 1000
    assert call(op=7 | (1 << 8) | (1 << 16)) == 1000 and call(op=-(1 << 31) | 7) == 1000
    assert call(period=0) == 1000
    assert call(C=12) == 1000
    assert call(out=px) == 1000
    assert call(y=host.data_ptr()) == 1000                   # the control block must be device memory
    torch.cuda.synchronize()
    assert call() == 0                                        # and no refused call left an error behind
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the models
@pytest.fixture(scope="module")
def case(cuda):
    """tests/controlnet_ref.py's case with both models on the device (the CPU copies stay fp32)."""
    c = dict(R.tiny_case())
    c["dunet"] = c["unet"].__class__("tiny")
    c["dunet"].load_state_dict(c["unet"].state_dict())
    c["dunet"] = c["dunet"].to(cuda, BF).prepare()
    c["dcnet"] = R.random_controlnet("tiny", seed=1).to(cuda, BF).prepare()
    return c


def test_controlnet_forward_matches_the_restatement(case):
    """diffusers' calling convention — (B*F, C, H, W) sample, (B*F, L, D) text, (B*F, 3, 8H, 8W)
    conditioning — and forward_rows in the loop's layout: every residual within 3 x the emulated
    deviation.  Printed: DESIGN.md's table."""
    c, cn = case, case["dcnet"]
    nf = c["x2"].shape[2]
    sample = c["x2"].permute(0, 2, 1, 3, 4).reshape(-1, 4, 8, 8).cuda()
    cond = c["cond2"].permute(0, 2, 1, 3, 4).reshape(-1, 3, 64, 64).cuda()
    ehs = c["ehs"].repeat_interleave(nf, 0).cuda()
    out = cn(sample, c["t"], ehs, cond)
    assert len(out.down_block_res_samples) == 4 and out[1] is out.mid_block_res_sample
    got = [*out.down_block_res_samples, out.mid_block_res_sample]
    # the loop's layout: 2 videos of 2 frames, the text rows per video
    te = ops.timestep_embed(torch.full((2,), float(c["t"]), device="cuda"), cn.time_proj.num_channels)
    ctx = cn.make_ctx(te, c["ehs"].to("cuda", BF).reshape(2 * 77, -1), 2, nf, 77, kv_cache={})
    rows = cn.forward_rows(ops.pack_latents(c["x2"].cuda(), dup=1, cpad=8), cn.embed_condition(c["cond2"].cuda()),
                           8, 8, ctx)
    for i, (g, a, ref, emu) in enumerate(zip(got, rows, c["res_fp32"], c["res_bf16"])):
        assert tuple(g.shape) == tuple(ref.shape) and g.dtype == BF
        e_emu = R.rel_l2(emu, ref)
        bar = BAR_FACTOR * e_emu
        e_dev = R.rel_l2(g, ref)
        e_rows = R.rel_l2(a.t.float().cpu().view(a.n, a.h, a.w, -1).permute(0, 3, 1, 2), ref)
        print(f"CONTROLNET residual {i} {tuple(ref.shape)}: emulated {e_emu:.5f} forward {e_dev:.5f} "
              f"forward_rows {e_rows:.5f} bar {bar:.5f}")
        assert 0 < bar <= BAR_CEILING
        assert torch.isfinite(g.float()).all()
        assert e_dev <= bar, (i, e_dev, bar)
        assert e_rows <= bar, (i, e_rows, bar)


def test_controlnet_forward_scales_with_op3(case):
    c, cn = case, case["dcnet"]
    sample = c["x2"].permute(0, 2, 1, 3, 4).reshape(-1, 4, 8, 8).cuda()
    cond = c["cond2"].permute(0, 2, 1, 3, 4).reshape(-1, 3, 64, 64).cuda()
    ehs = c["ehs"].repeat_interleave(2, 0).cuda()
    base = cn(sample, c["t"], ehs, cond, return_dict=False)
    base = [*base[0], base[1]]
    half = cn(sample, c["t"], ehs, cond, conditioning_scale=0.5)
    guess = cn(sample, c["t"], ehs, cond, conditioning_scale=0.5, guess_mode=True)
    ls = torch.logspace(-1, 0, 5)
    for i, b in enumerate(base):
        h = [*half.down_block_res_samples, half.mid_block_res_sample][i]
        g = [*guess.down_block_res_samples, guess.mid_block_res_sample][i]
        assert torch.equal(h.cpu(), (b.float().cpu() * torch.tensor(0.5)).to(BF))
        assert torch.equal(g.cpu(), (b.float().cpu() * (0.5 * ls[i])).to(BF))


def _unet_with_given(case, hooked):
    c, unet = case, case["dunet"]
    given = [g.cuda() for g in c["given"]]
    hook = unet.mid_block.register_forward_hook(lambda m, a, o: None) if hooked else None
    try:
        return unet(c["x2"].cuda(), c["t"], encoder_hidden_states=c["ehs"].cuda(),
                    down_block_additional_residuals=given[:-1], mid_block_additional_residual=given[-1]).sample
    finally:
        if hook is not None:
            hook.remove()


def test_unet_fast_path_takes_given_residuals(case):
    out = _unet_with_given(case, hooked=False)
    err = R.rel_l2(out, case["out_fp32"])
    print(f"UNET+residuals fast path: emulated {case['unet_emulated']:.5f} device {err:.5f} bar {case['unet_bar']:.5f}")
    assert err <= case["unet_bar"], err
    # the given tensors are not touched, and a second call gives the same bits
    assert torch.equal(bits(_unet_with_given(case, hooked=False)), bits(out))


def test_unet_hooked_path_takes_given_residuals(case):
    out = _unet_with_given(case, hooked=True)
    err = R.rel_l2(out, case["out_fp32"])
    print(f"UNET+residuals module path: emulated {case['unet_emulated_modules']:.5f} device {err:.5f} "
          f"bar {case['unet_bar_modules']:.5f}")
    assert err <= case["unet_bar_modules"], err


def test_unet_forward_refuses_a_wrong_count(case):
    given = [g.cuda() for g in case["given"]]
    with pytest.raises(ValueError, match="down-block residuals"):
        case["dunet"](case["x2"].cuda(), 961, encoder_hidden_states=case["ehs"].cuda(),
                      down_block_additional_residuals=given[:2], mid_block_additional_residual=given[-1])


# ---------------------------------------------------------------- the pipeline
def ddim():
    return DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)


def call_kw(c, steps=3):
    return dict(prompt_embeds=c["ehs"][1:2], negative_prompt_embeds=c["ehs"][0:1], latents=c["lat"], num_frames=2,
                height=64, width=64, num_inference_steps=steps, guidance_scale=G, output_type="latent",
                conditioning_frames=c["cond"][0].permute(1, 0, 2, 3))   # (F, 3, H, W) in [0, 1]


@pytest.fixture(scope="module")
def pipe(case):
    return AnimateDiffControlNetPipeline(case["dunet"], case["dcnet"], ddim())


@pytest.fixture(scope="module")
def plain(case):
    kw = call_kw(case)
    kw.pop("conditioning_frames")
    return AnimateDiffPipeline(case["dunet"], ddim())(**kw).frames.clone()


def test_graph_equals_eager_while_the_scale_changes(case, pipe, plain):
    """(start, end) = (0, 0.5) over 3 steps: scale 1, 0, 0 — read by the step index inside the replays."""
    kw = dict(call_kw(case), control_guidance_start=0.0, control_guidance_end=0.5)
    graph = pipe(**kw, use_graph=True).frames.clone()
    eager = pipe(**kw, use_graph=False).frames.clone()
    assert torch.equal(bits(graph), bits(eager))
    full = pipe(**call_kw(case)).frames.clone()
    assert not torch.equal(graph, full) and not torch.equal(graph, plain)
    # the loop itself: the capture succeeded, and a second run after reset equals the first
    s = ddim()
    s.set_timesteps(3)
    ctl = ControlNetConditioning(case["dcnet"], case["cond"], 1.0, False, 0.0, 0.5)
    loop = DenoiseLoop(case["dunet"], s, case["lat"], case["ehs"], G, control=ctl).prime()
    assert loop.graph is not None, loop.graph_error
    assert loop.step_idx.data_ptr() == loop.ctrl_block.data_ptr()
    assert ops.ctrl_table(loop.ctrl_block, 5)[:, 0].tolist() == [1.0, 0.0, 0.0]
    first = loop.run().clone()
    assert int(loop.step_idx.item()) == 3
    assert torch.equal(bits(first), bits(graph))
    loop.reset(case["lat"].cuda())
    assert torch.equal(bits(loop.run()), bits(first))


def test_disabled_control_is_the_plain_pipeline(case, pipe, plain):
    off = pipe(**call_kw(case), controlnet_conditioning_scale=0.0).frames
    assert torch.equal(off, plain)
    off = pipe(**call_kw(case), control_guidance_start=0.0, control_guidance_end=0.0).frames
    assert torch.equal(off, plain)
    on = pipe(**call_kw(case)).frames
    assert R.rel_l2(on, plain) > 3 * case["unet_bar"]


def test_ddim_run_matches_the_restatement(case, pipe):
    c = case
    table = R.scale_table(3, 5, 1.0, False, 0.0, 0.5)
    with torch.no_grad():
        ref, emu = (R.ddim_loop(c["usd"], c["csd"], c["cfg"], c["ccfg"], c["lat"], c["ehs"], c["cond"], table, False,
                                3, G, act) for act in ("fp32", "bf16"))
    got = pipe(**call_kw(c), control_guidance_start=0.0, control_guidance_end=0.5).frames
    e_emu, e_dev = R.rel_l2(emu, ref), R.rel_l2(got, ref)
    print(f"PIPELINE ddim (0, 0.5): emulated {e_emu:.5f} device {e_dev:.5f} bar {1.3 * e_emu:.5f}")
    assert e_dev <= 1.3 * e_emu


def test_guess_mode_leaves_the_unconditional_half_alone(case, monkeypatch):
    """One eager step: every skip's (and the mid output's) unconditional rows keep their bits, the
    conditional rows move; the ControlNet ran on the conditional half only."""
    seen = []
    inject = ControlState.inject

    def spy(self, skips, mid, ctx):
        before = [a.t.clone() for a in [*skips, mid]]
        inject(self, skips, mid, ctx)
        seen.append((self, before, [a.t.clone() for a in [*skips, mid]]))

    monkeypatch.setattr(ControlState, "inject", spy)
    s = ddim()
    s.set_timesteps(3)
    ctl = ControlNetConditioning(case["dcnet"], case["cond"], 1.0, True)
    loop = DenoiseLoop(case["dunet"], s, case["lat"], case["ehs"], G, use_graph=False, control=ctl)
    assert loop.cn_cond_only and loop.cn_batch == 1
    loop.step()
    torch.cuda.synchronize()
    state, before, after = seen[-1]
    assert state.cond_only and len(before) == 5
    for i, (b, a, r) in enumerate(zip(before, after, state.residuals)):
        h = b.shape[0] // 2
        assert r.t.shape[0] == h
        assert torch.equal(bits(a[:h]), bits(b[:h])), i
        assert not torch.equal(a[h:], b[h:]), i
    assert torch.allclose(ops.ctrl_table(loop.ctrl_block, 5)[0].cpu(), torch.logspace(-1, 0, 5))


def test_guess_mode_run_matches_the_restatement(case, pipe):
    c = case
    table = R.scale_table(3, 5, 1.0, True)
    with torch.no_grad():
        ref, emu = (R.ddim_loop(c["usd"], c["csd"], c["cfg"], c["ccfg"], c["lat"], c["ehs"], c["cond"], table, True,
                                3, G, act) for act in ("fp32", "bf16"))
    got = pipe(**call_kw(c), guess_mode=True).frames
    e_emu, e_dev = R.rel_l2(emu, ref), R.rel_l2(got, ref)
    print(f"PIPELINE guess mode: emulated {e_emu:.5f} device {e_dev:.5f} bar {1.3 * e_emu:.5f}")
    assert e_dev <= 1.3 * e_emu
    assert not torch.equal(got, pipe(**call_kw(c)).frames)


def test_lcm_run_matches_the_restatement(case):
    c, n = case, 4
    p = AnimateDiffControlNetPipeline(c["dunet"], c["dcnet"], LCMScheduler.from_config(None, beta_schedule="linear"))
    p.torch_dtype = F32
    got = p(**call_kw(c, steps=n), generator=torch.manual_seed(0)).frames
    gen = torch.manual_seed(0)   # latents are given: the step noise is all the call draws
    noise = torch.stack([randn_tensor(c["lat"].shape, gen, device="cuda", dtype=F32) for _ in range(n - 1)]).cpu()
    table = R.scale_table(n, 5)
    with torch.no_grad():
        ref, emu = (R.lcm_loop(c["usd"], c["csd"], c["cfg"], c["ccfg"], c["lat"], c["ehs"], c["cond"], table, False,
                               n, G, noise, act) for act in ("fp32", "bf16"))
    e_emu, e_dev = R.rel_l2(emu, ref), R.rel_l2(got, ref)
    print(f"PIPELINE lcm: emulated {e_emu:.5f} device {e_dev:.5f} bar {1.3 * e_emu:.5f}")
    assert torch.isfinite(got).all()
    assert e_dev <= 1.3 * e_emu


def test_ip_adapter_run_completes(cuda, case):
    from test_ip_adapter_host import synthetic_adapter
    p = AnimateDiffControlNetPipeline.from_config("tiny", device=cuda, vae=None)
    kw = call_kw(case, steps=2)
    without = p(**kw).frames.clone()
    p.load_ip_adapter(synthetic_adapter(p.unet, n=4, clip_dim=48, scale=3.0))
    embeds = torch.randn(2, 1, 48, generator=torch.Generator().manual_seed(2))
    with_ip = p(**kw, ip_adapter_image_embeds=embeds).frames
    assert torch.isfinite(with_ip).all() and not torch.equal(with_ip, without)
    p.unload_ip_adapter()
    assert torch.equal(p(**kw).frames, without)
