"""SparseCtrl on the MI355X: vd_rows_eltwise op 8 bit for bit inside tests/memframe.py frames and
its refusals, the tiny SparseControlNetModel (both embedding variants) against
tests/sparsectrl_ref.py, and AnimateDiffSparseControlNetPipeline end to end at 4 frames, 8 x 8
latents, 2 key frames at frames [0, 3].

Bars (none taken from the device):
  * op 8: equality of bits with torch index assignment over int16 bit patterns (any pattern,
    NaNs included: the op copies, it does no arithmetic);
  * the residuals: rel-L2 <= BAR_FACTOR x the bf16-emulating restatement's own deviation from the
    fp32 one, which must be positive and under BAR_CEILING — tests/test_gpu_controlnet.py's;
  * the DDIM run: 1.3 x the emulated deviation of the restatement's loop, the factor of
    test_ddim_run_matches_the_restatement there.
"""
import pytest
import torch

import memframe as mf
import sparsectrl_ref as S
from test_gpu_controlnet import BAR_CEILING, BAR_FACTOR
from vdiff import (AnimateDiffPipeline, AnimateDiffSparseControlNetPipeline, AutoencoderKL, DDIMScheduler, DenoiseLoop,
                   DPMSolverMultistepScheduler, LCMScheduler, SparseControlConditioning, init_synthetic_, ops)
from vdiff._lib import lib
from vdiff.pipeline import ControlState

pytestmark = pytest.mark.gpu
BF, F32, I16 = torch.bfloat16, torch.float32, torch.int16
G = 7.5
ONE = 0x3F80  # bf16 1.0


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else I16)


# ---------------------------------------------------------------- op 8
def key_bits(B, K, hw, cc, seed):
    """[B * K * hw, 8] int16 bit patterns: columns < cc anything at all, columns cc..7 poison."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-32768, 32768, (B * K * hw, 8), generator=g, dtype=torch.int32).to(I16)
    x[:, cc:] = -1
    return x


def cond_reference(x, idx, B, F, K, hw, cc):
    """prepare_sparse_control_conditioning as index assignment, on the bit patterns, in the rows'
    layout: zeros, then per (k, i) in order the key frame, the mask, zeros above."""
    x = x.view(B, K, hw, 8)
    out = torch.zeros(B, F, hw, 8, dtype=I16)
    for k, i in enumerate(idx):
        if 0 <= i < F:
            out[:, i] = 0
            out[:, i, :, :cc] = x[:, k, :, :cc]
            out[:, i, :, cc] = ONE
    return out.view(B * F * hw, 8)


CASES = [
    (1, 1, 1, 1, 4, [0]),
    (2, 5, 2, 3, 4, [4, 0]),
    (1, 32, 32, 7, 3, torch.randperm(32, generator=torch.Generator().manual_seed(0)).tolist()),
    (2, 16, 3, 64, 4, [0, 8, 15]),
    (1, 4, 2, 5, 4, [2, 2]),
    (1, 2, 1, 4099, 4, [1]),            # 8198 rows: a ragged grid tail
]


@pytest.mark.parametrize("slack", [0, 8])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:5])))
def test_sparse_cond_bit_for_bit_in_frames(cuda, case, slack):
    B, F, K, hw, cc, idx = case
    x = key_bits(B, K, hw, cc, 100 * F + hw)
    want = cond_reference(x, idx, B, F, K, hw, cc)
    xv, fx = mf.load2d(x.view(BF).cuda(), col_slack=slack, name="keys")
    ov, fo = mf.framed((B * F * hw, 8), BF, cuda, col_slack=slack, name="out")
    with mf.poisoned_empty():
        got = ops.sparse_cond(xv, idx, B, F, hw, cc, out=ov)
        own = ops.sparse_cond(xv, idx, B, F, hw, cc)       # the output the wrapper allocates itself
    torch.cuda.synchronize()
    mf.assert_all_intact(fx, fo)
    fo.assert_written(want.view(BF))
    assert got.data_ptr() == ov.data_ptr()
    assert torch.equal(bits(ov.cpu()), want)
    assert torch.equal(bits(own.cpu()), want)
    assert torch.equal(bits(xv.cpu()), x)                    # the key rows are only read
    if cc < 7:
        assert not (bits(ov.cpu())[:, cc + 1:] != 0).any()   # no poison column came through


def raw_call(h, op, x, ldx, y, K, y_f32, hw, F, rows, C, out, ldo):
    return h.vd_rows_eltwise(op, x, ldx, y, K, y_f32, hw, F, rows, C, out, ldo, torch.cuda.current_stream().cuda_stream)


def test_an_index_equal_to_F_leaves_the_frames_zero(cuda):
    """The entry point below the wrapper (which raises IndexError): idx = [1, F, -1] sets frame 1."""
    B, F, K, hw, cc = 2, 3, 3, 5, 4
    x = key_bits(B, K, hw, cc, 9)
    xv, fx = mf.load2d(x.view(BF).cuda(), name="keys")
    iv, fi = mf.framed_1d(K, torch.int32, cuda, name="idx")
    iv.copy_(torch.tensor([1, F, -1], dtype=torch.int32))
    ov, fo = mf.framed((B * F * hw, 8), BF, cuda, name="out")
    assert raw_call(lib(), 8 | (cc << 8), xv.data_ptr(), xv.stride(0), iv.data_ptr(), K, 1, hw, F, B * F * hw, 8,
                    ov.data_ptr(), ov.stride(0)) == 0
    torch.cuda.synchronize()
    mf.assert_all_intact(fx, fi, fo)
    fo.assert_written()
    want = cond_reference(x, [1, F, -1], B, F, K, hw, cc)
    assert torch.equal(bits(ov.cpu()), want)
    assert not bits(ov.cpu()).view(B, F, hw, 8)[:, [0, 2]].any()


def test_sparse_cond_refuses_with_device_operands(cuda):
    """Each call differs from a valid one in the one argument named and returns VD_EINVAL; nothing
    is launched (out stays poison) and no refused call leaves a sticky error behind."""
    h = lib()
    x = torch.zeros(2 * 4, 16, dtype=BF, device=cuda)            # B = 1, K = 2, hw = 4
    ov, fo = mf.framed((3 * 4, 16), BF, cuda, name="out")         # F = 3
    idx = torch.tensor([0, 2, 0, 0], dtype=torch.int32, device=cuda)
    px, po, py = x.data_ptr(), ov.data_ptr(), idx.data_ptr()
    host = torch.zeros(64, dtype=torch.int32)

    def call(op=8 | (4 << 8), x=px, ldx=16, y=py, K=2, y_f32=1, hw=4, F=3, rows=12, C=8, out=po, ldo=16):
        return raw_call(h, op, x, ldx, y, K, y_f32, hw, F, rows, C, out, ldo)

    refused = [
        call(op=8), call(op=8 | (8 << 8)), call(op=8 | (4 << 8) | (1 << 16)), call(op=-(1 << 31) | 8 | (4 << 8)),
        call(C=16), call(C=0),
        call(K=0), call(K=257), call(F=0), call(F=257, rows=257 * 4), call(hw=0),
        call(rows=13), call(rows=0),
        call(x=None), call(out=None), call(x=px + 2), call(out=po + 8), call(out=px),
        call(ldx=4), call(ldo=4), call(ldx=12), call(ldo=12),
        call(y=None), call(y=py + 2), call(y_f32=0), call(y_f32=2), call(y=host.data_ptr()),
    ]
    assert refused == [1000] * len(refused)
    torch.cuda.synchronize()
    assert bool(mf.is_poison(ov).all())                            # nothing was launched
    assert call() == 0                                             # and no refused call left an error behind
    torch.cuda.synchronize()
    fo.assert_intact()
    assert not bool(mf.is_poison(ov[:, :8]).any())


# ---------------------------------------------------------------- the models
@pytest.fixture(scope="module")
def case(cuda):
    """tests/sparsectrl_ref.py's case with the models on the device (the CPU copies stay fp32)."""
    c = dict(S.tiny_case())
    c["dunet"] = c["unet"].__class__("tiny")
    c["dunet"].load_state_dict(c["unet"].state_dict())
    c["dunet"] = c["dunet"].to(cuda, BF).prepare()
    for simplified in (True, False):
        v = dict(c[simplified])
        d = S.random_sparse_controlnet("tiny", seed=1 if simplified else 2, simplified=simplified)
        v["dcnet"] = d.to(cuda, BF).prepare()
        c[simplified] = v
    return c


def device_residuals(c, v, cond=None, mask=None, sample=None, **kw):
    cn = v["dcnet"]
    out = cn(c["x2"].cuda() if sample is None else sample, c["t"], c["ehs"].cuda(),
             (v["cond"] if cond is None else cond).cuda(), (v["mask"] if mask is None else mask).cuda(), **kw)
    return [*out.down_block_res_samples, out.mid_block_res_sample]


@pytest.mark.parametrize("simplified", [True, False], ids=["simplified", "full"])
def test_sparse_controlnet_matches_the_restatement(case, simplified):
    """forward (diffusers' layout) and forward_rows (the loop's) on 2 videos x 4 frames x 8 x 8
    latents with key frames at [0, 3], the condition rows from op 8.  Printed: DESIGN.md's table."""
    c, v = case, case[simplified]
    cn = v["dcnet"]
    got = device_residuals(c, v)
    assert len(got) == 5
    B, nf = 2, S.NF
    hc = v["cond"].shape[3]
    keys = ops.pack_latents(v["keys"].cuda(), dup=1, cpad=8)
    cond_rows = ops.sparse_cond(keys, S.IDX, B, nf, hc * hc, v["cond"].shape[1])
    assert torch.equal(bits(cond_rows), bits(cn.condition_rows(v["cond"], v["mask"])))
    te = ops.timestep_embed(torch.full((B,), float(c["t"]), device="cuda"), cn.time_proj.num_channels)
    ctx = cn.make_ctx(te, c["ehs"].to("cuda", BF).reshape(B * 77, -1), B, nf, 77, kv_cache={})
    rows = cn.forward_rows(cn.embed_condition(cond_rows, B * nf, hc, hc), 8, 8, ctx)
    for i, (g, a, ref, emu) in enumerate(zip(got, rows, v["res_fp32"], v["res_bf16"])):
        assert tuple(g.shape) == tuple(ref.shape) and g.dtype == BF
        e_emu = S.rel_l2(emu, ref)
        bar = BAR_FACTOR * e_emu
        e_dev = S.rel_l2(g, ref)
        e_rows = S.rel_l2(a.t.float().cpu().view(a.n, a.h, a.w, -1).permute(0, 3, 1, 2), ref)
        print(f"SPARSECTRL {'simplified' if simplified else 'full'} residual {i} {tuple(ref.shape)}: "
              f"emulated {e_emu:.5f} forward {e_dev:.5f} forward_rows {e_rows:.5f} bar {bar:.5f}")
        assert 0 < bar <= BAR_CEILING
        assert torch.isfinite(g.float()).all()
        assert e_dev <= bar, (i, e_dev, bar)
        assert e_rows <= bar, (i, e_rows, bar)


def test_residuals_ignore_the_latents_and_follow_the_key_frame(case):
    c, v = case, case[True]
    base = device_residuals(c, v)
    other = device_residuals(c, v, sample=torch.randn_like(c["x2"]).cuda())
    keys = v["keys"].clone()
    keys[:, :, 0] = keys[:, :, 0].flip(-1) + 0.25                  # the key frame at frame 0 alone
    cond, mask = S.prepare_sparse_control_conditioning(keys, S.NF, S.IDX)
    moved = device_residuals(c, v, cond=cond, mask=mask)
    last = [S.NF - 1, 2 * S.NF - 1]
    for i, (a, b, m) in enumerate(zip(base, other, moved)):
        assert torch.equal(bits(a), bits(b)), i
        # residual 0 is per frame; every later one sits behind a motion module
        assert torch.equal(bits(a[last]), bits(m[last])) == (i == 0), i


def test_forward_scales_with_op3(case):
    c, v = case, case[True]
    base = device_residuals(c, v, return_dict=True)
    half = device_residuals(c, v, conditioning_scale=0.5)
    guess = device_residuals(c, v, conditioning_scale=0.5, guess_mode=True)
    ls = torch.logspace(-1, 0, 5)
    for i, b in enumerate(base):
        assert torch.equal(half[i].cpu(), (b.float().cpu() * torch.tensor(0.5)).to(BF))
        assert torch.equal(guess[i].cpu(), (b.float().cpu() * (0.5 * ls[i])).to(BF))


def test_more_frames_than_the_motion_modules_take_are_refused(case):
    cn = case[True]["dcnet"]
    with pytest.raises(ValueError, match="motion_max_seq_length"):
        cn(torch.zeros(1, 4, 33, 8, 8), 1, case["ehs"][:1], torch.zeros(1, 4, 33, 8, 8), torch.zeros(1, 1, 33, 8, 8))


# ---------------------------------------------------------------- the pipeline
def ddim():
    return DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)


IMAGES = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(11))   # the tiny VAE is 2x: 8 x 8 latents


def call_kw(c, steps=3):
    return dict(prompt_embeds=c["ehs"][1:2], negative_prompt_embeds=c["ehs"][0:1], latents=c["lat"], num_frames=S.NF,
                height=64, width=64, num_inference_steps=steps, guidance_scale=G, output_type="latent")


def sparse_kw(c, steps=3):
    return dict(call_kw(c, steps), conditioning_frames=IMAGES, controlnet_frame_indices=S.IDX,
                generator=torch.manual_seed(3))


@pytest.fixture(scope="module")
def vae(cuda):
    return init_synthetic_(AutoencoderKL("tiny", encoder=True), seed=0).to(cuda, BF).prepare()


@pytest.fixture(scope="module")
def pipe(case, vae):
    return AnimateDiffSparseControlNetPipeline(case["dunet"], case[True]["dcnet"], ddim(), vae=vae)


@pytest.fixture(scope="module")
def plain(case):
    return AnimateDiffPipeline(case["dunet"], ddim())(**call_kw(case)).frames.clone()


@pytest.fixture(scope="module")
def conditioning(pipe):
    """What the pipeline's calls condition on: the key latents (seed 3) and diffusers' two tensors."""
    keys = pipe.prepare_key_frames(IMAGES, 8, 8, generator=torch.manual_seed(3))
    cond, mask = pipe.prepare_sparse_control_conditioning(keys, S.NF, S.IDX)
    assert tuple(cond.shape) == (1, 4, S.NF, 8, 8) and tuple(mask.shape) == (1, 1, S.NF, 8, 8)
    wc, wm = S.prepare_sparse_control_conditioning(keys.cpu().to(BF).float(), S.NF, S.IDX)
    assert torch.equal(cond.cpu(), wc) and torch.equal(mask.cpu(), wm)
    return keys.cpu(), cond.cpu(), mask.cpu()


def test_graph_equals_eager_and_a_second_run(case, pipe, plain, conditioning):
    graph = pipe(**sparse_kw(case), use_graph=True).frames.clone()
    eager = pipe(**sparse_kw(case), use_graph=False).frames.clone()
    assert torch.equal(bits(graph), bits(eager))
    assert not torch.equal(graph, plain)
    _, cond, mask = conditioning
    s = ddim()
    s.set_timesteps(3)
    ctl = SparseControlConditioning.from_tensors(case[True]["dcnet"], cond, mask)
    loop = DenoiseLoop(case["dunet"], s, case["lat"], case["ehs"], G, control=ctl).prime()
    assert loop.graph is not None, loop.graph_error
    assert loop.step_idx.data_ptr() == loop.ctrl_block.data_ptr()
    assert ops.ctrl_table(loop.ctrl_block, 5).cpu().tolist() == [[1.0] * 5] * 3
    first = loop.run().clone()
    assert torch.equal(bits(first), bits(graph))
    loop.reset(case["lat"].cuda())
    assert torch.equal(bits(loop.run()), bits(first))


def test_scale_zero_is_the_plain_pipeline(case, pipe, plain):
    off = pipe(**sparse_kw(case), controlnet_conditioning_scale=0.0).frames
    assert torch.equal(off, plain)
    on = pipe(**sparse_kw(case)).frames
    d = S.rel_l2(on, plain)
    print(f"SPARSECTRL pipeline: scale 1 vs plain {d:.5f}, 3 x the UNet bar {3 * case['unet_bar']:.5f}")
    assert d > 3 * case["unet_bar"]


def test_ddim_run_matches_the_restatement(case, pipe, conditioning):
    c, v = case, case[True]
    _, cond, mask = conditioning
    scales = S.scale_row(5)
    with torch.no_grad():
        ref, emu = (S.ddim_loop(c["usd"], v["csd"], c["cfg"], v["ccfg"], c["lat"], c["ehs"], cond, mask, scales,
                                False, 3, G, act) for act in ("fp32", "bf16"))
    got = pipe(**sparse_kw(c)).frames
    e_emu, e_dev = S.rel_l2(emu, ref), S.rel_l2(got, ref)
    print(f"SPARSECTRL pipeline ddim: emulated {e_emu:.5f} device {e_dev:.5f} bar {1.3 * e_emu:.5f}")
    assert e_dev <= 1.3 * e_emu


def test_guess_mode_leaves_the_unconditional_half_alone(case, conditioning, monkeypatch):
    seen = []
    inject = ControlState.inject

    def spy(self, skips, mid, ctx):
        before = [a.t.clone() for a in [*skips, mid]]
        inject(self, skips, mid, ctx)
        seen.append((self, before, [a.t.clone() for a in [*skips, mid]]))

    monkeypatch.setattr(ControlState, "inject", spy)
    _, cond, mask = conditioning
    s = ddim()
    s.set_timesteps(3)
    ctl = SparseControlConditioning.from_tensors(case[True]["dcnet"], cond, mask, 1.0, True)
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


def test_lcm_and_dpm_runs_complete(case, vae, pipe):
    base = pipe(**sparse_kw(case)).frames
    for sched in (LCMScheduler.from_config(None, beta_schedule="linear"),
                  DPMSolverMultistepScheduler.from_config(DDIMScheduler().config)):
        p = AnimateDiffSparseControlNetPipeline(case["dunet"], case[True]["dcnet"], sched, vae=vae)
        p.torch_dtype = F32
        got = p(**sparse_kw(case, steps=4)).frames
        assert torch.isfinite(got).all() and not torch.equal(got, base)


def test_pixel_conditioning_runs_through_the_full_embedding(case):
    """The scribble variant: [0, 1] images at 8 x the latents, no VAE."""
    p = AnimateDiffSparseControlNetPipeline(case["dunet"], case[False]["dcnet"], ddim())
    imgs = case[False]["keys"][0].permute(1, 0, 2, 3)              # (K, 3, 64, 64)
    kw = dict(call_kw(case), conditioning_frames=imgs, controlnet_frame_indices=S.IDX)
    on = p(**kw).frames
    assert torch.isfinite(on).all()
    assert torch.equal(p(**kw, controlnet_conditioning_scale=0.0).frames,
                       AnimateDiffPipeline(case["dunet"], ddim())(**call_kw(case)).frames)


def test_refusals_on_the_device(case, pipe, conditioning):
    _, cond, mask = conditioning
    with pytest.raises(IndexError, match="out of bounds"):
        pipe(**dict(sparse_kw(case), controlnet_frame_indices=[0, 4]))
    with pytest.raises(ValueError, match="3 controlnet_frame_indices for 2 conditioning frames"):
        pipe(**dict(sparse_kw(case), controlnet_frame_indices=[0, 1, 2]))
    with pytest.raises(ValueError, match="asked for 16 x 16"):
        pipe(**dict(sparse_kw(case), conditioning_frames=torch.rand(2, 3, 64, 64)))
    no_enc = AnimateDiffSparseControlNetPipeline(case["dunet"], case[True]["dcnet"], ddim(),
                                                 vae=init_synthetic_(AutoencoderKL("tiny"), seed=0).to("cuda", BF))
    with pytest.raises(ValueError, match="VAE with its encoder"):
        no_enc(**sparse_kw(case))
    case["dunet"].enable_free_noise(context_length=2, context_stride=1)
    try:
        s = ddim()
        s.set_timesteps(2)
        ctl = SparseControlConditioning.from_tensors(case[True]["dcnet"], cond, mask)
        with pytest.raises(NotImplementedError, match="FreeNoise"):
            DenoiseLoop(case["dunet"], s, case["lat"], case["ehs"], G, control=ctl)
    finally:
        case["dunet"].disable_free_noise()
    assert pipe._control is None
