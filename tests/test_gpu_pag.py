"""Perturbed-attention guidance on the MI355X: the four step kernels under VD_STEP_PAG bit for bit
against tests/pag_ref.py run in torch fp32 on the CPU, inside poison-and-canary frames; the same
operands without the flag against the existing references; one PAG-applied spatial block and one
motion block against the restatement; and AnimateDiffPAGPipeline end to end on the tiny case
(2 frames of 8 x 8 latents): graph against eager while the adaptive scale changes and clamps, the
DDIM run against pag_ref's loop, LCM, DPM-Solver++, no CFG, FreeU, FreeInit, IP-Adapter, scale 0,
and the refused combinations.

Bars (none taken from the device):
  * the step kernels: equality;
  * the blocks: rel-L2 against the fp32 restatement <= 3 x the bf16-emulating restatement's own
    deviation (tests/test_gpu_controlnet.py's module bar), on a case where identity attention
    alone moves the output by more than 10 such bars (tests/test_pag_host.py asserts that);
  * the DDIM run: 1.3 x the bf16-emulating loop's rel-L2 (the ControlNet run test's bar).
"""
import pytest
import torch

import controlnet_ref as C
import memframe as mf
import pag_ref as R
import vdiff._lib as L
from vdiff import (AnimateDiffPAGPipeline, AnimateDiffPipeline, ControlNetConditioning, DDIMScheduler, DenoiseLoop,
                   DPMSolverMultistepScheduler, EulerDiscreteScheduler, LCMScheduler, PerturbedAttentionGuidance,
                   UNetMotionModel, ops)
from vdiff.models.blocks import Ctx
from vdiff.models.layers import Act, fmap_rows

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
G = 7.5
N = 5                                    # rows of the kernel tests' tables
SCALES = [0.25, 1.1, 2.7, 0.0, 0.505]    # step 2 reads 2.7, a step past the table the last entry


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def ddim(n=None):
    s = DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)
    if n is not None:
        s.set_timesteps(n)
    return s


def dpm(alg="dpmsolver++", n=None):
    s = DPMSolverMultistepScheduler.from_config(DDIMScheduler().config, algorithm_type=alg,
                                                use_karras_sigmas=alg == "dpmsolver++")
    if n is not None:
        s.set_timesteps(n)
    return s


# ---------------------------------------------------------------- 1. the step kernels
KINDS = ["ddim", "euler", "lcm", "dpm", "dpm_sde"]


@pytest.fixture(scope="module")
def tables():
    """5-row tables of every scheduler.  DPM: row 2 is second order, row 4 ("zero" final) first."""
    e = EulerDiscreteScheduler.from_config(None, timestep_spacing="linspace", beta_schedule="linear")
    e.set_timesteps(N)
    lc = LCMScheduler.from_config(None, beta_schedule="linear")
    lc.set_timesteps(N)
    out = dict(ddim=ddim(N).coefficient_table(ddim(N).timesteps), euler=e.coefficient_table(e.timesteps),
               lcm=lc.coefficient_table(lc.timesteps), dpm=dpm("dpmsolver++", N).coefficient_table(),
               dpm_sde=dpm("sde-dpmsolver++", N).coefficient_table())
    assert [tuple(out[k].shape) for k in KINDS] == [(N, 4), (N, 4), (N, 8), (N, 8), (N, 8)]
    assert [int(f) & 1 for f in out["dpm"][:, 7]] == [0, 1, 1, 1, 0] == [int(f) & 1 for f in out["dpm_sde"][:, 7]]
    assert out["lcm"][:, 6].tolist() == [1, 1, 1, 1, 0]
    return {k: v.float().contiguous() for k, v in out.items()}


STEP_OPS = dict(ddim=ops.ddim_cfg_step, euler=ops.euler_cfg_step, lcm=ops.lcm_cfg_step, dpm=ops.dpm_cfg_step,
                dpm_sde=ops.dpm_cfg_step)
# (B, C, F, H, W): 120 elements (one ragged block), 840 (four blocks, the last ragged), 1260 (five, ragged)
SHAPES = [(1, 4, 2, 3, 5), (2, 4, 3, 5, 7), (1, 4, 5, 7, 9)]


def operands(kind, table, shape, ncfg, step, slack, cuda, pag):
    """The framed operands of one call and the CPU values behind them."""
    B, Cc, Fr, H, W = shape
    rows, numel = B * Fr * H * W, B * Cc * Fr * H * W
    st = min(step, N - 1)
    g = torch.Generator().manual_seed(10000 * KINDS.index(kind) + 1000 * ncfg + 10 * numel + step)
    v = dict(eps=torch.randn(ncfg * rows, Cc, generator=g), lat=torch.randn(shape, generator=g),
             m1=torch.randn(shape, generator=g), noise=torch.randn(shape, generator=g), st=st, row=table[st])
    slabs = kind in ("lcm", "dpm_sde")
    body = torch.full((table.numel() + (N * numel if slabs else 0),), float("nan"))
    body[:table.numel()] = table.reshape(-1)
    if slabs:   # every slab NaN but the step's own
        body[table.numel() + st * numel:table.numel() + (st + 1) * numel] = v["noise"].reshape(-1)
    if pag:     # the scales: every entry NaN but the step's own, and NaN padding up to a multiple of 4
        buf = torch.full((ops.pag_prefix(N) + body.numel(),), float("nan"))
        buf[st] = SCALES[st]
        buf[ops.pag_prefix(N):] = body
    else:
        buf = body if slabs or kind in ("ddim", "euler") else table.clone()
    v["second"] = kind.startswith("dpm") and bool(int(table[st, 7]) & 1)
    v["noisy"] = kind == "dpm_sde" or (kind == "lcm" and float(table[st, 6]) != 0)
    f = {}
    f["eps"] = mf.load2d(v["eps"].to(cuda), col_slack=slack, name="eps")
    f["lat"] = mf.loadnd(v["lat"].to(cuda), name="latents")
    f["coef"] = mf.loadnd(buf.to(cuda), name="coef")
    f["x0"] = mf.framed_nd(shape, F32, cuda, name="x0_out")   # 0xFF: a NaN that must not be read ...
    if v["second"]:
        f["x0"][1].load(v["m1"].to(cuda))                      # ... but by a second-order DPM row
    f["next"] = mf.framed((ncfg * rows, 8), BF, cuda, name="next_in")
    return v, f


def check(kind, v, f, shape, ncfg, e, step):
    B, Cc, Fr, H, W = shape
    rows = B * Fr * H * W
    want, x0, nxt = R.step(kind.split("_")[0], e, v["lat"], v["row"], v["m1"] if v["second"] else None,
                           v["noise"] if v["noisy"] else None)
    xv, x0v, nv = f["lat"][0], f["x0"][0], f["next"][0]
    assert torch.isfinite(want).all() and torch.isfinite(x0).all() and torch.isfinite(xv).all()
    assert torch.equal(bits(xv), bits(want))
    assert torch.equal(bits(x0v), bits(x0))
    packed = nxt.permute(0, 2, 3, 4, 1).reshape(rows, Cc).to(BF)
    for h in range(ncfg):   # every copy of next_in, and its padding columns
        copy = nv[h * rows:(h + 1) * rows].cpu()
        assert torch.equal(bits(copy[:, :Cc]), bits(packed)), h
        assert (copy[:, Cc:].view(torch.int16) == 0).all(), h
    mf.assert_all_intact(*(fr for _, fr in f.values()))
    f["x0"][1].assert_written(x0)
    f["next"][1].assert_written()


@pytest.mark.parametrize("step", [2, 9], ids=["middle", "past_end"])
@pytest.mark.parametrize("slack", [0, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=["1x4x2x3x5", "2x4x3x5x7", "1x4x5x7x9"])
@pytest.mark.parametrize("ncfg", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_pag_step_matches_reference_bit_for_bit(cuda, tables, kind, ncfg, shape, slack, step):
    B, Cc, Fr, H, W = shape
    v, f = operands(kind, tables[kind], shape, ncfg, step, slack, cuda, pag=True)
    assert f["eps"][0].stride(0) == Cc + 2 * slack
    assert v["second"] == (kind.startswith("dpm") and step == 2)
    before = bits(f["coef"][0])
    sidx = torch.tensor([step], device=cuda, dtype=torch.int32)
    STEP_OPS[kind](f["eps"][0], ncfg, G, f["lat"][0], f["coef"][0], step_idx=sidx, x0_out=f["x0"][0],
                   next_in=f["next"][0], pag_n=N)
    torch.cuda.synchronize()
    e = v["eps"].reshape(ncfg, B, Fr, H, W, Cc).permute(0, 1, 5, 2, 3, 4)
    check(kind, v, f, shape, ncfg, R.combine(list(e), G, torch.tensor(SCALES, dtype=F32)[v["st"]]), step)
    assert torch.equal(bits(f["coef"][0]), before)   # scales, rows and slabs are read-only
    assert int(sidx.item()) == step


# ---------------------------------------------------------------- 2. without the flag
@pytest.mark.parametrize("ncfg", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_calls_without_the_flag_keep_their_bits(cuda, tables, kind, ncfg):
    """The operands of the PAG test, no flag: the one- and two-branch combine of the existing
    references (oracle.ddim_ref.cfg_combine's e_u + g (e_c - e_u)), every output bit for bit."""
    shape, step = SHAPES[1], 2
    B, Cc, Fr, H, W = shape
    v, f = operands(kind, tables[kind], shape, ncfg, step, 4, cuda, pag=False)
    sidx = torch.tensor([step], device=cuda, dtype=torch.int32)
    STEP_OPS[kind](f["eps"][0], ncfg, G, f["lat"][0], f["coef"][0], step_idx=sidx, x0_out=f["x0"][0],
                   next_in=f["next"][0])
    torch.cuda.synchronize()
    e = v["eps"].reshape(ncfg, B, Fr, H, W, Cc).permute(0, 1, 5, 2, 3, 4)
    e = e[0] + G * (e[1] - e[0]) if ncfg == 2 else e[0]
    check(kind, v, f, shape, ncfg, e, step)


def test_entry_point_refusals_with_device_operands(cuda, tables):
    """tests/test_pag_host.py's flag words with operands the entry point would otherwise take."""
    B, Cc, Fr, H, W = 1, 4, 2, 3, 5
    eps = torch.zeros(3 * Fr * H * W, Cc, device=cuda)
    lat = torch.ones(B, Cc, Fr, H, W, device=cuda)
    coef = ops.pag_coef(SCALES, tables["ddim"].to(cuda))
    stream = torch.cuda.current_stream().cuda_stream
    h, PAG = L.lib(), L.VD_STEP_PAG

    def call(fn, ncfg, coef_p=coef.data_ptr()):
        return fn(eps.data_ptr(), Cc, ncfg, 1.0, lat.data_ptr(), B, Cc, Fr, H, W, coef_p, N, None, None, None, 0, stream)
    for fn in (h.vd_ddim_cfg_step, h.vd_euler_cfg_step):
        assert call(fn, 1 | PAG) == L.VD_EINVAL
        assert call(fn, 4 | PAG) == L.VD_EINVAL
        assert call(fn, 3) == L.VD_EINVAL
        assert call(fn, 3 | PAG | 0x200) == L.VD_EINVAL
        assert call(fn, 3 | PAG, coef_p=coef.data_ptr() + 4) == L.VD_EINVAL
    torch.cuda.synchronize()
    assert (lat == 1).all()
    assert call(h.vd_ddim_cfg_step, 3 | PAG) == 0
    torch.cuda.synchronize()
    assert not (lat == 1).any() and torch.isfinite(lat).all()
    with pytest.raises(ValueError, match="PAG scales"):
        ops.pag_coef([1.0, float("nan")], tables["ddim"].to(cuda))
    with pytest.raises(ValueError, match="PAG scales in front of a table"):
        ops.ddim_cfg_step(eps, 3, 1.0, lat, ops.pag_coef(SCALES[:4], tables["ddim"].to(cuda)), pag_n=4)


# ---------------------------------------------------------------- 3. the blocks
@pytest.fixture(scope="module")
def case(cuda):
    """tests/pag_ref.py's case with the UNet on the device, the default layers marked."""
    c = dict(R.pag_case())
    d = UNetMotionModel("tiny")
    d.load_state_dict(c["unet"].state_dict())
    c["dunet"] = d.to(cuda, BF).prepare()
    assert c["dunet"].set_pag_applied_layers(R.DEFAULT_LAYERS) == c["layers"]
    return c


@pytest.mark.parametrize("kind", ["spatial", "motion"])
def test_pag_block_matches_the_restatement(case, kind):
    """3 videos of 3 frames at 5 x 3, the last video perturbed: its rows are to_out(V(norm(x))) of
    the restatement, the other videos' rows the plain block's."""
    b = R.block_case(kind)
    mid = case["dunet"].mid_block
    blk = mid.attentions[0] if kind == "spatial" else mid.motion_modules[0]
    n, k = b["batch"] * b["frames"], (b["batch"] - 1) * b["frames"]
    x = Act(fmap_rows(b["x"].cuda().to(BF)), n, b["h"], b["w"])
    ehs = b["ehs"].to("cuda", BF).reshape(b["batch"] * 77, -1)

    def run(pag_batch):
        ctx = Ctx(b["batch"], b["frames"], None, ehs, 77)
        ctx.pag_batch = pag_batch
        out = blk.run(x, ctx).t
        return out.float().cpu().view(n, b["h"], b["w"], -1).permute(0, 3, 1, 2)
    got, plain = run(1), run(0)
    torch.cuda.synchronize()
    e_kept, e_pert = C.rel_l2(got[:k], b["want"][:k]), C.rel_l2(got[k:], b["want"][k:])
    e_plain = C.rel_l2(plain, b["plain_fp32"])
    print(f"PAG block {kind}: kept {e_kept:.5f} (emulated {b['emulated_kept']:.5f}, bar {b['bar_kept']:.5f}) "
          f"perturbed {e_pert:.5f} (emulated {b['emulated_pert']:.5f}, bar {b['bar_pert']:.5f}) "
          f"plain {e_plain:.5f} separation {b['separation']:.5f}")
    assert torch.isfinite(got).all()
    assert b["separation"] >= 10 * max(b["bar_kept"], b["bar_pert"])
    assert 0 < max(b["bar_kept"], b["bar_pert"]) <= R.BAR_CEILING
    assert e_kept <= b["bar_kept"]
    assert e_pert <= b["bar_pert"]
    assert e_plain <= R.BAR_FACTOR * C.rel_l2(b["plain_bf16"], b["plain_fp32"])
    # and the device itself tells the two apart on the perturbed video
    assert C.rel_l2(got[k:], plain[k:]) > 5 * b["bar_pert"]


@pytest.mark.parametrize("h, w", [(4, 4), (5, 3)], ids=["kept_rows_fold", "kept_rows_leave_the_fold"])
def test_pag_spatial_block_where_norm1_folds_into_the_qkv_gemm(cuda, h, w):
    """A level-1 spatial block of the full config (320 channels, 8 heads of 40), whose norm1 folds
    into the QKV GEMM (LnFold): 3 videos of 2 frames, the last perturbed.  At 4 x 4 the kept rows
    (64) keep the fold and the perturbed rows take the norm and the plain V GEMM; at 5 x 3 the
    caller folds at 90 rows, the kept 60 rows do not, and the block normalises all of them."""
    from vdiff import init_synthetic_
    from vdiff.models.blocks import Transformer2DModel
    from oracle import unet_ref as U
    batch, frames, gain = 3, 2, R.TO_OUT_GAIN
    m = init_synthetic_(Transformer2DModel(8, 40, 320, 768, 32), seed=3)
    with torch.no_grad():
        m.transformer_blocks[0].attn1.to_out[0].weight.mul_(gain)
    sd = {f"m.{k}": v.detach().float() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(10 * h + w)
    n, k = batch * frames, (batch - 1) * frames
    x = torch.randn(n, 320, h, w, generator=g).to(BF).float()
    ehs = torch.randn(batch, 77, 768, generator=g).to(BF).float()
    ehs_img = ehs.repeat_interleave(frames, 0)
    with torch.no_grad():
        plain, plain_emu = (U.transformer2d(sd, "m", x, ehs_img, 8, 32, U.ROUNDERS[a]) for a in ("fp32", "bf16"))
        with R.identity_attention(["m.transformer_blocks.0.attn1"]):
            pert, pert_emu = (U.transformer2d(sd, "m", x, ehs_img, 8, 32, U.ROUNDERS[a]) for a in ("fp32", "bf16"))
    want = torch.cat([plain[:k], pert[k:]])
    bar_kept = R.BAR_FACTOR * C.rel_l2(plain_emu[:k], want[:k])
    bar_pert = R.BAR_FACTOR * C.rel_l2(pert_emu[k:], want[k:])
    assert C.rel_l2(pert[k:], plain[k:]) >= 10 * max(bar_kept, bar_pert) and max(bar_kept, bar_pert) <= R.BAR_CEILING
    d = m.to(cuda, BF)
    for sub in d.modules():
        if hasattr(sub, "prepare"):
            sub.prepare()
    blk = d.transformer_blocks[0]
    blk.attn1.pag = True
    M = n * h * w
    assert blk.fold(1, M) is not None
    print(f"PAG level-1 block {h}x{w}: fold at {M} rows yes, at the kept {M * k // n} rows "
          f"{'yes' if blk.fold(1, M * k // n) is not None else 'no'}")
    ctx = Ctx(batch, frames, None, ehs.to(cuda, BF).reshape(batch * 77, -1), 77)
    ctx.pag_batch = 1
    got = d.run(Act(fmap_rows(x.to(cuda, BF)), n, h, w), ctx).t.float().cpu().view(n, h, w, -1).permute(0, 3, 1, 2)
    e_kept, e_pert = C.rel_l2(got[:k], want[:k]), C.rel_l2(got[k:], want[k:])
    print(f"PAG level-1 block {h}x{w}: kept {e_kept:.5f} bar {bar_kept:.5f} perturbed {e_pert:.5f} bar {bar_pert:.5f}")
    assert e_kept <= bar_kept and e_pert <= bar_pert


# ---------------------------------------------------------------- 4. the pipeline
STEPS = 4
PAG_KW = dict(pag_scale=3.0, pag_adaptive_scale=0.005)   # over 4 DDIM steps: 1.755, 0.505, 0, 0


def call_kw(c, g=G, steps=STEPS):
    return dict(prompt_embeds=c["ehs"][1:2], negative_prompt_embeds=c["ehs"][0:1], latents=c["lat"], num_frames=2,
                height=64, width=64, num_inference_steps=steps, guidance_scale=g, output_type="latent")


@pytest.fixture(scope="module")
def pipe(case):
    return AnimateDiffPAGPipeline(case["dunet"], ddim())


@pytest.fixture(scope="module")
def plain(case):
    return AnimateDiffPipeline(case["dunet"], ddim())(**call_kw(case)).frames.clone()


@pytest.fixture(scope="module")
def adaptive(case, pipe):
    return pipe(**call_kw(case), **PAG_KW, use_graph=True).frames.clone()


def test_graph_equals_eager_while_the_scale_changes_and_clamps(case, pipe, plain, adaptive):
    eager = pipe(**call_kw(case), **PAG_KW, use_graph=False).frames
    assert torch.isfinite(adaptive).all()
    assert torch.equal(bits(adaptive), bits(eager))
    constant = pipe(**call_kw(case), pag_scale=3.0).frames
    assert not torch.equal(adaptive, constant) and not torch.equal(adaptive, plain)
    assert pipe.do_perturbed_attention_guidance and not pipe.do_pag_adaptive_scaling
    # the loop itself: three branches on one capture, the table the kernel reads, reset, reschedule
    s = ddim(STEPS)
    ehs3 = torch.cat([case["ehs"], case["ehs"][1:]])
    loop = DenoiseLoop(case["dunet"], s, case["lat"], ehs3, G, pag=PerturbedAttentionGuidance(**{
        "scale": PAG_KW["pag_scale"], "adaptive_scale": PAG_KW["pag_adaptive_scale"]})).prime()
    assert loop.graph is not None, loop.graph_error
    assert (loop.ncfg, loop.Bt, loop.x_in2.shape[0]) == (3, 3, 3 * 2 * 8 * 8)
    want = R.scale_table(3.0, 0.005, s.timesteps.tolist())
    assert want[1] > 0 and want[2] == 0 and torch.equal(loop.pag_tab.cpu(), want)
    first = loop.run().clone()
    assert int(loop.step_idx.item()) == STEPS and torch.equal(bits(first), bits(adaptive))
    loop.reset(case["lat"].cuda())
    assert torch.equal(bits(loop.run()), bits(first))
    s.set_timesteps(3)
    loop.reschedule(s.timesteps)
    assert torch.equal(loop.pag_tab[:3].cpu(), R.scale_table(3.0, 0.005, s.timesteps.tolist()))
    loop.reset(case["lat"].cuda())
    fresh = DenoiseLoop(case["dunet"], ddim(3), case["lat"], ehs3, G, use_graph=False,
                        pag=PerturbedAttentionGuidance(3.0, 0.005)).prime().run()
    assert torch.equal(bits(loop.run()), bits(fresh))


def test_ddim_run_matches_the_restatement(case, adaptive):
    c = case
    with torch.no_grad():
        ref, emu = (R.ddim_loop(c["usd"], c["cfg"], c["lat"], c["ehs"], STEPS, G, 3.0, 0.005, c["layers"], act)
                    for act in ("fp32", "bf16"))
        off = R.ddim_loop(c["usd"], c["cfg"], c["lat"], c["ehs"], STEPS, G, 0.0, 0.0, c["layers"])
    e_emu, e_dev = C.rel_l2(emu, ref), C.rel_l2(adaptive, ref)
    print(f"PIPELINE pag ddim (3.0, 0.005), 4 steps: emulated {e_emu:.5f} device {e_dev:.5f} bar {1.3 * e_emu:.5f} "
          f"(reference with PAG off is {C.rel_l2(off, ref):.5f} away)")
    assert 0 < e_emu < 0.1
    assert e_dev <= 1.3 * e_emu


def test_lcm_and_dpm_runs_complete(case, plain):
    outs = []
    for sched in (LCMScheduler.from_config(None, beta_schedule="linear"), dpm("dpmsolver++"), dpm("sde-dpmsolver++")):
        p = AnimateDiffPAGPipeline(case["dunet"], sched)
        p.torch_dtype = F32
        on = p(**call_kw(case), **PAG_KW, generator=torch.manual_seed(0)).frames.clone()
        off = p(**call_kw(case), pag_scale=0.0, generator=torch.manual_seed(0)).frames
        assert torch.isfinite(on).all() and not torch.equal(on, off)
        outs.append(on)
    assert not torch.equal(outs[1], outs[2])
    e = AnimateDiffPAGPipeline(case["dunet"], EulerDiscreteScheduler.from_config(
        None, timestep_spacing="linspace", beta_schedule="linear"))
    assert torch.isfinite(e(**call_kw(case), **PAG_KW).frames).all()


def test_run_without_cfg_has_two_branches(case, pipe):
    kw = call_kw(case, g=1.0)
    kw.pop("negative_prompt_embeds")
    got = pipe(**kw, **PAG_KW).frames.clone()
    eager = pipe(**kw, **PAG_KW, use_graph=False).frames
    off = AnimateDiffPipeline(case["dunet"], ddim())(**kw).frames
    assert torch.isfinite(got).all() and torch.equal(bits(got), bits(eager)) and not torch.equal(got, off)
    loop = DenoiseLoop(case["dunet"], ddim(STEPS), case["lat"], case["ehs"][[1, 1]], 1.0, use_graph=False,
                       pag=PerturbedAttentionGuidance(3.0, 0.005)).prime()
    assert (loop.ncfg, loop.Bt) == (2, 2)
    assert torch.equal(bits(loop.run()), bits(got))
    with torch.no_grad():
        c = case
        ref, emu = (R.ddim_loop(c["usd"], c["cfg"], c["lat"], c["ehs"], STEPS, 1.0, 3.0, 0.005, c["layers"], act)
                    for act in ("fp32", "bf16"))
    e_emu, e_dev = C.rel_l2(emu, ref), C.rel_l2(got, ref)
    print(f"PIPELINE pag ddim without CFG: emulated {e_emu:.5f} device {e_dev:.5f} bar {1.3 * e_emu:.5f}")
    assert e_dev <= 1.3 * e_emu


def test_freeu_free_init_and_ip_adapter_compose(cuda, case, pipe, adaptive):
    pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.5, b2=1.6)
    try:
        out = pipe(**call_kw(case), **PAG_KW).frames
        assert torch.isfinite(out).all() and not torch.equal(out, adaptive)
    finally:
        pipe.disable_freeu()
    # FreeInit's fast sampling runs a shorter schedule first: reschedule() refills the PAG scales
    pipe.enable_free_init(num_iters=2, use_fast_sampling=True)
    try:
        out = pipe(**call_kw(case), **PAG_KW, generator=torch.manual_seed(0)).frames
        assert torch.isfinite(out).all()
    finally:
        pipe.disable_free_init()
    assert torch.equal(bits(pipe(**call_kw(case), **PAG_KW).frames), bits(adaptive))
    from test_ip_adapter_host import synthetic_adapter
    p = AnimateDiffPAGPipeline.from_config("tiny", device=cuda, vae=None)
    kw = call_kw(case, steps=2)
    without = p(**kw, **PAG_KW).frames.clone()
    p.load_ip_adapter(synthetic_adapter(p.unet, n=4, clip_dim=48, scale=3.0))
    embeds = torch.randn(2, 1, 48, generator=torch.Generator().manual_seed(2))
    with_ip = p(**kw, **PAG_KW, ip_adapter_image_embeds=embeds).frames
    assert torch.isfinite(with_ip).all() and not torch.equal(with_ip, without)


# ---------------------------------------------------------------- 5. scale 0
def test_scale_zero_is_the_plain_pipeline(case, pipe):
    kw = call_kw(case)
    kw.pop("latents")
    base = AnimateDiffPipeline(case["dunet"], ddim())
    want = base(**kw, generator=torch.manual_seed(11)).frames.clone()
    got = pipe(**kw, pag_scale=0.0, generator=torch.manual_seed(11)).frames
    assert torch.equal(bits(got), bits(want))
    assert not pipe.do_perturbed_attention_guidance
    on = pipe(**kw, pag_scale=3.0, generator=torch.manual_seed(11)).frames
    assert not torch.equal(on, want)
    # the marks alone change nothing: the plain pipeline on the marked UNet, after a PAG run
    assert case["dunet"].pag_applied_layers() == case["layers"]
    assert torch.equal(bits(base(**kw, generator=torch.manual_seed(11)).frames), bits(want))


# ---------------------------------------------------------------- 6. refusals
def test_refused_combinations(case, pipe):
    pag = PerturbedAttentionGuidance(3.0)
    ehs3 = torch.cat([case["ehs"], case["ehs"][1:]])
    with pytest.raises(NotImplementedError, match="cfg_shard"):
        DenoiseLoop(case["dunet"], ddim(STEPS), case["lat"], ehs3, G, cfg_shard=object(), pag=pag)
    control = ControlNetConditioning(C.tiny_case()["cnet"], C.tiny_case()["cond"])
    with pytest.raises(NotImplementedError, match="ControlNet"):
        DenoiseLoop(case["dunet"], ddim(STEPS), case["lat"], ehs3, G, control=control, pag=pag)
    pipe.dist = object()   # any frame shard: refused before it is used
    try:
        with pytest.raises(NotImplementedError, match="dist="):
            pipe(**call_kw(case), **PAG_KW)
    finally:
        pipe.dist = None
    pipe.enable_free_noise(context_length=2, context_stride=1)
    try:
        with pytest.raises(NotImplementedError, match="FreeNoise"):
            pipe(**call_kw(case), **PAG_KW)
        with pytest.raises(NotImplementedError, match="FreeNoise"):
            DenoiseLoop(case["dunet"], ddim(STEPS), case["lat"], ehs3, G, pag=pag)
    finally:
        pipe.disable_free_noise()
    with pytest.raises(ValueError, match="prompt_embeds batch"):
        DenoiseLoop(case["dunet"], ddim(STEPS), case["lat"], case["ehs"], G, pag=pag)
    case["dunet"].set_pag_applied_layers(None)
    try:
        with pytest.raises(ValueError, match="set_pag_applied_layers"):
            DenoiseLoop(case["dunet"], ddim(STEPS), case["lat"], ehs3, G, pag=pag)
    finally:
        case["dunet"].set_pag_applied_layers(R.DEFAULT_LAYERS)
