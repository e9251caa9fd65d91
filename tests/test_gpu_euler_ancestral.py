"""The Euler-ancestral step on the MI355X: the kernel (vd_euler_cfg_step with VD_STEP_ANCESTRAL) bit
for bit against tests/euler_ancestral_ref.py run in torch fp32 on the CPU, inside poison-and-canary
frames, with NaN in every slab a row must not read; an Euler table under the flag against the
unflagged kernel; the VD_EINVAL table; EulerAncestralDiscreteScheduler.step's chain; DenoiseLoop
eagerly, on the captured graph, after reset and reschedule; the tiny-UNet loop against
oracle/unet_ref.py's blocks driven through the reference loop; and the five pipelines.

Bars (none taken from the code under test): equality everywhere but the oracle check.  There the
existing Euler loop test's measure is kept (rel-L2 of the final latents against the fp32 oracle),
but its bar of 1 % belongs to the first 3 of 25 steps, where the sample is still the initial noise
at sigma ~ 14 and the UNet's bf16 error is a small part of it; it does not transfer to a whole
4-step schedule that ends on the x0 prediction itself.  So plain Euler's error on the identical
config is measured against the oracle in the same test, and the stochastic loop is allowed 1.5
times it: the added noise is identical on both sides and contributes no error of its own, the
factor covers the two extra fp32 operations per element.  Both figures are printed.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import euler_ancestral_ref as R
import memframe as mf
import vdiff._lib as L
from vdiff import (AnimateDiffControlNetPipeline, AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline, DDIMScheduler,
                   DenoiseLoop, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, UNetMotionModel,
                   init_synthetic_, ops)
from vdiff.pipeline import randn_tensor

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
F32, BF = torch.float32, torch.bfloat16
N_STEPS = 4
G = 2.0
NAN = float("nan")
A = L.VD_STEP_ANCESTRAL


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def sched(n=N_STEPS, cls=EulerAncestralDiscreteScheduler, **kw):
    s = cls.from_config(DDIMScheduler().config, timestep_spacing="linspace", beta_schedule="linear", **kw)
    if n is not None:
        s.set_timesteps(n)
    return s


# ---------------------------------------------------------------- the kernel
N_TAB = 5


@pytest.fixture(scope="module")
def table():
    """The restatement's 5-step table (the scheduler's own agrees bit for bit, tests/test_euler_ancestral_host.py)."""
    _, sig = R.set_timesteps(N_TAB, acp=R.alphas_cumprod(beta_start=0.00085, beta_end=0.012))
    tab = R.table(sig)
    assert torch.equal(tab, sched(N_TAB).coefficient_table())
    assert (tab[:-1, 3] > 0).all() and tab[-1].tolist() == [float(sig[-2]), 0.0, 1.0, 0.0]
    return tab


# (B, C, F, H, W), eps column slack (ld_eps = C + 2 * slack): one element per channel; 120 elements
# (not a multiple of any vector width, half a block); 7752 elements (31 blocks, the last ragged); and
# 840 elements with ld_eps = 8 > C.  cpad is 8 everywhere (4 zero padding columns).
SHAPES = [((1, 4, 1, 1, 1), 0), ((1, 4, 2, 3, 5), 0), ((2, 4, 3, 17, 19), 0), ((2, 4, 3, 5, 7), 2)]
SHAPE_IDS = ["1x4x1x1x1", "1x4x2x3x5", "2x4x3x17x19", "2x4x3x5x7_ld8"]
STEPS = [0, 2, 4, 9]
STEP_IDS = ["first", "middle", "last", "past_end"]
BRANCHES = [(1, False), (2, False), (2, True), (3, True)]
BRANCH_IDS = ["ncfg1", "ncfg2", "pag2", "pag3"]
SCALES = [3.0, 2.5, 0.0, 1.25, 0.5]


def guided(eps, ncfg, pag, shape, scale):
    """The guided eps in latent layout, one fp32 torch op at a time (include/vdiff.h)."""
    B, C, Fr, H, W = shape
    e = eps.reshape(ncfg, B, Fr, H, W, C).permute(0, 1, 5, 2, 3, 4)
    if pag:
        return R.pag_combine(list(e), torch.tensor(G), torch.tensor(scale))
    return e[0] if ncfg == 1 else R.cfg_combine(e[0], e[1], torch.tensor(G))


def framed_call(cuda, shape, slack, ncfg, pag, tab, step, eps, lat, slabs, flagged=True):
    """One launch with every operand framed -> (latents, x0_out, next_in) on the CPU, after the
    frame checks: nothing stored outside the three outputs, all of them written, coef untouched."""
    B, C, Fr, H, W = shape
    cpad, n = 8, len(tab)
    rows = B * Fr * H * W
    ev, fe = mf.load2d(eps.to(cuda), col_slack=slack, name="eps")   # the slack columns are NaN
    assert ev.stride(0) == C + 2 * slack
    xv, fx = mf.loadnd(lat.to(cuda), name="latents")
    body = torch.cat([tab.reshape(-1), slabs.reshape(-1)]) if flagged else tab.reshape(-1)
    coef = ops.pag_coef(SCALES[:n], body) if pag else body.clone()
    cv, fc = mf.loadnd(coef.to(cuda), name="coef")                  # behind the last slab: the frame's poison
    before = bits(cv)
    x0v, f0 = mf.framed_nd(shape, F32, cuda, name="x0_out")
    nv, fn = mf.framed((ncfg * rows, cpad), BF, cuda, name="next_in")  # pre-filled with 0xFF
    sidx = torch.tensor([step], device=cuda, dtype=torch.int32)
    if flagged:
        ops.euler_ancestral_cfg_step(ev, ncfg, G, xv, cv, step_idx=sidx, x0_out=x0v, next_in=nv, pag_n=n if pag else 0)
    else:
        ops.euler_cfg_step(ev, ncfg, G, xv, cv if pag else cv.view(n, 4), step_idx=sidx, x0_out=x0v, next_in=nv,
                           pag_n=n if pag else 0)
    torch.cuda.synchronize()
    mf.assert_all_intact(fe, fx, fc, f0, fn)
    f0.assert_written()
    fn.assert_written()
    assert torch.equal(bits(cv), before)  # rows and slabs are read-only
    assert int(sidx.item()) == step
    return xv.cpu(), x0v.cpu(), nv.cpu()


@pytest.mark.parametrize("step", STEPS, ids=STEP_IDS)
@pytest.mark.parametrize("ncfg, pag", BRANCHES, ids=BRANCH_IDS)
@pytest.mark.parametrize("shape, slack", SHAPES, ids=SHAPE_IDS)
def test_kernel_matches_reference_bit_for_bit(cuda, table, shape, slack, ncfg, pag, step):
    B, C, Fr, H, W = shape
    rows = B * Fr * H * W
    st = min(step, N_TAB - 1)
    last = st == N_TAB - 1
    g = torch.Generator().manual_seed(1000 * pag + 100 * ncfg + 10 * B + step)
    eps = torch.randn(ncfg * rows, C, generator=g)
    lat = torch.randn(shape, generator=g) * table[st, 0]
    noise = torch.randn(shape, generator=g)
    # every slab NaN but the step's own — and on the last step, whose sigma_up is 0, that one too
    slabs = torch.full((N_TAB,) + shape, NAN)
    if not last:
        slabs[st] = noise
    got, x0, nxt = framed_call(cuda, shape, slack, ncfg, pag, table, step, eps, lat, slabs)

    e = guided(eps, ncfg, pag, shape, SCALES[st])
    want, want0, want_in = R.step(e, lat, table[st], noise)
    assert torch.isfinite(want).all() and torch.isfinite(want0).all()
    if not last:
        assert not torch.equal(want, R.step(e, lat, table[st], torch.zeros_like(noise))[0])  # the noise matters
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(x0), bits(want0))
    packed = want_in.permute(0, 2, 3, 4, 1).reshape(rows, C).to(BF)
    for h in range(ncfg):
        half = nxt[h * rows:(h + 1) * rows]
        assert torch.equal(bits(half[:, :C]), bits(packed))
        assert (half[:, C:].view(torch.int16) == 0).all()


@pytest.mark.parametrize("step", [0, 4], ids=["first", "last"])
@pytest.mark.parametrize("ncfg, pag", [(2, False), (3, True)], ids=["ncfg2", "pag3"])
def test_euler_table_under_the_flag_is_the_euler_kernel(cuda, ncfg, pag, step):
    """sigma_down = sigma_next and slot 3 = 0: no slab is read (all NaN), and the result is the
    unflagged kernel's bit for bit."""
    shape, slack = (2, 4, 3, 5, 7), 2
    tab = sched(N_TAB, EulerDiscreteScheduler).coefficient_table()
    assert not tab[:, 3].any()
    g = torch.Generator().manual_seed(7 + step)
    eps = torch.randn(ncfg * 2 * 3 * 5 * 7, 4, generator=g)
    lat = torch.randn(shape, generator=g) * tab[step, 0]
    slabs = torch.full((N_TAB,) + shape, NAN)
    flagged = framed_call(cuda, shape, slack, ncfg, pag, tab, step, eps, lat, slabs)
    plain = framed_call(cuda, shape, slack, ncfg, pag, tab, step, eps, lat, slabs, flagged=False)
    for a, b in zip(flagged, plain):
        assert torch.isfinite(a.float()).all() and torch.equal(bits(a), bits(b))


def test_last_step_of_a_real_schedule_ignores_its_slab(cuda, table):
    shape = (1, 4, 2, 3, 5)
    g = torch.Generator().manual_seed(11)
    eps = torch.randn(2 * 3 * 5, 4, generator=g)
    lat = torch.randn(shape, generator=g) * table[-1, 0]
    got, x0, nxt = framed_call(cuda, shape, 0, 1, False, table, N_TAB - 1, eps, lat, torch.full((N_TAB,) + shape, NAN))
    e = guided(eps, 1, False, shape, 0.0)
    want, want0, _ = R.step(e, lat, table[-1], None)
    assert torch.isfinite(x0).all() and torch.isfinite(got).all() and torch.isfinite(nxt.float()).all()
    assert torch.equal(bits(x0), bits(want0)) and torch.equal(bits(got), bits(want))
    assert torch.equal(bits(x0), bits(lat - table[-1, 0] * e))


def test_einval_table_leaves_the_outputs_untouched(cuda):
    B, C, Fr, H, W = 1, 4, 2, 8, 8
    n = B * C * Fr * H * W
    eps = torch.zeros(3 * Fr * H * W, C, device=cuda)
    lat = torch.ones(B, C, Fr, H, W, device=cuda)
    x0 = torch.full_like(lat, 2.0)
    nxt = torch.full((3 * Fr * H * W, 8), 3.0, device=cuda, dtype=BF)
    # 4 scales, then one row and one slab: valid with or without VD_STEP_PAG, 16-byte aligned either way
    coef = torch.ones(4 + ops.euler_a_buffer_numel(1, n) + 4, device=cuda)
    assert coef.data_ptr() % 16 == 0
    keep = [t.clone() for t in (lat, x0, nxt)]

    def call(fn, ncfg, off=0):
        return fn(eps.data_ptr(), C, ncfg, 1.0, lat.data_ptr(), B, C, Fr, H, W, coef.data_ptr() + off, 1, None,
                  x0.data_ptr(), nxt.data_ptr(), 8, None)
    h = L.lib()
    cases = []
    for low in (1, 2):
        for bit in (L.VD_STEP_LCM, L.VD_STEP_DPM, L.VD_STEP_UNIPC, 0x200, 0x1000):
            cases.append((h.vd_euler_cfg_step, low | A | bit, 0))
        cases.append((h.vd_ddim_cfg_step, low | A, 0))
        cases.append((h.vd_euler_cfg_step, low | A, 4))          # misaligned coef
        cases.append((h.vd_euler_cfg_step, low | A, 8))
    cases.append((h.vd_euler_cfg_step, 3 | A, 0))                # low byte 3 without PAG
    cases.append((h.vd_euler_cfg_step, 1 | A | L.VD_STEP_PAG, 0))  # low byte 1 with it
    cases.append((h.vd_euler_cfg_step, 3 | A | L.VD_STEP_PAG | L.VD_STEP_LCM, 0))
    cases.append((h.vd_euler_cfg_step, 3 | A | L.VD_STEP_PAG, 4))
    for fn, ncfg, off in cases:
        assert call(fn, ncfg, off) == L.VD_EINVAL, (fn.__name__ if hasattr(fn, "__name__") else fn, hex(ncfg), off)
    torch.cuda.synchronize()
    for t, k in zip((lat, x0, nxt), keep):
        assert torch.equal(t, k)
    # the wrapper checks the size the library cannot see
    with pytest.raises(ValueError, match="not a multiple"):
        ops.euler_ancestral_cfg_step(eps[:Fr * H * W], 1, 1.0, lat, coef[:4 + n + 1])
    with pytest.raises(ValueError, match="PAG scales in front"):
        ops.euler_ancestral_cfg_step(eps, 3, 1.0, lat, torch.ones(4 + 2 * (4 + n), device=cuda), pag_n=1)
    assert torch.equal(lat, keep[0])
    # and the accepted calls do write: the flag alone (x0 = 1 - 1 * 0, x = 1 + 0 * 0 + 1 * 1), and with PAG
    assert call(h.vd_euler_cfg_step, 2 | A) == L.VD_OK
    torch.cuda.synchronize()
    assert (x0 == 1).all() and (lat == 2).all()
    assert call(h.vd_euler_cfg_step, 3 | A | L.VD_STEP_PAG) == L.VD_OK
    torch.cuda.synchronize()
    assert (x0 == 2).all() and (lat == 3).all()


# ---------------------------------------------------------------- scheduler.step
def test_scheduler_step_chain_equals_the_reference_loop(cuda):
    n = 6
    s = sched(n)
    _, sig = R.set_timesteps(n, acp=R.alphas_cumprod(beta_start=0.00085, beta_end=0.012))
    tab = R.table(sig)
    g = torch.Generator().manual_seed(5)
    shape = (1, 4, 3, 5, 7)
    x = torch.randn(shape, generator=g) * s.init_noise_sigma
    eps = [torch.randn(shape, generator=g) for _ in range(n)]
    gen, twin = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    draws = [randn_tensor(shape, twin, device="cuda", dtype=F32).cpu() for _ in range(n)]
    want, want0 = R.loop(x, eps, draws, tab)
    y = x.cuda()
    for i, t in enumerate(s.timesteps):
        state = gen.get_state()
        out = s.step(eps[i].cuda(), t, y, generator=gen)
        assert not torch.equal(gen.get_state(), state)  # every step draws, the last included
        assert torch.equal(bits(out.pred_original_sample), bits(want0[i]))
        y = out.prev_sample
    assert s.step_index == n and torch.equal(gen.get_state(), twin.get_state())
    assert torch.equal(bits(y), bits(want))
    s.set_timesteps(n)
    first = s.step(eps[0].cuda(), s.timesteps[0], x.cuda(), generator=torch.Generator().manual_seed(9), return_dict=False)
    assert isinstance(first, tuple) and torch.equal(bits(first[0]), bits(R.step(eps[0], x, tab[0], draws[0])[0]))


# ---------------------------------------------------------------- loop
@pytest.fixture(scope="module")
def tiny(cuda):
    """The tiny UNet and the golden inputs cut to 2 frames x 32^2; two fixed sets of step noise."""
    unet = init_synthetic_(UNetMotionModel("tiny"), seed=0).to("cuda", BF).prepare()
    g = np.load(GOLD / "tiny_unet.npz")
    lat = torch.from_numpy(g["latents"])[:, :, :2, :32, :32].contiguous().cuda() * sched().init_noise_sigma
    ehs = torch.from_numpy(g["ehs"]).cuda()
    gen = torch.Generator().manual_seed(3)
    noise = [torch.stack([randn_tensor(lat.shape, gen, device="cuda", dtype=F32) for _ in range(N_STEPS)])
             for _ in range(2)]
    return dict(unet=unet, lat=lat, ehs=ehs, noise=noise[0], other=noise[1])


@pytest.fixture(scope="module")
def eager(tiny):
    """The eager 4-step loop with each noise set, computed once."""
    out = {}
    for k in ("noise", "other"):
        loop = DenoiseLoop(tiny["unet"], sched(), tiny["lat"], tiny["ehs"], G, use_graph=False, step_noise=tiny[k]).prime()
        assert loop.graph is None
        out[k] = loop.run().clone()
    assert torch.isfinite(out["noise"]).all() and not torch.equal(out["noise"], out["other"])
    return out


def test_eager_loop_equals_unet_plus_scheduler_step(tiny, eager):
    s = sched()
    gen = torch.Generator().manual_seed(3)  # the stream tiny["noise"] was drawn from
    x = tiny["lat"]
    for t in s.timesteps:
        xi = s.scale_model_input(torch.cat([x, x]), t)
        u, c = tiny["unet"](xi, t, encoder_hidden_states=tiny["ehs"]).sample.chunk(2)
        x = s.step(u + G * (c - u), t, x, generator=gen).prev_sample
    assert torch.equal(bits(x), bits(eager["noise"]))


def test_graph_replay_reset_and_reschedule(tiny, eager):
    loop = DenoiseLoop(tiny["unet"], sched(), tiny["lat"], tiny["ehs"], G, use_graph=True, step_noise=tiny["noise"]).prime()
    assert loop.graph is not None, loop.graph_error
    assert loop.noise_slabs.shape == (N_STEPS,) + tuple(tiny["lat"].shape) and loop.coef_rows.shape == (N_STEPS, 4)
    assert loop.coef.numel() == ops.euler_a_buffer_numel(N_STEPS, tiny["lat"].numel())
    assert loop.noise_slabs.data_ptr() == loop.coef.data_ptr() + 4 * 4 * N_STEPS
    assert torch.equal(bits(loop.run()), bits(eager["noise"]))
    assert int(loop.step_idx.item()) == N_STEPS
    loop.reset(tiny["lat"], step_noise=tiny["other"])
    assert torch.equal(bits(loop.run()), bits(eager["other"]))  # same capture, other noise
    loop.reset(tiny["lat"])  # None keeps the slabs
    assert torch.equal(bits(loop.run()), bits(eager["other"]))
    with pytest.raises(RuntimeError, match="scheduled steps"):
        loop.run(1)
    # fewer steps on the same capture: a 3-step schedule's rows and noise in the tables' prefix
    s3 = sched(3)
    loop.scheduler = s3
    loop.reschedule(s3.timesteps)
    loop.reset(tiny["lat"], step_noise=tiny["noise"][:3])
    got = loop.run().clone()
    assert int(loop.step_idx.item()) == 3
    fresh = DenoiseLoop(tiny["unet"], sched(3), tiny["lat"], tiny["ehs"], G, use_graph=False,
                        step_noise=tiny["noise"][:3]).prime().run()
    assert torch.equal(bits(got), bits(fresh))


def test_loop_refusals(tiny):
    u, lat, ehs = tiny["unet"], tiny["lat"], tiny["ehs"]
    with pytest.raises(ValueError, match="needs step_noise"):
        DenoiseLoop(u, sched(), lat, ehs, G)
    with pytest.raises(ValueError, match="step_noise of shape"):
        DenoiseLoop(u, sched(), lat, ehs, G, step_noise=tiny["noise"][:3])  # one slab per step, the last included
    with pytest.raises(ValueError, match="step_noise of shape"):
        DenoiseLoop(u, sched(), lat, ehs, G, step_noise=tiny["noise"][:, :, :, :1])
    with pytest.raises(ValueError, match="LCM scheduler"):
        DenoiseLoop(u, sched(cls=EulerDiscreteScheduler), lat, ehs, G, step_noise=tiny["noise"])


def test_tiny_loop_matches_the_oracle():
    """4 steps, CFG 7.5, on tests/controlnet_ref.py's tiny case (2 frames of 8 x 8 latents) against
    oracle/unet_ref.py's blocks in fp32 driven through the reference loop with the same noise; the
    bar is 1.5 x plain Euler's error on the identical config (module docstring)."""
    import controlnet_ref as C
    c = C.tiny_case()
    g = 7.5
    dunet = UNetMotionModel("tiny")
    dunet.load_state_dict(c["unet"].state_dict())
    dunet = dunet.to("cuda", BF).prepare()
    acp = R.alphas_cumprod(beta_start=0.00085, beta_end=0.012)
    ts, sig = R.set_timesteps(N_STEPS, acp=acp)
    x = c["lat"].float() * R.init_noise_sigma(sig)
    gen = torch.Generator().manual_seed(21)
    noise = [torch.randn(x.shape, generator=gen) for _ in range(N_STEPS)]

    def unet_fn(x_in, t):
        return C.unet_forward_residuals(c["usd"], c["cfg"], x_in, t, c["ehs"], None, "fp32")
    with torch.no_grad():
        want_a = R.denoise_loop(unet_fn, x, sig, ts, noise, g)
        euler_tab = torch.stack([sig[:-1], sig[1:], R._sqrt(sig[1:] ** 2 + 1), torch.zeros(N_STEPS)], 1)
        want_e = R.denoise_loop(unet_fn, x, sig, ts, [None] * N_STEPS, g, tab=euler_tab)
    s = sched()
    assert torch.equal(s.sigmas, sig)
    got_a = DenoiseLoop(dunet, s, x, c["ehs"], g, step_noise=torch.stack(noise)).prime().run()
    got_e = DenoiseLoop(dunet, sched(cls=EulerDiscreteScheduler), x, c["ehs"], g).prime().run()
    e_a, e_e = C.rel_l2(got_a, want_a), C.rel_l2(got_e, want_e)
    print(f"LOOP 4 steps vs oracle: euler ancestral {e_a:.5f} euler {e_e:.5f} bar {1.5 * e_e:.5f}")
    assert torch.isfinite(got_a).all() and not torch.equal(want_a, want_e)
    assert 0 < e_e < 0.1
    assert e_a <= 1.5 * e_e


# ---------------------------------------------------------------- pipelines
def call_kw(tiny):
    neg, pos = tiny["ehs"].chunk(2)
    return dict(prompt_embeds=pos, negative_prompt_embeds=neg, num_frames=2, height=256, width=256,
                num_inference_steps=N_STEPS, guidance_scale=G, output_type="latent")


@pytest.fixture(scope="module")
def pipe(tiny):
    p = AnimateDiffPipeline(tiny["unet"], sched(None))
    p.torch_dtype = F32  # the noise dtype; fp32 so that scheduler.step's own draws are the same stream
    return p


def test_text_to_video_is_reproducible_draws_in_diffusers_order_and_differs_from_euler(tiny, pipe):
    got = pipe(**call_kw(tiny), generator=torch.manual_seed(0)).frames.clone()
    again = pipe(**call_kw(tiny), generator=torch.manual_seed(0)).frames
    assert torch.isfinite(got).all() and torch.equal(bits(got), bits(again))
    other = pipe(**call_kw(tiny), generator=torch.manual_seed(1)).frames
    assert not torch.equal(got, other)
    # diffusers' loop by hand: the latents, then one draw inside every scheduler.step
    gen = torch.manual_seed(0)
    s = sched()
    x = randn_tensor((1, 4, 2, 32, 32), gen, device="cuda", dtype=F32) * s.init_noise_sigma
    for t in s.timesteps:
        xi = s.scale_model_input(torch.cat([x, x]), t)
        u, c = tiny["unet"](xi, t, encoder_hidden_states=tiny["ehs"]).sample.chunk(2)
        x = s.step(u + G * (c - u), t, x, generator=gen).prev_sample
    assert torch.equal(bits(got), bits(x))
    euler = AnimateDiffPipeline(tiny["unet"], sched(None, EulerDiscreteScheduler))
    euler.torch_dtype = F32
    plain = euler(**call_kw(tiny), generator=torch.manual_seed(0)).frames
    assert torch.isfinite(plain).all() and not torch.equal(got, plain)


def test_video_to_video_runs_the_cut_schedule(tiny):
    """strength 0.5 of 4 steps: add_noise at the third timestep, then the last two steps and two draws."""
    v2v = AnimateDiffVideoToVideoPipeline.from_config("tiny", scheduler=sched(None))
    kw = call_kw(tiny)
    kw.pop("num_frames")
    clean = tiny["lat"] / sched().init_noise_sigma
    got = v2v(**kw, latents=clean, strength=0.5, generator=torch.manual_seed(0)).frames
    s = sched()
    ts = s.timesteps[2:]
    assert len(ts) == 2
    gen = torch.manual_seed(0)
    noise = torch.stack([randn_tensor(clean.shape, gen, device="cuda", dtype=v2v.torch_dtype) for _ in range(2)]).float()
    want = DenoiseLoop(v2v.unet, s, clean, tiny["ehs"], G, timesteps=ts, use_graph=False,
                       step_noise=noise).prime().run()
    assert torch.isfinite(got).all() and torch.equal(bits(got), bits(want))


def test_free_init_draws_each_iteration_after_the_filter(tiny, pipe):
    pipe.enable_free_init(num_iters=2)
    try:
        got = pipe(**call_kw(tiny), generator=torch.manual_seed(0)).frames
        gen = torch.manual_seed(0)
        x = randn_tensor((1, 4, 2, 32, 32), gen, device="cuda", dtype=F32) * sched().init_noise_sigma
        for i in range(2):
            x, ts = pipe._apply_free_init(x, i, N_STEPS, gen)       # iteration 1 draws z_rand here
            noise = torch.stack([randn_tensor(x.shape, gen, device="cuda", dtype=F32) for _ in range(N_STEPS)])
            x = DenoiseLoop(tiny["unet"], pipe.scheduler, x, tiny["ehs"], G, timesteps=ts, use_graph=False,
                            step_noise=noise).prime().run().clone()
        assert torch.isfinite(got).all() and torch.equal(bits(got), bits(x))
    finally:
        pipe.disable_free_init()
        pipe._free_init_initial_noise = pipe._free_init_table = pipe._free_init_scratch = None


def test_pag_pipeline_runs_three_branches_on_the_graph(cuda):
    """The PAG scales sit in front of the 4-float rows and the slabs behind them."""
    import pag_ref as P
    from vdiff import AnimateDiffPAGPipeline
    c = P.pag_case()
    dunet = UNetMotionModel("tiny")
    dunet.load_state_dict(c["unet"].state_dict())
    dunet = dunet.to(cuda, BF).prepare()
    assert dunet.set_pag_applied_layers(P.DEFAULT_LAYERS) == c["layers"]
    kw = dict(prompt_embeds=c["ehs"][1:2], negative_prompt_embeds=c["ehs"][0:1], latents=c["lat"], num_frames=2,
              height=64, width=64, num_inference_steps=4, guidance_scale=7.5, output_type="latent")
    pag = dict(pag_scale=3.0, pag_adaptive_scale=0.005)
    p = AnimateDiffPAGPipeline(dunet, sched(None))
    on = p(**kw, **pag, generator=torch.manual_seed(2)).frames.clone()
    eager = p(**kw, **pag, generator=torch.manual_seed(2), use_graph=False).frames.clone()
    off = p(**kw, pag_scale=0.0, generator=torch.manual_seed(2)).frames.clone()
    plain = AnimateDiffPipeline(dunet, sched(None))(**kw, generator=torch.manual_seed(2)).frames
    assert torch.isfinite(on).all()
    assert torch.equal(bits(on), bits(eager))
    assert torch.equal(bits(off), bits(plain)) and not torch.equal(on, off)


def test_controlnet_and_sparsectrl_pipelines_take_the_scheduler(cuda, tiny):
    from vdiff import AnimateDiffSparseControlNetPipeline
    p = AnimateDiffControlNetPipeline.from_config("tiny", device=cuda, vae=None, scheduler=sched(None))
    neg, pos = tiny["ehs"].chunk(2)
    lat = (tiny["lat"][:, :, :, :8, :8] / sched().init_noise_sigma).contiguous()
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat, num_frames=2, height=64, width=64,
              num_inference_steps=4, guidance_scale=G, output_type="latent")
    frames = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    plain = AnimateDiffPipeline(p.unet, sched(None))
    plain.torch_dtype = p.torch_dtype  # the step noise is drawn in it
    want = plain(**kw, generator=torch.manual_seed(4)).frames.clone()
    off = p(**kw, conditioning_frames=frames, controlnet_conditioning_scale=0.0, generator=torch.manual_seed(4)).frames
    assert torch.isfinite(want).all() and torch.equal(off, want)
    on = p(**kw, conditioning_frames=frames, generator=torch.manual_seed(4)).frames
    assert torch.isfinite(on).all() and not torch.equal(on, want)

    sp = AnimateDiffSparseControlNetPipeline.from_config("tiny", device=cuda, scheduler=sched(None))
    g = torch.Generator().manual_seed(11)
    lat4 = torch.randn(1, 4, 4, 8, 8, generator=g)
    ehs = torch.randn(2, 77, sp.unet.config["cross_attention_dim"], generator=g)
    kw = dict(prompt_embeds=ehs[1:2], negative_prompt_embeds=ehs[0:1], latents=lat4, num_frames=4, height=64, width=64,
              num_inference_steps=4, guidance_scale=G, output_type="latent")
    sparse = dict(conditioning_frames=torch.rand(2, 3, 16, 16, generator=g), controlnet_frame_indices=[0, 3])
    # the key frames' posterior is sampled on the call's generator before the step noise, so a plain
    # pipeline on the same seed adds other noise: the graph is held to the eager run instead
    on = sp(**kw, **sparse, generator=torch.manual_seed(3)).frames.clone()
    eager = sp(**kw, **sparse, generator=torch.manual_seed(3), use_graph=False).frames.clone()
    off = sp(**kw, **sparse, controlnet_conditioning_scale=0.0, generator=torch.manual_seed(3)).frames
    assert torch.isfinite(on).all() and torch.equal(bits(on), bits(eager))
    assert torch.isfinite(off).all() and not torch.equal(on, off)


def test_frame_sharded_pipeline_is_refused(tiny, pipe):
    pipe.dist = object()  # any frame shard: refused before it is used
    try:
        with pytest.raises(NotImplementedError, match="not sharded"):
            pipe(**call_kw(tiny))
    finally:
        pipe.dist = None
