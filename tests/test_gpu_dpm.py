"""The DPM-Solver++ step on the MI355X: the kernel (vd_ddim_cfg_step with VD_STEP_DPM) bit for bit
against tests/dpm_ref.py run in torch fp32 on the CPU, inside poison-and-canary frames; whole
schedules through the kernel with the history handed from step to step; DenoiseLoop with a
DPMSolverMultistepScheduler eagerly, on the captured graph, after reset and reschedule; the three
pipelines against hand-driven runs that draw in diffusers' order; and the 4-step pipeline's final
latents against the fp32 CPU restatement (oracle/unet_ref.py blocks + dpm_ref).

Bars (none taken from the device): equality everywhere but the last check, whose bar is 1.3 x the
rel-L2 of the bf16-emulating CPU restatement against the fp32 one (tests/test_gpu_controlnet.py's
convention); both figures are printed and stand in DESIGN.md's table.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import dpm_ref as R
import memframe as mf
import vdiff._lib as L
from vdiff import (AnimateDiffControlNetPipeline, AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline, DDIMScheduler,
                   DenoiseLoop, DPMSolverMultistepScheduler, EulerDiscreteScheduler, LCMScheduler, UNetMotionModel,
                   init_synthetic_, ops)
from vdiff.pipeline import randn_tensor

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
F32, BF = torch.float32, torch.bfloat16
N_STEPS = 4
G = 2.0
TYPES = ["dpmsolver++", "sde-dpmsolver++"]
IDS = ["det", "sde"]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def sched(alg="dpmsolver++", n=None, **kw):
    """The SD-1.5 config the pipelines here run; the deterministic type with Karras sigmas."""
    kw.setdefault("use_karras_sigmas", alg == "dpmsolver++")
    s = DPMSolverMultistepScheduler.from_config(DDIMScheduler().config, algorithm_type=alg, **kw)
    if n is not None:
        s.set_timesteps(n)
    return s


def ref_for(s, n, **kw):
    c = s.config
    return R.DPMRef(coef="rows", solver_order=c.solver_order, algorithm_type=c.algorithm_type,
                    lower_order_final=c.lower_order_final, euler_at_final=c.euler_at_final,
                    use_karras_sigmas=c.use_karras_sigmas, final_sigmas_type=c.final_sigmas_type,
                    timestep_spacing=c.timestep_spacing, steps_offset=c.steps_offset, beta_schedule=c.beta_schedule,
                    beta_start=c.beta_start, beta_end=c.beta_end, **kw).set_timesteps(n)


# ---------------------------------------------------------------- the kernel
@pytest.fixture(scope="module")
def tables():
    """5-step tables of both types: row 0 and row 4 ("zero" final) first order, rows 1..3 second."""
    out = {}
    for alg in TYPES:
        s = sched(alg, 5)
        tab = s.coefficient_table()
        assert torch.equal(tab, ref_for(s, 5).table())
        assert [int(f) & 1 for f in tab[:, 7]] == [0, 1, 1, 1, 0]
        out[alg] = tab
    return out


# (B, C, F, H, W), eps column slack (ld_eps = C + 2 * slack): the second shape has an odd element
# count (grid-stride tail, more than one block) and ld_eps = cpad = 8
SHAPES = [((1, 4, 2, 8, 8), 0), ((2, 4, 3, 5, 7), 2)]


@pytest.mark.parametrize("step", [0, 2, 4, 9], ids=["first", "middle", "last", "past_end"])
@pytest.mark.parametrize("alg", TYPES, ids=IDS)
@pytest.mark.parametrize("shape, slack", SHAPES, ids=["1x4x2x8x8", "2x4x3x5x7_ld8"])
@pytest.mark.parametrize("ncfg", [1, 2])
def test_kernel_matches_reference_bit_for_bit(cuda, tables, ncfg, shape, slack, alg, step):
    B, C, Fr, H, W = shape
    cpad, n = 8, 5
    rows, numel = B * Fr * H * W, B * C * Fr * H * W
    table = tables[alg]
    st = min(step, n - 1)
    second, sde = bool(int(table[st, 7]) & 1), alg.startswith("sde")
    assert second == (step == 2)
    g = torch.Generator().manual_seed(1000 * sde + 100 * ncfg + 10 * B + step)
    eps = torch.randn(ncfg * rows, C, generator=g)
    lat = torch.randn(shape, generator=g)
    m1 = torch.randn(shape, generator=g)
    noise = torch.randn(shape, generator=g)

    ev, fe = mf.load2d(eps.to(cuda), col_slack=slack, name="eps")   # the slack columns are NaN
    assert ev.stride(0) == C + 2 * slack
    xv, fx = mf.loadnd(lat.to(cuda), name="latents")
    if sde:  # rows, then n slabs: every slab NaN but the step's own
        buf = torch.full((ops.dpm_buffer_numel(n, numel, True),), float("nan"))
        buf[:8 * n] = table.reshape(-1)
        buf[8 * n + st * numel:8 * n + (st + 1) * numel] = noise.reshape(-1)
    else:    # rows alone: whatever follows them is the frame's poison
        buf = table.clone()
    cv, fc = mf.loadnd(buf.to(cuda), name="coef")
    before = bits(cv)
    # the history: m1 where the row is second order, else 0xFF (a NaN that must not be read)
    x0v, f0 = mf.framed_nd(shape, F32, cuda, name="x0_out")
    if second:
        f0.load(m1.to(cuda))
    nv, fn = mf.framed((ncfg * rows, cpad), BF, cuda, name="next_in")  # pre-filled with 0xFF
    sidx = torch.tensor([step], device=cuda, dtype=torch.int32)

    ops.dpm_cfg_step(ev, ncfg, G, xv, cv, step_idx=sidx, x0_out=x0v, next_in=nv)
    torch.cuda.synchronize()

    e = eps.reshape(ncfg, B, Fr, H, W, C).permute(0, 1, 5, 2, 3, 4)
    e = R.cfg_combine(e[0], e[1], G) if ncfg == 2 else e[0]
    want, x0 = R.kernel_step(e, lat, m1 if second else None, table[st], noise if sde else None)
    assert torch.isfinite(want).all() and torch.isfinite(x0).all()
    assert torch.isfinite(xv).all() and torch.isfinite(x0v).all()
    assert torch.equal(bits(xv), bits(want))
    assert torch.equal(bits(x0v), bits(x0))
    packed = want.permute(0, 2, 3, 4, 1).reshape(rows, C).to(BF)
    for h in range(ncfg):
        half = nv[h * rows:(h + 1) * rows].cpu()
        assert torch.equal(bits(half[:, :C]), bits(packed))
        assert (half[:, C:].view(torch.int16) == 0).all()
    mf.assert_all_intact(fe, fx, fc, f0, fn)
    f0.assert_written(x0)
    assert torch.equal(bits(cv), before)  # rows and slabs are read-only
    assert int(sidx.item()) == step


def test_entry_point_refusals_with_device_operands(cuda):
    """tests/test_dpm_host.py's cases with operands the entry point would otherwise take: the
    valid call returns 0, each refused one differs from it in the argument named."""
    B, C, Fr, H, W = 1, 4, 2, 8, 8
    eps = torch.zeros(2 * Fr * H * W, C, device=cuda)
    lat = torch.ones(B, C, Fr, H, W, device=cuda)
    hist = torch.zeros_like(lat)
    coef = sched("dpmsolver++", 5).coefficient_table().to(cuda)
    stream = torch.cuda.current_stream().cuda_stream

    def call(fn, ncfg, x0=hist.data_ptr(), coef_p=coef.data_ptr()):
        return fn(eps.data_ptr(), C, ncfg, 1.0, lat.data_ptr(), B, C, Fr, H, W, coef_p, 5, None, x0, None, 0, stream)
    h = L.lib()
    assert call(h.vd_ddim_cfg_step, 2 | L.VD_STEP_DPM | L.VD_STEP_LCM) == L.VD_EINVAL
    assert call(h.vd_ddim_cfg_step, 2 | L.VD_STEP_DPM | 0x200) == L.VD_EINVAL
    assert call(h.vd_ddim_cfg_step, 3 | L.VD_STEP_DPM) == L.VD_EINVAL
    assert call(h.vd_ddim_cfg_step, 2 | L.VD_STEP_DPM, x0=None) == L.VD_EINVAL
    assert call(h.vd_ddim_cfg_step, 2 | L.VD_STEP_DPM, x0=lat.data_ptr()) == L.VD_EINVAL
    assert call(h.vd_ddim_cfg_step, 2 | L.VD_STEP_DPM, coef_p=coef.data_ptr() + 4) == L.VD_EINVAL
    assert call(h.vd_euler_cfg_step, 2 | L.VD_STEP_DPM) == L.VD_EINVAL
    torch.cuda.synchronize()
    assert (lat == 1).all() and (hist == 0).all()
    assert call(h.vd_ddim_cfg_step, 2 | L.VD_STEP_DPM) == 0
    torch.cuda.synchronize()
    # eps = 0: x0 = x / alpha_s, and the first-order row moved the latents
    assert torch.equal(hist.cpu(), torch.ones(B, C, Fr, H, W) / coef[0, 0].cpu())
    assert not (lat == 1).any()


@pytest.mark.parametrize("alg", TYPES, ids=IDS)
@pytest.mark.parametrize("n, final", [(5, "zero"), (16, "sigma_min")])
def test_whole_schedule_hands_the_history_over(cuda, n, final, alg):
    """Fresh random eps on every step, a 64-element latent, the device step counter: the kernel's
    run and DPMSolverMultistepScheduler.step's both equal the stateful reference under ==.  The
    16-step "sigma_min" schedule ends on a second-order step."""
    shape = (1, 4, 1, 4, 4)
    s = sched(alg, n, final_sigmas_type=final)
    ref = ref_for(s, n)
    tab = s.coefficient_table()
    assert torch.equal(tab, ref.table())
    assert int(tab[-1, 7]) & 1 == (final == "sigma_min")
    sde = s.sde
    g = torch.Generator().manual_seed(n)
    lat0 = torch.randn(shape, generator=g)
    eps = torch.randn(n, 16, 4, generator=g)
    noise = torch.randn((n,) + shape, generator=g)
    if sde:
        coef = torch.cat([tab.reshape(-1), noise.reshape(-1)]).to(cuda)
    else:
        coef = tab.to(cuda)
    lat = lat0.to(cuda)
    hist = torch.full(shape, float("nan"), device=cuda)
    sidx = torch.zeros(1, device=cuda, dtype=torch.int32)
    s2 = sched(alg, n, final_sigmas_type=final)
    x_api = lat0.to(cuda)
    x_ref = lat0
    for i in range(n):
        ops.dpm_cfg_step(eps[i].to(cuda), 1, 1.0, lat, coef, step_idx=sidx, x0_out=hist)
        ops.step_advance(sidx)
        e = eps[i].reshape(1, 1, 4, 4, 4).permute(0, 4, 1, 2, 3)
        x_ref = ref.step(e, x_ref, noise[i] if sde else None)
        assert torch.equal(bits(lat), bits(x_ref)), i
        assert torch.equal(bits(hist), bits(ref.model_outputs[-1])), i
        x_api = s2.step(e.to(cuda), s.timesteps[i], x_api, variance_noise=noise[i].to(cuda) if sde else None).prev_sample
        assert torch.equal(bits(x_api), bits(x_ref)), i
    assert int(sidx.item()) == n and s2.step_index == n and s2.lower_order_nums == 2


# ---------------------------------------------------------------- loop and scheduler
@pytest.fixture(scope="module")
def tiny(cuda):
    """The tiny UNet and the golden inputs cut to 2 frames x 32^2; two fixed sets of step noise."""
    unet = init_synthetic_(UNetMotionModel("tiny"), seed=0).to("cuda", BF).prepare()
    g = np.load(GOLD / "tiny_unet.npz")
    lat = torch.from_numpy(g["latents"])[:, :, :2, :32, :32].contiguous().cuda()
    ehs = torch.from_numpy(g["ehs"]).cuda()
    gen = torch.Generator().manual_seed(3)
    noise = [torch.stack([randn_tensor(lat.shape, gen, device="cuda", dtype=F32) for _ in range(N_STEPS)])
             for _ in range(2)]
    return dict(unet=unet, lat=lat, ehs=ehs, noise=noise[0], other=noise[1])


def loop_kw(tiny, alg, key="noise", n=N_STEPS):
    return dict(step_noise=tiny[key][:n]) if alg.startswith("sde") else {}


@pytest.fixture(scope="module")
def eager(tiny):
    """The eager 4-step loops, computed once: both types; the SDE type with each noise set."""
    out = {}
    for alg, key in [("dpmsolver++", "noise"), ("sde-dpmsolver++", "noise"), ("sde-dpmsolver++", "other")]:
        loop = DenoiseLoop(tiny["unet"], sched(alg, N_STEPS), tiny["lat"], tiny["ehs"], G, use_graph=False,
                           **loop_kw(tiny, alg, key)).prime()
        assert loop.graph is None and loop.x0_hist.shape == loop.lat.shape
        out[alg, key] = loop.run().clone()
        assert torch.isfinite(out[alg, key]).all()
    assert len({tuple(bits(v).flatten().tolist()) for v in out.values()}) == 3
    return out


@pytest.mark.parametrize("alg", TYPES, ids=IDS)
def test_eager_loop_equals_unet_plus_scheduler_step(tiny, eager, alg):
    s = sched(alg, N_STEPS)
    gen = torch.Generator().manual_seed(3)  # the stream tiny["noise"] was drawn from
    x = tiny["lat"]
    for i, t in enumerate(s.timesteps):
        eps = tiny["unet"](torch.cat([x, x]), t, encoder_hidden_states=tiny["ehs"]).sample
        u, c = eps.chunk(2)
        state = gen.get_state()
        x = s.step(u + G * (c - u), t, x, generator=gen).prev_sample
        # the SDE type draws once on every step, the last included; the deterministic type never
        assert torch.equal(gen.get_state(), state) == (not s.sde)
    assert s.step_index == N_STEPS
    assert torch.equal(bits(x), bits(eager[alg, "noise"]))


@pytest.mark.parametrize("alg", TYPES, ids=IDS)
def test_graph_replays_carry_the_history(tiny, eager, alg):
    s = sched(alg, N_STEPS)
    loop = DenoiseLoop(tiny["unet"], s, tiny["lat"], tiny["ehs"], G, use_graph=True, **loop_kw(tiny, alg)).prime()
    assert loop.graph is not None, loop.graph_error
    assert torch.equal(bits(loop.run()), bits(eager[alg, "noise"]))
    assert int(loop.step_idx.item()) == N_STEPS
    # the same capture after reset: the stale history of the finished run is never read
    if s.sde:
        loop.reset(tiny["lat"], step_noise=tiny["other"])
        assert torch.equal(bits(loop.run()), bits(eager[alg, "other"]))
        loop.reset(tiny["lat"])  # None keeps the slabs
        assert torch.equal(bits(loop.run()), bits(eager[alg, "other"]))
    else:
        loop.reset(tiny["lat"])
        assert torch.equal(bits(loop.run()), bits(eager[alg, "noise"]))
    with pytest.raises(RuntimeError, match="scheduled steps"):
        loop.run(1)
    # a 3-step schedule on the same capture equals a fresh 3-step loop
    s.set_timesteps(3)
    loop.reschedule(s.timesteps)
    loop.reset(tiny["lat"], **loop_kw(tiny, alg, n=3))
    got = loop.run().clone()
    assert int(loop.step_idx.item()) == 3
    fresh = DenoiseLoop(tiny["unet"], sched(alg, 3), tiny["lat"], tiny["ehs"], G, use_graph=False,
                        **loop_kw(tiny, alg, n=3)).prime().run()
    assert torch.equal(bits(got), bits(fresh))
    assert not torch.equal(got, eager[alg, "noise"])


def test_loop_refusals_and_other_kinds_hold_no_history(tiny):
    u, lat, ehs = tiny["unet"], tiny["lat"], tiny["ehs"]
    with pytest.raises(ValueError, match="needs step_noise"):
        DenoiseLoop(u, sched("sde-dpmsolver++", N_STEPS), lat, ehs, G)
    with pytest.raises(ValueError, match="step_noise of shape"):   # every step draws: n - 1 slabs are too few
        DenoiseLoop(u, sched("sde-dpmsolver++", N_STEPS), lat, ehs, G, step_noise=tiny["noise"][:N_STEPS - 1])
    with pytest.raises(ValueError, match="step_noise is for"):
        DenoiseLoop(u, sched("dpmsolver++", N_STEPS), lat, ehs, G, step_noise=tiny["noise"])
    d = DDIMScheduler(beta_schedule="linear")
    e = EulerDiscreteScheduler.from_config(None, timestep_spacing="linspace", beta_schedule="linear")
    lc = LCMScheduler.from_config(None, beta_schedule="linear")
    for s, kw in [(d, {}), (e, {}), (lc, dict(step_noise=tiny["noise"][:N_STEPS - 1]))]:
        s.set_timesteps(N_STEPS)
        loop = DenoiseLoop(u, s, lat, ehs, G, use_graph=False, **kw)
        assert not hasattr(loop, "x0_hist") and loop.step_kwargs == {}


# ---------------------------------------------------------------- pipelines
def call_kw(tiny):
    neg, pos = tiny["ehs"].chunk(2)
    return dict(prompt_embeds=pos, negative_prompt_embeds=neg, num_frames=2, height=256, width=256,
                num_inference_steps=N_STEPS, guidance_scale=G, output_type="latent")


@pytest.mark.parametrize("alg", TYPES, ids=IDS)
def test_pipeline_draws_in_diffusers_order(tiny, alg):
    pipe = AnimateDiffPipeline(tiny["unet"], sched(alg))
    pipe.torch_dtype = F32
    got = pipe(**call_kw(tiny), generator=torch.manual_seed(0)).frames
    # diffusers' loop by hand: the latents, then (SDE) one fp32 draw inside every scheduler.step
    gen = torch.manual_seed(0)
    x = randn_tensor((1, 4, 2, 32, 32), gen, device="cuda", dtype=F32)
    s = sched(alg, N_STEPS)
    for t in s.timesteps:
        u, c = tiny["unet"](torch.cat([x, x]), t, encoder_hidden_states=tiny["ehs"]).sample.chunk(2)
        x = s.step(u + G * (c - u), t, x, generator=gen).prev_sample
    assert torch.equal(bits(got), bits(x))
    if alg.startswith("sde"):   # the same run with the n fp32 slabs drawn up front, right after the latents
        gen = torch.manual_seed(0)
        x = randn_tensor((1, 4, 2, 32, 32), gen, device="cuda", dtype=F32)
        noise = torch.stack([randn_tensor(x.shape, gen, device="cuda", dtype=F32) for _ in range(N_STEPS)])
        want = DenoiseLoop(tiny["unet"], sched(alg, N_STEPS), x, tiny["ehs"], G, use_graph=False,
                           step_noise=noise).prime().run()
        assert torch.equal(bits(got), bits(want))


def test_pipeline_refusals(tiny):
    pipe = AnimateDiffPipeline(tiny["unet"], sched("sde-dpmsolver++"))
    pipe.dist = object()  # any frame shard: refused before it is used
    try:
        with pytest.raises(NotImplementedError, match="not sharded"):
            pipe(**call_kw(tiny))
    finally:
        pipe.dist = None
    pipe.enable_free_init(num_iters=2)
    with pytest.raises(NotImplementedError, match="FreeInit with DPMSolverMultistepScheduler"):
        pipe(**call_kw(tiny))
    pipe.disable_free_init()


@pytest.mark.parametrize("alg", TYPES, ids=IDS)
def test_video_to_video_runs_a_slice_with_a_first_order_start(tiny, alg):
    """strength 0.5 of 4 steps runs the last two timesteps: row 0 of the slice is first order."""
    v2v = AnimateDiffVideoToVideoPipeline.from_config("tiny", scheduler=sched(alg))
    kw = call_kw(tiny)
    kw.pop("num_frames")
    got = v2v(**kw, latents=tiny["lat"], strength=0.5, generator=torch.manual_seed(0)).frames
    s = sched(alg, N_STEPS)
    ts = s.timesteps[2:]
    rows = s.coefficient_table(ts)
    assert int(rows[0, 7]) & 1 == 0 and int(s.coefficient_table()[2, 7]) & 1 == 1
    gen = torch.manual_seed(0)
    extra = {}
    if s.sde:
        extra = dict(step_noise=torch.stack([randn_tensor(tiny["lat"].shape, gen, device="cuda", dtype=F32)
                                             for _ in range(2)]))
    want = DenoiseLoop(v2v.unet, s, tiny["lat"], tiny["ehs"], G, timesteps=ts, use_graph=False, **extra).prime().run()
    assert torch.equal(bits(got), bits(want))


def test_controlnet_pipeline_with_a_disabled_control_is_the_plain_pipeline(cuda, tiny):
    p = AnimateDiffControlNetPipeline.from_config("tiny", device=cuda, vae=None, scheduler=sched())
    plain = AnimateDiffPipeline(p.unet, sched())
    neg, pos = tiny["ehs"].chunk(2)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=tiny["lat"][:, :, :, :8, :8].contiguous(),
              num_frames=2, height=64, width=64, num_inference_steps=N_STEPS, guidance_scale=G, output_type="latent")
    frames = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    want = plain(**kw).frames.clone()
    off = p(**kw, conditioning_frames=frames, controlnet_conditioning_scale=0.0).frames
    assert torch.equal(off, want)
    on = p(**kw, conditioning_frames=frames).frames
    assert torch.isfinite(on).all() and not torch.equal(on, want)


# ---------------------------------------------------------------- against the fp32 restatement
def test_pipeline_matches_the_fp32_restatement(cuda):
    """The 4-step deterministic pipeline (Karras, CFG 7.5) on tests/controlnet_ref.py's tiny case —
    2 frames of 8 x 8 latents — against oracle/unet_ref.py's blocks + dpm_ref in fp32 on the CPU.
    Bar: 1.3 x the bf16-emulating restatement's own rel-L2; the emulated figure is computed here
    on the CPU, never from a device value."""
    import controlnet_ref as C
    c = C.tiny_case()
    g = 7.5
    s = sched("dpmsolver++", N_STEPS)

    def restatement(act):
        ref = ref_for(s, N_STEPS)
        x = c["lat"].float()
        for t in ref.timesteps.tolist():
            eps = C.unet_forward_residuals(c["usd"], c["cfg"], torch.cat([x, x]), int(t), c["ehs"], None, act)
            u, cnd = eps.chunk(2)
            x = ref.step(R.cfg_combine(u, cnd, g), x)
        return x
    with torch.no_grad():
        want, emu = restatement("fp32"), restatement("bf16")
    dunet = UNetMotionModel("tiny")
    dunet.load_state_dict(c["unet"].state_dict())
    pipe = AnimateDiffPipeline(dunet.to(cuda, BF).prepare(), sched())
    got = pipe(prompt_embeds=c["ehs"][1:2], negative_prompt_embeds=c["ehs"][0:1], latents=c["lat"], num_frames=2,
               height=64, width=64, num_inference_steps=N_STEPS, guidance_scale=g, output_type="latent").frames
    e_emu, e_dev = C.rel_l2(emu, want), C.rel_l2(got, want)
    print(f"PIPELINE dpm++ 2M karras, 4 steps: emulated {e_emu:.5f} device {e_dev:.5f} bar {1.3 * e_emu:.5f}")
    assert torch.isfinite(got).all()
    assert 0 < e_emu < 0.1
    assert e_dev <= 1.3 * e_emu
