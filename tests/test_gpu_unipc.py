"""The UniPC step on the MI355X: the kernel (vd_ddim_cfg_step with VD_STEP_UNIPC) bit for bit against
tests/unipc_ref.py run in torch fp32 on the CPU, inside poison-and-canary frames, with NaN in every
state slab a row must not read; whole schedules through the kernel with the three-slab state handed
from step to step in place; DenoiseLoop with a UniPCMultistepScheduler eagerly, on the captured
graph, after reset and reschedule; the pipelines; and the 4-step pipeline's final latents against
the fp32 CPU restatement (oracle/unet_ref.py blocks + unipc_ref).

Bars (none taken from the device): equality everywhere but the last check, whose bar is that of
tests/test_gpu_dpm.py's fp32-restatement test: 1.3 x the rel-L2 of the bf16-emulating CPU
restatement against the fp32 one; both figures are printed.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import memframe as mf
import unipc_ref as R
import vdiff._lib as L
from vdiff import (AnimateDiffControlNetPipeline, AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline, DDIMScheduler,
                   DenoiseLoop, DPMSolverMultistepScheduler, EulerDiscreteScheduler, UNetMotionModel,
                   UniPCMultistepScheduler, init_synthetic_, ops)

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
F32, BF = torch.float32, torch.bfloat16
N_STEPS = 6
G = 2.0
NAN = float("nan")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def sched(n=None, **kw):
    """The SD-1.5 config the pipelines here run, with Karras sigmas."""
    kw.setdefault("use_karras_sigmas", True)
    s = UniPCMultistepScheduler.from_config(DDIMScheduler().config, **kw)
    if n is not None:
        s.set_timesteps(n)
    return s


def ref_for(s, n, **kw):
    c = s.config
    return R.UniPCRef(coef="rows", solver_order=c.solver_order, solver_type=c.solver_type,
                      disable_corrector=c.disable_corrector, use_karras_sigmas=c.use_karras_sigmas,
                      final_sigmas_type=c.final_sigmas_type, timestep_spacing=c.timestep_spacing,
                      steps_offset=c.steps_offset, beta_schedule=c.beta_schedule, beta_start=c.beta_start,
                      beta_end=c.beta_end, **kw).set_timesteps(n)


# ---------------------------------------------------------------- the kernel
@pytest.fixture(scope="module")
def tables():
    """5-step tables of the restatement's rows (the scheduler's own agree, tests/test_unipc_host.py):
    the default (flags 0, 1|4, 1|2|4, 1|2|4, 1|2 with s_next = 0), one with step 0's corrector
    disabled (row 1: flags 4) and a first-order one (flags 1)."""
    out = {}
    for name, kw, flags in [("default", {}, [0, 5, 7, 7, 3]), ("nocorr", dict(disable_corrector=[0]), [0, 4, 7, 7, 3]),
                            ("order1", dict(solver_order=1), [0, 1, 1, 1, 1])]:
        s = sched(5, **kw)
        tab = ref_for(s, 5).table()
        assert tab[:, 12].tolist() == [float(f) for f in flags]
        assert torch.equal(s.coefficient_table()[:, 12], tab[:, 12])
        assert torch.isfinite(tab).all() and tab[-1, 8] == 0 and tab[-1, 9] == -1
        out[name] = tab
    return out


# (B, C, F, H, W), eps column slack (ld_eps = C + 2 * slack): 512 elements (two full blocks) with
# ld_eps = C and with slack; 840 elements (four blocks, the last ragged) with slack
SHAPES = [((1, 4, 2, 8, 8), 0), ((1, 4, 2, 8, 8), 8), ((2, 4, 3, 5, 7), 8)]
SHAPE_IDS = ["1x4x2x8x8", "1x4x2x8x8_slack8", "2x4x3x5x7_slack8"]
# (table, step): every kind of row, and a step index past the end (clamped to the last row)
ROWS = [("default", 0), ("default", 1), ("default", 2), ("default", 4), ("default", 9), ("nocorr", 1), ("order1", 2)]
ROW_IDS = ["first_0", "second_1+4", "middle_1+2+4", "last_1+2", "past_end", "no_corrector_4", "order_one_1"]
SCALES = [3.0, 2.5, 0.0, 1.25, 0.5]
# (ncfg, PAG, table, step): plain ncfg 1 and 2 on every row; perturbed-attention guidance, which
# changes the guided eps alone, with low byte 2 on the middle row and 3 on the last
CASES = [(ncfg, False, name, step) for ncfg in (1, 2) for name, step in ROWS] + \
        [(2, True, "default", 2), (3, True, "default", 4)]
CASE_IDS = [f"ncfg{ncfg}-{rid}" for ncfg in (1, 2) for rid in ROW_IDS] + ["pag2-middle_1+2+4", "pag3-last_1+2"]


def guided(eps, ncfg, pag, B, C, Fr, H, W, scale):
    """The guided eps in latent layout, one fp32 torch op at a time (include/vdiff.h)."""
    e = eps.reshape(ncfg, B, Fr, H, W, C).permute(0, 1, 5, 2, 3, 4)
    g, s = torch.tensor(G), torch.tensor(scale)
    if not pag:
        return e[0] if ncfg == 1 else e[0] + g * (e[1] - e[0])
    if ncfg == 2:
        return e[0] + s * (e[0] - e[1])
    return (e[0] + g * (e[1] - e[0])) + s * (e[1] - e[2])


@pytest.mark.parametrize("ncfg, pag, name, step", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("shape, slack", SHAPES, ids=SHAPE_IDS)
def test_kernel_matches_reference_bit_for_bit(cuda, tables, shape, slack, ncfg, pag, name, step):
    B, C, Fr, H, W = shape
    cpad, n = 8, 5
    rows = B * Fr * H * W
    table = tables[name]
    st = min(step, n - 1)
    flags = int(table[st, 12])
    g = torch.Generator().manual_seed(1000 * pag + 100 * ncfg + 10 * B + step)
    eps = torch.randn(ncfg * rows, C, generator=g)
    lat = torch.randn(shape, generator=g)
    state = torch.randn((3,) + shape, generator=g)
    # what the row must not read is NaN: everything at flags 0, S1 unless the corrector is second
    # order, S2 without a corrector
    if not flags:
        state[0] = NAN
    if not flags & 2:
        state[1] = NAN
    if not flags & 1:
        state[2] = NAN

    ev, fe = mf.load2d(eps.to(cuda), col_slack=slack, name="eps")   # the slack columns are NaN
    assert ev.stride(0) == C + 2 * slack
    xv, fx = mf.loadnd(lat.to(cuda), name="latents")
    coef = ops.pag_coef(SCALES, table) if pag else table.clone()
    cv, fc = mf.loadnd(coef.to(cuda), name="coef")                  # rows alone: what follows is the frame's poison
    before = bits(cv)
    sv, fs = mf.loadnd(state.to(cuda), name="x0_out")
    nv, fn = mf.framed((ncfg * rows, cpad), BF, cuda, name="next_in")  # pre-filled with 0xFF
    sidx = torch.tensor([step], device=cuda, dtype=torch.int32)

    ops.unipc_cfg_step(ev, ncfg, G, xv, cv, step_idx=sidx, x0_out=sv, next_in=nv, pag_n=n if pag else 0)
    torch.cuda.synchronize()

    e = guided(eps, ncfg, pag, B, C, Fr, H, W, SCALES[st])
    want, s0, s1, s2 = R.kernel_step(e, lat, state[0], state[1], state[2], table[st])
    for t in (want, s0, s1, s2):
        assert torch.isfinite(t).all()
    if not flags:
        assert torch.equal(s1, s0) and torch.equal(s2, lat)
    if step == 4:
        assert torch.equal(want, s0)                                # s_next = 0: x_next = m_t
    assert torch.isfinite(xv).all() and torch.isfinite(sv).all()
    assert torch.equal(bits(xv), bits(want))
    assert torch.equal(bits(sv[0]), bits(s0))
    assert torch.equal(bits(sv[1]), bits(s1))
    assert torch.equal(bits(sv[2]), bits(s2))
    packed = want.permute(0, 2, 3, 4, 1).reshape(rows, C).to(BF)
    for h in range(ncfg):
        half = nv[h * rows:(h + 1) * rows].cpu()
        assert torch.equal(bits(half[:, :C]), bits(packed))
        assert (half[:, C:].view(torch.int16) == 0).all()
    mf.assert_all_intact(fe, fx, fc, fs, fn)
    fs.assert_written(torch.stack([s0, s1, s2]))
    assert torch.equal(bits(cv), before)  # the rows are read-only
    assert int(sidx.item()) == step


def test_entry_point_refusals_with_device_operands(cuda):
    """tests/test_unipc_host.py's cases with operands the entry point would otherwise take: the
    valid calls return 0, each refused one differs from one of them in the argument named."""
    B, C, Fr, H, W = 1, 4, 2, 8, 8
    N = B * C * Fr * H * W
    eps = torch.zeros(3 * Fr * H * W, C, device=cuda)
    # one allocation: the latents in the middle, room for a state on either side
    pool = torch.zeros(8 * N, device=cuda)
    lat = pool[3 * N:4 * N].view(B, C, Fr, H, W)
    lat.fill_(1.0)
    state = pool[4 * N:7 * N]                                       # right behind the latents: no overlap
    tab = sched(5).coefficient_table()
    coef = tab.to(cuda)
    pcoef = ops.pag_coef(SCALES, tab).to(cuda)
    stream = torch.cuda.current_stream().cuda_stream
    U, PAG = L.VD_STEP_UNIPC, L.VD_STEP_PAG

    def call(fn, ncfg, x0=state.data_ptr(), coef_p=None):
        if coef_p is None:
            coef_p = (pcoef if ncfg & PAG else coef).data_ptr()
        return fn(eps.data_ptr(), C, ncfg, 1.0, lat.data_ptr(), B, C, Fr, H, W, coef_p, 5, None, x0, None, 0, stream)
    h = L.lib()
    f = h.vd_ddim_cfg_step
    for bad in (2 | U | L.VD_STEP_LCM, 2 | U | L.VD_STEP_DPM, 2 | U | 0x200, 2 | U | 0x1000, U, 3 | U, 1 | U | PAG,
                4 | U | PAG):
        assert call(f, bad) == L.VD_EINVAL, hex(bad)
    assert call(f, 1 | 0x200) == L.VD_EINVAL and call(f, 1 | 0x1000) == L.VD_EINVAL
    for word in (1 | U, 2 | U, 2 | U | PAG, 3 | U | PAG):
        assert call(f, word, x0=None) == L.VD_EINVAL
        assert call(f, word, coef_p=coef.data_ptr() + 4) == L.VD_EINVAL
        for off in (0, -3 * N + 1, N - 1, -N):                      # floats from the latents' base
            assert call(f, word, x0=lat.data_ptr() + 4 * off) == L.VD_EINVAL, (hex(word), off)
        assert call(h.vd_euler_cfg_step, word) == L.VD_EINVAL
    torch.cuda.synchronize()
    assert (lat == 1).all() and (pool[:3 * N] == 0).all() and (pool[4 * N:] == 0).all()
    # the valid words, the state right behind and right in front of the latents
    assert call(f, 2 | U) == 0
    torch.cuda.synchronize()
    # eps = 0 on row 0: m_t = x / alpha_s in S0 and S1, the sample itself in S2, and the latents moved
    m = torch.ones(N) / tab[0, 0]
    assert torch.equal(state.cpu(), torch.cat([m, m, torch.ones(N)]))
    assert torch.equal(lat.cpu().flatten(), tab[0, 8] * torch.ones(N) - tab[0, 9] * m)
    assert (pool[:3 * N] == 0).all() and (pool[7 * N:] == 0).all()
    for word in (1 | U, 2 | U | PAG, 3 | U | PAG):
        assert call(f, word, x0=pool.data_ptr()) == 0, hex(word)    # [0, 3N): ends where the latents begin
    torch.cuda.synchronize()
    assert torch.isfinite(pool).all() and (pool[7 * N:] == 0).all()
    with pytest.raises(ValueError, match="three times the latents' size"):
        ops.unipc_cfg_step(eps, 1, 1.0, lat, coef, x0_out=pool[:N])
    with pytest.raises(ValueError, match="three times the latents' size"):
        ops.unipc_cfg_step(eps, 1, 1.0, lat, coef)
    with pytest.raises(ValueError, match=r"coef is \[n, 16\] rows"):
        ops.unipc_cfg_step(eps, 1, 1.0, lat, coef[:, :8].contiguous(), x0_out=pool[:3 * N])
    with pytest.raises(ValueError, match="PAG scales coef holds"):
        ops.unipc_cfg_step(eps, 2, 1.0, lat, pcoef[:-16].contiguous(), x0_out=pool[:3 * N], pag_n=5)


@pytest.mark.parametrize("n, kw", [(5, {}), (16, dict(final_sigmas_type="sigma_min", use_karras_sigmas=False)),
                                   (6, dict(solver_type="bh1")), (6, dict(disable_corrector=[1]))],
                         ids=["n5_zero", "n16_sigma_min", "bh1", "disable_corrector_1"])
def test_whole_schedule_hands_the_state_over(cuda, n, kw):
    """Fresh random eps on every step, a 64-element latent, the device step counter, the state
    starting as NaN and handed over in place: the kernel's run and UniPCMultistepScheduler.step's
    both equal the stateful reference under ==, the state slabs too."""
    shape = (1, 4, 1, 4, 4)
    s = sched(n, **kw)
    ref = ref_for(s, n)
    tab = ref.table()
    assert torch.equal(tab[:, 12], s.coefficient_table()[:, 12])
    if "disable_corrector" in kw:
        assert tab[:, 12].tolist() == [0.0, 5.0, 4.0, 7.0, 7.0, 3.0]
    g = torch.Generator().manual_seed(n)
    lat0 = torch.randn(shape, generator=g)
    eps = torch.randn(n, 16, 4, generator=g)
    coef = tab.to(cuda)
    lat = lat0.to(cuda)
    state = torch.full((3,) + shape, NAN, device=cuda)
    sidx = torch.zeros(1, device=cuda, dtype=torch.int32)
    s2 = sched(n, **kw)
    x_api = lat0.to(cuda)
    x_ref = lat0
    for i in range(n):
        ops.unipc_cfg_step(eps[i].to(cuda), 1, 1.0, lat, coef, step_idx=sidx, x0_out=state)
        ops.step_advance(sidx)
        e = eps[i].reshape(1, 1, 4, 4, 4).permute(0, 4, 1, 2, 3)
        x_ref = ref.step(e, x_ref)
        assert torch.isfinite(x_ref).all()
        assert torch.equal(bits(lat), bits(x_ref)), i
        assert torch.equal(bits(state[0]), bits(ref.model_outputs[-1])), i
        assert torch.equal(bits(state[2]), bits(ref.last_sample)), i
        if i:
            assert torch.equal(bits(state[1]), bits(ref.model_outputs[-2])), i
        x_api = s2.step(e.to(cuda), s.timesteps[i], x_api).prev_sample
        assert torch.equal(bits(x_api), bits(x_ref)), i
        assert s2.this_order == ref.this_order
    assert int(sidx.item()) == n and s2.step_index == n and s2.lower_order_nums == 2


# ---------------------------------------------------------------- loop and scheduler
@pytest.fixture(scope="module")
def tiny(cuda):
    """The tiny UNet and the golden inputs cut to 2 frames x 32^2."""
    unet = init_synthetic_(UNetMotionModel("tiny"), seed=0).to("cuda", BF).prepare()
    g = np.load(GOLD / "tiny_unet.npz")
    lat = torch.from_numpy(g["latents"])[:, :, :2, :32, :32].contiguous().cuda()
    ehs = torch.from_numpy(g["ehs"]).cuda()
    return dict(unet=unet, lat=lat, ehs=ehs)


@pytest.fixture(scope="module")
def eager(tiny):
    """The eager 6-step loop, computed once."""
    loop = DenoiseLoop(tiny["unet"], sched(N_STEPS), tiny["lat"], tiny["ehs"], G, use_graph=False).prime()
    assert loop.graph is None and loop.unipc_state.shape == (3,) + tuple(loop.lat.shape)
    assert loop.coef.shape == (N_STEPS, 16) and loop.coef[:, 12].tolist() == [0.0, 5.0, 7.0, 7.0, 7.0, 3.0]
    out = loop.run().clone()
    assert torch.isfinite(out).all()
    return out


def test_eager_loop_equals_unet_plus_scheduler_step(tiny, eager):
    s = sched(N_STEPS)
    x = tiny["lat"]
    for t in s.timesteps:
        eps = tiny["unet"](torch.cat([x, x]), t, encoder_hidden_states=tiny["ehs"]).sample
        u, c = eps.chunk(2)
        x = s.step(u + G * (c - u), t, x).prev_sample
    assert s.step_index == N_STEPS
    assert torch.equal(bits(x), bits(eager))


def test_graph_replays_carry_the_state(tiny, eager):
    s = sched(N_STEPS)
    loop = DenoiseLoop(tiny["unet"], s, tiny["lat"], tiny["ehs"], G, use_graph=True).prime()
    assert loop.graph is not None, loop.graph_error
    assert torch.equal(bits(loop.run()), bits(eager))
    assert int(loop.step_idx.item()) == N_STEPS
    # the same capture after reset: the stale state of the finished run is never read — nor NaN
    loop.reset(tiny["lat"])
    assert torch.equal(bits(loop.run()), bits(eager))
    loop.reset(tiny["lat"])
    loop.unipc_state.fill_(NAN)
    assert torch.equal(bits(loop.run()), bits(eager))
    with pytest.raises(RuntimeError, match="scheduled steps"):
        loop.run(1)
    # a 4-step schedule on the same capture equals a fresh 4-step loop
    s.set_timesteps(4)
    loop.reschedule(s.timesteps)
    loop.reset(tiny["lat"])
    got = loop.run().clone()
    assert int(loop.step_idx.item()) == 4
    fresh = DenoiseLoop(tiny["unet"], sched(4), tiny["lat"], tiny["ehs"], G, use_graph=False).prime().run()
    assert torch.equal(bits(got), bits(fresh))
    assert not torch.equal(got, eager)


def test_other_kinds_hold_no_three_slab_state(tiny):
    u, lat, ehs = tiny["unet"], tiny["lat"], tiny["ehs"]
    with pytest.raises(ValueError, match="step_noise is for"):
        DenoiseLoop(u, sched(N_STEPS), lat, ehs, G, step_noise=torch.zeros((N_STEPS,) + tuple(lat.shape)))
    d = DDIMScheduler(beta_schedule="linear")
    e = EulerDiscreteScheduler.from_config(None, timestep_spacing="linspace", beta_schedule="linear")
    m = DPMSolverMultistepScheduler.from_config(DDIMScheduler().config)
    for s in (d, e, m):
        s.set_timesteps(4)
        loop = DenoiseLoop(u, s, lat, ehs, G, use_graph=False)
        assert not hasattr(loop, "unipc_state")
        assert all(v.numel() == lat.numel() for v in loop.step_kwargs.values())


# ---------------------------------------------------------------- pipelines
def call_kw(tiny):
    neg, pos = tiny["ehs"].chunk(2)
    return dict(prompt_embeds=pos, negative_prompt_embeds=neg, num_frames=2, height=256, width=256,
                num_inference_steps=N_STEPS, guidance_scale=G, output_type="latent")


def test_pipeline_equals_the_loop_and_refuses_free_init(tiny, eager):
    pipe = AnimateDiffPipeline(tiny["unet"], sched())
    got = pipe(**call_kw(tiny), latents=tiny["lat"]).frames
    assert torch.equal(bits(got), bits(eager))
    pipe.enable_free_init(num_iters=2)
    with pytest.raises(NotImplementedError, match="FreeInit with UniPCMultistepScheduler"):
        pipe(**call_kw(tiny))
    pipe.disable_free_init()


def test_video_to_video_runs_a_slice_that_starts_fresh(tiny):
    """strength 0.5 of 6 steps runs the last three timesteps: row 0 of the slice has flags 0, row 1
    a first-order corrector."""
    v2v = AnimateDiffVideoToVideoPipeline.from_config("tiny", scheduler=sched())
    kw = call_kw(tiny)
    kw.pop("num_frames")
    got = v2v(**kw, latents=tiny["lat"], strength=0.5, generator=torch.manual_seed(0)).frames
    s = sched(N_STEPS)
    ts = s.timesteps[3:]
    rows = s.coefficient_table(ts)
    assert rows[:, 12].tolist() == [0.0, 5.0, 3.0] and s.coefficient_table()[3:, 12].tolist() == [7.0, 7.0, 3.0]
    want = DenoiseLoop(v2v.unet, s, tiny["lat"], tiny["ehs"], G, timesteps=ts, use_graph=False).prime().run()
    assert torch.equal(bits(got), bits(want))


def test_controlnet_pipeline_with_a_disabled_control_is_the_plain_pipeline(cuda, tiny):
    p = AnimateDiffControlNetPipeline.from_config("tiny", device=cuda, vae=None, scheduler=sched())
    plain = AnimateDiffPipeline(p.unet, sched())
    neg, pos = tiny["ehs"].chunk(2)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=tiny["lat"][:, :, :, :8, :8].contiguous(),
              num_frames=2, height=64, width=64, num_inference_steps=4, guidance_scale=G, output_type="latent")
    frames = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    want = plain(**kw).frames.clone()
    off = p(**kw, conditioning_frames=frames, controlnet_conditioning_scale=0.0).frames
    assert torch.equal(off, want)
    on = p(**kw, conditioning_frames=frames).frames
    assert torch.isfinite(on).all() and not torch.equal(on, want)


def test_pag_pipeline_runs_on_the_graph(cuda):
    """The fourth pipeline: the PAG scales sit in front of the 16-float rows, three branches."""
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
    p = AnimateDiffPAGPipeline(dunet, sched())
    on = p(**kw, **pag).frames.clone()
    eager = p(**kw, **pag, use_graph=False).frames.clone()
    off = p(**kw, pag_scale=0.0).frames.clone()
    plain = AnimateDiffPipeline(dunet, sched())(**kw).frames
    assert torch.isfinite(on).all()
    assert torch.equal(bits(on), bits(eager))
    assert torch.equal(bits(off), bits(plain)) and not torch.equal(on, off)


def test_sparsectrl_pipeline_with_a_zero_scale_is_the_plain_pipeline(cuda):
    """The fifth pipeline, on from_config's synthetic models: 4 frames of 8 x 8 latents, key frames 0 and 3."""
    from vdiff import AnimateDiffSparseControlNetPipeline
    p = AnimateDiffSparseControlNetPipeline.from_config("tiny", device=cuda, scheduler=sched())
    g = torch.Generator().manual_seed(11)
    lat = torch.randn(1, 4, 4, 8, 8, generator=g)
    ehs = torch.randn(2, 77, p.unet.config["cross_attention_dim"], generator=g)
    kw = dict(prompt_embeds=ehs[1:2], negative_prompt_embeds=ehs[0:1], latents=lat, num_frames=4, height=64, width=64,
              num_inference_steps=4, guidance_scale=G, output_type="latent")
    sparse = dict(conditioning_frames=torch.rand(2, 3, 16, 16, generator=g), controlnet_frame_indices=[0, 3])
    plain = AnimateDiffPipeline(p.unet, sched())(**kw).frames.clone()
    off = p(**kw, **sparse, controlnet_conditioning_scale=0.0, generator=torch.manual_seed(3)).frames.clone()
    on = p(**kw, **sparse, generator=torch.manual_seed(3)).frames.clone()
    eager = p(**kw, **sparse, generator=torch.manual_seed(3), use_graph=False).frames
    assert torch.equal(off, plain)
    assert torch.isfinite(on).all() and not torch.equal(on, plain)
    assert torch.equal(bits(on), bits(eager))


# ---------------------------------------------------------------- against the fp32 restatement
def test_pipeline_matches_the_fp32_restatement(cuda):
    """The 4-step pipeline (Karras, CFG 7.5) on tests/controlnet_ref.py's tiny case — 2 frames of
    8 x 8 latents — against oracle/unet_ref.py's blocks + unipc_ref in fp32 on the CPU.  Bar, as
    tests/test_gpu_dpm.py's: 1.3 x the bf16-emulating restatement's own rel-L2; the emulated figure
    is computed here on the CPU, never from a device value."""
    import controlnet_ref as C
    c = C.tiny_case()
    g = 7.5
    s = sched(4)

    def restatement(act):
        ref = ref_for(s, 4)
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
               height=64, width=64, num_inference_steps=4, guidance_scale=g, output_type="latent").frames
    e_emu, e_dev = C.rel_l2(emu, want), C.rel_l2(got, want)
    print(f"PIPELINE unipc bh2 karras, 4 steps: emulated {e_emu:.5f} device {e_dev:.5f} bar {1.3 * e_emu:.5f}")
    assert torch.isfinite(got).all()
    assert 0 < e_emu < 0.1
    assert e_dev <= 1.3 * e_emu
