"""The LCM step on the MI355X: the kernel (vd_ddim_cfg_step with VD_STEP_LCM) bit for bit against
tests/lcm_ref.py run in torch fp32 on the CPU, inside poison-and-canary frames; DenoiseLoop with
an LCMScheduler eagerly, stepwise and on the captured graph; LCMScheduler.step's draws; both the
plain and the FreeInit pipeline against hand-driven runs that draw in diffusers' order."""
from pathlib import Path

import numpy as np
import pytest
import torch

import lcm_ref as R
import memframe as mf
import vdiff._lib as L
from vdiff import (AnimateDiffPipeline, DenoiseLoop, LCMScheduler, UNetMotionModel, init_synthetic_, ops)
from vdiff.pipeline import randn_tensor

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
F32, BF = torch.float32, torch.bfloat16
N_STEPS = 4
G = 2.0


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


# ---------------------------------------------------------------- the kernel
@pytest.fixture(scope="module")
def table():
    ts = R.lcm_timesteps(N_STEPS)
    return R.table(ts, R.alphas_cumprod(schedule="linear"))


# (B, C, F, H, W), eps column slack (ld_eps = C + 2 * slack): the second shape has an odd element
# count (grid-stride tail) and ld_eps = cpad = 8
SHAPES = [((1, 4, 2, 8, 8), 0), ((2, 4, 3, 5, 7), 2)]


@pytest.mark.parametrize("step", [0, 2, 3, 7], ids=["first", "middle", "last", "past_end"])
@pytest.mark.parametrize("shape, slack", SHAPES, ids=["1x4x2x8x8", "2x4x3x5x7_ld8"])
@pytest.mark.parametrize("ncfg", [1, 2])
def test_kernel_matches_reference_bit_for_bit(cuda, table, ncfg, shape, slack, step):
    B, C, Fr, H, W = shape
    cpad = 8
    rows, numel = B * Fr * H * W, B * C * Fr * H * W
    st = min(step, N_STEPS - 1)
    last = st == N_STEPS - 1
    g = torch.Generator().manual_seed(100 * ncfg + 10 * B + step)
    eps = torch.randn(ncfg * rows, C, generator=g)
    lat = torch.randn(shape, generator=g)
    noise = torch.randn(shape, generator=g)

    ev, fe = mf.load2d(eps.to(cuda), col_slack=slack, name="eps")   # the slack columns are NaN
    assert ev.stride(0) == C + 2 * slack
    xv, fx = mf.loadnd(lat.to(cuda), name="latents")
    # rows, then N_STEPS slabs: every slab NaN but the step's own — and on the last step that one too
    buf = torch.full((ops.lcm_buffer_numel(N_STEPS, numel),), float("nan"))
    buf[:8 * N_STEPS] = table.reshape(-1)
    if not last:
        buf[8 * N_STEPS + st * numel:8 * N_STEPS + (st + 1) * numel] = noise.reshape(-1)
    cv, fc = mf.loadnd(buf.to(cuda), name="coef")
    before = bits(cv)
    x0v, f0 = mf.framed_nd(shape, F32, cuda, name="x0_out")
    nv, fn = mf.framed((ncfg * rows, cpad), BF, cuda, name="next_in")  # pre-filled with 0xFF
    sidx = torch.tensor([step], device=cuda, dtype=torch.int32)

    ops.lcm_cfg_step(ev, ncfg, G, xv, cv, step_idx=sidx, x0_out=x0v, next_in=nv)
    torch.cuda.synchronize()

    e = eps.reshape(ncfg, B, Fr, H, W, C).permute(0, 1, 5, 2, 3, 4)
    e = R.cfg_combine(e[0], e[1], G) if ncfg == 2 else e[0]
    want, den = R.lcm_step(e, lat, table[st], noise)
    if last:
        assert torch.equal(want, den)
    assert torch.isfinite(xv).all() and torch.isfinite(x0v).all()
    assert torch.equal(bits(xv), bits(want))
    assert torch.equal(bits(x0v), bits(den))
    packed = want.permute(0, 2, 3, 4, 1).reshape(rows, C).to(BF)
    for h in range(ncfg):
        half = nv[h * rows:(h + 1) * rows].cpu()
        assert torch.equal(bits(half[:, :C]), bits(packed))
        assert (half[:, C:].view(torch.int16) == 0).all()
    mf.assert_all_intact(fe, fx, fc, f0, fn)
    f0.assert_written(den)
    assert torch.equal(bits(cv), before)  # rows and slabs are read-only
    assert int(sidx.item()) == step


def test_entry_points_refuse_other_flag_bits(cuda):
    B, C, Fr, H, W = 1, 4, 2, 8, 8
    eps = torch.zeros(2 * Fr * H * W, C, device=cuda)
    lat = torch.zeros(B, C, Fr, H, W, device=cuda)
    coef = torch.zeros(ops.lcm_buffer_numel(1, lat.numel()), device=cuda)
    keep = lat.clone()

    def call(fn, ncfg):
        return fn(eps.data_ptr(), C, ncfg, 1.0, lat.data_ptr(), B, C, Fr, H, W, coef.data_ptr(), 1, None, None, None,
                  0, None)
    h = L.lib()
    assert call(h.vd_ddim_cfg_step, 1 | 0x200) == L.VD_EINVAL
    assert call(h.vd_ddim_cfg_step, 2 | L.VD_STEP_LCM | 0x200) == L.VD_EINVAL
    assert call(h.vd_euler_cfg_step, 1 | L.VD_STEP_LCM) == L.VD_EINVAL
    assert call(h.vd_euler_cfg_step, 2 | L.VD_STEP_LCM) == L.VD_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(lat, keep)


# ---------------------------------------------------------------- loop and scheduler
@pytest.fixture(scope="module")
def tiny(cuda):
    """The tiny UNet and the golden inputs cut to 2 frames x 32^2; two fixed sets of step noise."""
    unet = init_synthetic_(UNetMotionModel("tiny"), seed=0).to("cuda", BF).prepare()
    g = np.load(GOLD / "tiny_unet.npz")
    lat = torch.from_numpy(g["latents"])[:, :, :2, :32, :32].contiguous().cuda()
    ehs = torch.from_numpy(g["ehs"]).cuda()
    gen = torch.Generator().manual_seed(3)
    noise = [torch.stack([randn_tensor(lat.shape, gen, device="cuda", dtype=F32) for _ in range(N_STEPS - 1)])
             for _ in range(2)]
    return dict(unet=unet, lat=lat, ehs=ehs, noise=noise[0], other=noise[1])


def sched():
    s = LCMScheduler.from_config(None, beta_schedule="linear")
    s.set_timesteps(N_STEPS)
    return s


@pytest.fixture(scope="module")
def eager(tiny):
    """The eager 4-step loop with each noise set, computed once."""
    out = {}
    for k in ("noise", "other"):
        loop = DenoiseLoop(tiny["unet"], sched(), tiny["lat"], tiny["ehs"], G, use_graph=False, step_noise=tiny[k]).prime()
        assert loop.graph is None
        out[k] = loop.run().clone()
    assert not torch.equal(out["noise"], out["other"])
    return out


def test_eager_loop_equals_unet_plus_scheduler_step(tiny, eager):
    s = sched()
    gen = torch.Generator().manual_seed(3)  # the stream tiny["noise"] was drawn from
    x = tiny["lat"]
    for i, t in enumerate(s.timesteps):
        eps = tiny["unet"](torch.cat([x, x]), t, encoder_hidden_states=tiny["ehs"]).sample
        u, c = eps.chunk(2)
        state = gen.get_state()
        out = s.step(u + G * (c - u), t, x, generator=gen)
        # every step but the last draws once; the last draws nothing
        assert torch.equal(gen.get_state(), state) == (i == N_STEPS - 1)
        if i == N_STEPS - 1:
            assert torch.equal(out.prev_sample, out.denoised)
        x = out.prev_sample
    assert s.step_index == N_STEPS
    assert torch.equal(bits(x), bits(eager["noise"]))


def test_graph_replays_read_the_noise_inside_the_launch(tiny, eager):
    loop = DenoiseLoop(tiny["unet"], sched(), tiny["lat"], tiny["ehs"], G, use_graph=True, step_noise=tiny["noise"]).prime()
    assert loop.graph is not None, loop.graph_error
    assert torch.equal(bits(loop.run()), bits(eager["noise"]))
    assert int(loop.step_idx.item()) == N_STEPS
    loop.reset(tiny["lat"], step_noise=tiny["other"])
    assert torch.equal(bits(loop.run()), bits(eager["other"]))  # same capture, other noise
    loop.reset(tiny["lat"])  # None keeps the slabs
    assert torch.equal(bits(loop.run()), bits(eager["other"]))
    with pytest.raises(RuntimeError, match="scheduled steps"):
        loop.run(1)


def test_loop_refusals(tiny):
    u, lat, ehs = tiny["unet"], tiny["lat"], tiny["ehs"]
    with pytest.raises(ValueError, match="needs step_noise"):
        DenoiseLoop(u, sched(), lat, ehs, G)
    with pytest.raises(ValueError, match="step_noise of shape"):
        DenoiseLoop(u, sched(), lat, ehs, G, step_noise=tiny["noise"][:2])
    with pytest.raises(ValueError, match="step_noise of shape"):
        DenoiseLoop(u, sched(), lat, ehs, G, step_noise=tiny["noise"][:, :, :, :1])
    from vdiff import DDIMScheduler
    d = DDIMScheduler(beta_schedule="linear")
    d.set_timesteps(N_STEPS)
    with pytest.raises(ValueError, match="LCM scheduler"):
        DenoiseLoop(u, d, lat, ehs, G, step_noise=tiny["noise"])


# ---------------------------------------------------------------- pipelines
@pytest.fixture(scope="module")
def pipe(tiny):
    p = AnimateDiffPipeline(tiny["unet"], LCMScheduler.from_config(None, beta_schedule="linear"))
    p.torch_dtype = F32  # the noise dtype; fp32 so that scheduler.step's own draws are the same stream
    return p


def call_kw(tiny):
    neg, pos = tiny["ehs"].chunk(2)
    return dict(prompt_embeds=pos, negative_prompt_embeds=neg, num_frames=2, height=256, width=256,
                num_inference_steps=N_STEPS, guidance_scale=G, output_type="latent")


def test_pipeline_draws_in_diffusers_order(tiny, pipe):
    got = pipe(**call_kw(tiny), generator=torch.manual_seed(0)).frames
    # diffusers' loop by hand: the latents, then one draw inside every non-final scheduler.step
    gen = torch.manual_seed(0)
    x = randn_tensor((1, 4, 2, 32, 32), gen, device="cuda", dtype=F32)
    s = sched()
    for t in s.timesteps:
        u, c = tiny["unet"](torch.cat([x, x]), t, encoder_hidden_states=tiny["ehs"]).sample.chunk(2)
        x = s.step(u + G * (c - u), t, x, generator=gen).prev_sample
    assert torch.equal(bits(got), bits(x))


def test_pipeline_under_free_init_draws_each_iteration_after_the_filter(tiny, pipe):
    pipe.enable_free_init(num_iters=2)
    try:
        got = pipe(**call_kw(tiny), generator=torch.manual_seed(0)).frames
        gen = torch.manual_seed(0)
        x = randn_tensor((1, 4, 2, 32, 32), gen, device="cuda", dtype=F32)
        for i in range(2):
            x, ts = pipe._apply_free_init(x, i, N_STEPS, gen)       # iteration 1 draws z_rand here
            noise = torch.stack([randn_tensor(x.shape, gen, device="cuda", dtype=F32) for _ in range(N_STEPS - 1)])
            x = DenoiseLoop(tiny["unet"], pipe.scheduler, x, tiny["ehs"], G, timesteps=ts, use_graph=False,
                            step_noise=noise).prime().run().clone()
        assert torch.equal(bits(got), bits(x))
    finally:
        pipe.disable_free_init()
        pipe._free_init_initial_noise = pipe._free_init_table = pipe._free_init_scratch = None


def test_video_to_video_slices_the_lcm_schedule(tiny):
    """strength 0.5 of 4 steps runs the last two LCM timesteps: one draw, rows of the cut schedule."""
    from vdiff import AnimateDiffVideoToVideoPipeline
    v2v = AnimateDiffVideoToVideoPipeline.from_config("tiny", scheduler=LCMScheduler.from_config(None, beta_schedule="linear"))
    kw = call_kw(tiny)
    kw.pop("num_frames")
    got = v2v(**kw, latents=tiny["lat"], strength=0.5, generator=torch.manual_seed(0)).frames
    s = sched()
    ts = s.timesteps[2:]
    assert ts.tolist() == [499, 259]
    gen = torch.manual_seed(0)
    noise = torch.stack([randn_tensor(tiny["lat"].shape, gen, device="cuda", dtype=v2v.torch_dtype)]).float()
    want = DenoiseLoop(v2v.unet, s, tiny["lat"], tiny["ehs"], G, timesteps=ts, use_graph=False,
                       step_noise=noise).prime().run()
    assert torch.equal(bits(got), bits(want))


def test_frame_sharded_lcm_is_refused(tiny, pipe):
    pipe.dist = object()  # any frame shard: refused before it is used
    try:
        with pytest.raises(NotImplementedError, match="not sharded"):
            pipe(**call_kw(tiny))
    finally:
        pipe.dist = None
