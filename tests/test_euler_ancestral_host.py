"""EulerAncestralDiscreteScheduler on the CPU: diffusers' surface and config, the schedule it shares
with EulerDiscreteScheduler, the coefficient table against the restatement of diffusers' scheduler
(tests/euler_ancestral_ref.py, unpinned) bit for bit and against its fp64 form, the identities of
that fp64 table, the pipeline's step-noise draws, and every refusal before any launch.

Bounds of the fp32 table against fp64.  The estimate one would write down first — each radicand is 4
or 5 fp32 operations, the square root halves their relative error, the correctly rounded root adds
half an ulp: 2 fp32 ulps — does not hold, because it ignores cancellation: in t^2 - sigma_up^2
the two terms agree in their leading bits whenever sigma >> sigma_to (sigma_down ~ sigma_to^2 / sigma),
and sigma^2 - sigma_to^2 loses bits likewise when two sigmas are close (50 steps).  Measured over the
schedules below (steps {1, 2, 7, 25, 50} x the three spacings x linear / scaled_linear) against the
fp64 table: sigma_up at worst 2.506 ulps, sigma_down at worst 11918144.4 ulps (the 2-step linspace
schedule, 157 -> 0.01, where sigma_down = 6e-7 is all rounding error in diffusers' fp32 too).  The
bounds asserted are those worst cases plus one ulp.  Since an ulp bound on a cancelled value says
little, sigma_down's radicand is also held in absolute terms, by reasoning alone: sigma_up <= sigma_to
is within 3.5 ulps, so sigma_up^2 is within 2 * 3.5 * sigma_to * ulp(sigma_to) <= 10 ulp(sigma_to^2)
(x ulp(x) <= 1.42 ulp(x^2)), and the square, sigma_to^2, the subtraction and the final root add half
an ulp each at most: |sigma_down^2 - its fp64 value| <= 12 ulp(sigma_to^2)."""
import ctypes
import inspect
import types

import pytest
import torch

import euler_ancestral_ref as R
import vdiff
import vdiff._lib as L
from vdiff import EulerAncestralDiscreteScheduler as EA
from vdiff import EulerDiscreteScheduler, ops

STEPS = [1, 2, 7, 25, 50]
SPACINGS = ["linspace", "leading", "trailing"]
DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                trained_betas=None, prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0,
                rescale_betas_zero_snr=False)


def test_surface_is_diffusers():
    s = EA()
    assert (s.kind, s.order) == ("euler_a", 1)
    assert dict(s.config) == DEFAULTS
    assert list(inspect.signature(s.step).parameters) == ["model_output", "timestep", "sample", "generator",
                                                          "return_dict"]
    assert inspect.signature(s.step).parameters["generator"].default is None
    assert inspect.signature(s.step).parameters["return_dict"].default is True
    assert vdiff.EulerAncestralDiscreteSchedulerOutput._fields == ("prev_sample", "pred_original_sample")
    assert len(s) == 1000
    assert L.VD_STEP_ANCESTRAL == ops.STEP_ANCESTRAL == 0x4000
    assert ops.EULER_A_ROW == 4 and ops.euler_a_buffer_numel(3, 10) == 3 * 14
    assert ops.SCHED_STEP["euler_a"] is ops.euler_ancestral_cfg_step
    header = (L.LIB_PATH.parents[2] / "include" / "vdiff.h").read_text()
    assert "enum { VD_STEP_ANCESTRAL = 0x4000 }" in header


@pytest.mark.parametrize("other", [vdiff.DDIMScheduler, vdiff.EulerDiscreteScheduler, vdiff.LCMScheduler,
                                   vdiff.DPMSolverMultistepScheduler, vdiff.UniPCMultistepScheduler])
def test_from_config_of_every_other_scheduler(other):
    src = other().config
    s = EA.from_config(src)
    assert set(s.config) == set(DEFAULTS)
    for k in DEFAULTS:  # what the other config holds is taken, the rest keeps diffusers' default
        assert s.config[k] == (src[k] if k in src else DEFAULTS[k])
    s2 = EA.from_config(src, timestep_spacing="trailing", not_a_key=1)
    assert s2.config.timestep_spacing == "trailing" and "not_a_key" not in s2.config
    back = other.from_config(s.config)
    assert back.config["beta_schedule"] == s.config["beta_schedule"]


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("n", STEPS)
def test_schedule_is_eulers(n, spacing):
    kw = dict(timestep_spacing=spacing, steps_offset=1 if spacing == "leading" else 0)
    a, e = EA(**kw), EulerDiscreteScheduler(beta_start=0.0001, beta_end=0.02, beta_schedule="linear", **kw)
    assert torch.equal(a.sigmas, e.sigmas) and torch.equal(a.timesteps, e.timesteps)  # before set_timesteps
    a.set_timesteps(n)
    e.set_timesteps(n)
    assert torch.equal(a.timesteps, e.timesteps) and torch.equal(a.sigmas, e.sigmas)
    assert a.sigmas.dtype == torch.float32 and a.sigmas[-1] == 0 and len(a.sigmas) == n + 1
    assert a.init_noise_sigma == e.init_noise_sigma
    assert [a.input_divisor(i) for i in range(n)] == [e.input_divisor(i) for i in range(n)]
    ts, sig = R.set_timesteps(n, spacing, kw["steps_offset"])
    assert torch.equal(a.timesteps, ts) and torch.equal(a.sigmas, sig)
    assert a.init_noise_sigma == R.init_noise_sigma(sig, spacing)
    x, noise = torch.randn(2, 4, 1, 3, 3), torch.randn(2, 4, 1, 3, 3)
    t = a.timesteps[[0, n // 2]]
    assert torch.equal(a.add_noise(x, noise, t), e.add_noise(x, noise, t))
    assert torch.equal(a.scale_model_input(x, a.timesteps[0]), e.scale_model_input(x, e.timesteps[0]))
    a.set_begin_index(n - 1)
    a._step_index = None
    a._init_step_index(a.timesteps[0])
    assert a.step_index == n - 1


def test_repeated_timestep_takes_the_second_match():
    a = EA()
    a.set_timesteps(7)
    st = torch.tensor([999.0, 500.0, 500.0, 1.0])
    assert a.index_for_timestep(500.0, st) == 2 and a.index_for_timestep(999.0, st) == 0
    with pytest.raises(ValueError, match="not in the schedule"):
        a.index_for_timestep(3.0)


# worst case measured over this file's schedules against the fp64 table, plus one ulp (module docstring)
UP_ULPS = 2.506 + 1
DOWN_ULPS = 11918144.4 + 1


def ulp32(x):
    """The fp32 ulp at |x| (fp64 tensor in, fp64 out)."""
    x = x.abs().float()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


@pytest.mark.parametrize("schedule", ["linear", "scaled_linear"])
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("n", STEPS)
def test_table_equals_the_restatement_and_is_close_to_fp64(n, spacing, schedule):
    off = 1 if spacing == "leading" else 0
    s = EA(timestep_spacing=spacing, steps_offset=off, beta_schedule=schedule)
    s.set_timesteps(n)
    acp = R.alphas_cumprod(schedule=schedule)
    assert torch.equal(acp, s.alphas_cumprod)
    ts, sig = R.set_timesteps(n, spacing, off, acp)
    assert torch.equal(s.sigmas, sig)
    tab = s.coefficient_table()
    assert tab.shape == (n, 4) and tab.dtype == torch.float32
    want = R.table(sig)
    assert torch.equal(tab.view(torch.int32), want.view(torch.int32))
    for i in range(n):
        assert torch.equal(s.coefficients(i), tab[i])
    assert torch.equal(tab[:, 0], sig[:-1])
    # a sub-schedule (the video-to-video slice) and a timestep repeated past the schedule
    if n > 2:
        assert torch.equal(s.coefficient_table(s.timesteps[1:]), tab[1:])
        assert torch.equal(s.coefficient_table(torch.cat([s.timesteps, s.timesteps[:2]])), torch.cat([tab, tab[:2]]))
    t64 = R.table(sig, torch.float64)
    for col, name, bound in ((3, "sigma_up", UP_ULPS), (1, "sigma_down", DOWN_ULPS)):
        err = (tab[:, col].double() - t64[:, col]).abs() / ulp32(t64[:, col])
        worst = err.max().item()
        print(f"TABLE {schedule} {spacing} n={n}: {name} worst {worst:.3f} ulp")
        assert worst <= bound, (name, worst)
    rad = (tab[:, 1].double() ** 2 - t64[:, 1] ** 2).abs() / ulp32(sig[1:].double() ** 2)
    print(f"TABLE {schedule} {spacing} n={n}: sigma_down^2 worst {rad[:-1].max().item() if n > 1 else 0:.3f} ulp of sigma_to^2")
    assert (rad[:-1] <= 12).all() and rad[-1] == 0


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("n", STEPS)
def test_fp64_table_identities(n, spacing):
    off = 1 if spacing == "leading" else 0
    _, sig = R.set_timesteps(n, spacing, off)
    t = R.table(sig, torch.float64)
    s, down, div, up = t.unbind(1)
    to = sig[1:].double()
    assert torch.allclose(down ** 2 + up ** 2, to ** 2, rtol=1e-12, atol=0)
    assert t[-1].tolist() == [float(sig[-2]), 0.0, 1.0, 0.0]
    assert (down[:-1] < to[:-1]).all() and (up[:-1] > 0).all() and (down[:-1] > 0).all()
    assert torch.equal(div, torch.sqrt(to ** 2 + 1))
    f32 = R.table(sig)
    assert f32[-1].tolist() == [float(sig[-2]), 0.0, 1.0, 0.0]  # the fp32 table's last row reads no slab


def test_zero_noise_loop_is_an_euler_loop_to_sigma_down():
    n = 7
    _, sig = R.set_timesteps(n)
    tab = R.table(sig)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 3, 5, 5, generator=g) * sig[0]
    eps = [torch.randn(2, 4, 3, 5, 5, generator=g) for _ in range(n)]
    zeros = [torch.zeros_like(x) for _ in range(n)]
    got, x0s = R.loop(x, eps, zeros, tab)
    # the same loop written independently: EulerDiscreteScheduler's update towards sigma_down
    y = x.clone()
    for i in range(n):
        sigma = sig[i]
        up = torch.sqrt((sig[i + 1] ** 2 * (sigma ** 2 - sig[i + 1] ** 2) / sigma ** 2).double()).float()
        down = torch.sqrt((sig[i + 1] ** 2 - up ** 2).double()).float()
        pred = y - sigma * eps[i]
        assert torch.equal(pred, x0s[i])
        y = y + (y - pred) / sigma * (down - sigma)
    assert torch.equal(got, y)
    assert torch.allclose(got, x0s[-1], rtol=1e-4, atol=1e-5)  # sigma_down = 0 at the end: the sample is x0
    # and the noise does matter on every step but the last
    noisy, _ = R.loop(x, eps, [torch.ones_like(x)] * n, tab)
    assert not torch.equal(noisy, got)
    nan_last = zeros[:-1] + [torch.full_like(x, float("nan"))]
    assert torch.equal(R.loop(x, eps, nan_last, tab)[0], got)


def pipeline(sched=None, dtype=None):
    p = vdiff.AnimateDiffPipeline(vdiff.UNetMotionModel("tiny"), sched or EA())
    p.torch_dtype = dtype
    return p


@pytest.mark.parametrize("dtype", [None, torch.float32, torch.float16])
def test_step_noise_is_n_draws_in_step_order_in_torch_dtype(dtype):
    p = pipeline(dtype=dtype)
    lat = torch.zeros(1, 4, 2, 3, 5)
    got = p._step_noise(lat, 4, torch.Generator().manual_seed(7))
    assert got.shape == (4, 1, 4, 2, 3, 5) and got.dtype == torch.float32
    gen = torch.Generator().manual_seed(7)
    want = torch.stack([torch.randn(lat.shape, generator=gen, dtype=dtype or torch.float32) for _ in range(4)]).float()
    assert torch.equal(got, want)
    assert torch.equal(p._step_noise(lat, 4, torch.Generator().manual_seed(7)), got)
    assert not torch.equal(got[0], got[1])
    z = p._step_noise(lat, 4, None, draw=False)
    assert z.shape == got.shape and z.dtype == torch.float32 and not z.any()
    assert pipeline(vdiff.EulerDiscreteScheduler())._step_noise(lat, 4, None) is None


@pytest.mark.parametrize("kw, name", [(dict(prediction_type="v_prediction"), "prediction_type"),
                                      (dict(prediction_type="sample"), "prediction_type"),
                                      (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"),
                                      (dict(beta_schedule="squaredcos_cap_v2"), "beta_schedule")])
def test_config_refusals_raise_by_name(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        EA(**kw)
    with pytest.raises(NotImplementedError, match=name):
        EA.from_config(vdiff.DDIMScheduler().config, **kw)


def test_step_refuses_cpu_tensors_and_a_missing_schedule():
    s = EA()
    x = torch.zeros(1, 4, 2, 8, 8)
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(x, 999, x)
    s.set_timesteps(4)
    with pytest.raises(ValueError, match="GPU"):
        s.step(x, 999, x)


def test_frame_sharded_pipeline_is_refused_by_name():
    p = pipeline()
    p._refuse_scheduler_combinations()  # unsharded: nothing to refuse, FreeInit included
    p.enable_free_init(num_iters=2)
    p._refuse_scheduler_combinations()
    p.disable_free_init()
    p.dist = object()  # any frame shard: refused before it is used
    with pytest.raises(NotImplementedError, match="EulerAncestralDiscreteScheduler.*not sharded"):
        p._refuse_scheduler_combinations()
    with pytest.raises(NotImplementedError, match="not sharded"):
        p(prompt_embeds=torch.zeros(1, 77, 64), num_frames=2, height=64, width=64, num_inference_steps=2,
          output_type="latent")


def test_dit_loop_refuses_the_scheduler_by_name():
    from vdiff.models.dit import DiTDenoiseLoop
    s = EA()
    s.set_timesteps(4)
    model = types.SimpleNamespace(device=torch.device("cpu"))  # refused before the model is touched
    with pytest.raises(NotImplementedError, match="EulerAncestralDiscreteScheduler"):
        DiTDenoiseLoop(model, s, torch.zeros(1, 4, 2, 8, 8), torch.zeros(2, 77, 64), 7.5)


def test_load_scheduler_maps_the_class_name(tmp_path):
    import json

    from vdiff.pretrained import load_scheduler
    cfg = dict(DEFAULTS, _class_name="EulerAncestralDiscreteScheduler", _diffusers_version="0.30.0",
               beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    (tmp_path / "scheduler_config.json").write_text(json.dumps(cfg))
    s = load_scheduler(tmp_path)
    assert isinstance(s, EA) and s.config.beta_schedule == "scaled_linear" and s.config.beta_end == 0.012


def test_entry_point_validates_the_flag_before_any_launch():
    """VD_STEP_ANCESTRAL rides on vd_euler_cfg_step's ncfg: with a sibling scheduler flag, a stray
    bit, a low byte of 3 without PAG or an unaligned coef it is VD_EINVAL, and vd_ddim_cfg_step
    refuses it.  No GPU needed: every call returns before a launch."""
    h = L.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    A = L.VD_STEP_ANCESTRAL
    args = lambda ncfg, coef=p: (p, 8, ncfg, 1.0, p, 1, 4, 1, 2, 2, coef, 1, None, None, None, 0, None)  # noqa: E731
    for sibling in (L.VD_STEP_LCM, L.VD_STEP_DPM, L.VD_STEP_UNIPC, 0x200, 0x1000, 0x8000):
        for low in (1, 2):
            assert h.vd_euler_cfg_step(*args(low | A | sibling)) == L.VD_EINVAL
            assert h.vd_euler_cfg_step(*args(low | A | L.VD_STEP_PAG | sibling)) == L.VD_EINVAL
    assert h.vd_euler_cfg_step(*args(A)) == L.VD_EINVAL
    assert h.vd_euler_cfg_step(*args(3 | A)) == L.VD_EINVAL
    assert h.vd_euler_cfg_step(*args(1 | A | L.VD_STEP_PAG)) == L.VD_EINVAL
    assert h.vd_euler_cfg_step(*args(1 | A, coef=p + 4)) == L.VD_EINVAL
    assert h.vd_euler_cfg_step(*args(2 | A, coef=p + 8)) == L.VD_EINVAL
    assert h.vd_euler_cfg_step(*args(2 | A | L.VD_STEP_PAG, coef=p + 4)) == L.VD_EINVAL
    for low in (1, 2):
        assert h.vd_ddim_cfg_step(*args(low | A)) == L.VD_EINVAL
        assert h.vd_ddim_cfg_step(*args(low | A | L.VD_STEP_LCM)) == L.VD_EINVAL
    # what stayed refused on the unflagged entry point
    for bit in (L.VD_STEP_LCM, L.VD_STEP_DPM, L.VD_STEP_UNIPC, 0x200, 0x1000):
        assert h.vd_euler_cfg_step(*args(1 | bit)) == L.VD_EINVAL
    assert h.vd_version() == 6


def test_ops_step_needs_gpu_tensors():
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.euler_ancestral_cfg_step(torch.zeros(4, 1), 1, 1.0, torch.zeros(1, 1, 1, 1, 4), torch.zeros(8))
