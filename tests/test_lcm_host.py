"""LCMScheduler on the CPU: the timestep rule, the coefficient rows against the restatement of
diffusers' scheduler (tests/lcm_ref.py, unpinned), the refusals, and the entry point's argument
checks before any launch."""
import ctypes

import pytest
import torch

import lcm_ref as R
import vdiff
import vdiff._lib as L
from vdiff import LCMScheduler, ops


def test_surface():
    s = LCMScheduler()
    assert (s.kind, s.order, s.init_noise_sigma) == ("lcm", 1, 1.0)
    want = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                trained_betas=None, original_inference_steps=50, clip_sample=False, clip_sample_range=1.0,
                set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon", thresholding=False,
                timestep_spacing="leading", timestep_scaling=10.0, rescale_betas_zero_snr=False)
    assert dict(s.config) == want
    s2 = LCMScheduler.from_config(vdiff.DDIMScheduler().config, beta_schedule="linear")
    assert s2.config.beta_schedule == "linear" and s2.config.original_inference_steps == 50
    assert L.VD_STEP_LCM == ops.STEP_LCM == 0x100
    assert ops.SCHED_STEP["lcm"] is ops.lcm_cfg_step
    x = torch.randn(2, 3)
    assert s.scale_model_input(x, 5) is x


def test_timesteps_of_the_default_config():
    s = LCMScheduler()
    s.set_timesteps(4)
    assert s.timesteps.tolist() == [999, 759, 499, 259]
    assert s.timesteps.dtype == torch.int64
    s.set_timesteps(8)
    assert s.timesteps.tolist() == [999, 879, 759, 639, 499, 379, 259, 139]


@pytest.mark.parametrize("n, orig, strength", [(4, None, 0.5), (6, None, 1.0), (3, 20, 0.8), (50, None, 1.0)])
def test_timesteps_match_the_restatement(n, orig, strength):
    s = LCMScheduler()
    s.set_timesteps(n, original_inference_steps=orig, strength=strength)
    assert s.timesteps.tolist() == R.lcm_timesteps(n, original_steps=orig or 50, strength=strength).tolist()
    assert s.num_inference_steps == n


def test_set_timesteps_value_errors():
    s = LCMScheduler()
    with pytest.raises(ValueError, match="num_inference_steps"):
        s.set_timesteps(51)  # more steps than the 50 the origin schedule holds
    with pytest.raises(ValueError, match="smaller than"):
        s.set_timesteps(30, strength=0.5)  # origin holds 25
    with pytest.raises(ValueError, match="original_steps"):
        s.set_timesteps(4, original_inference_steps=2000)


@pytest.mark.parametrize("schedule", ["scaled_linear", "linear"])
@pytest.mark.parametrize("n", [1, 4, 6])
def test_table_rows_equal_the_restatement_bit_for_bit(schedule, n):
    s = LCMScheduler(beta_schedule=schedule)
    s.set_timesteps(n)
    acp = R.alphas_cumprod(schedule=schedule)
    assert torch.equal(acp, s.alphas_cumprod)
    ts = s.timesteps.tolist()
    tab = s.coefficient_table()
    assert tab.shape == (n, 8) and tab.dtype == torch.float32
    assert torch.equal(tab, R.table(ts, acp))
    for i in range(n):
        assert torch.equal(s.coefficients(i), tab[i])
    # the last row adds no noise, every other one does; the pad column is 0
    assert tab[:, 6].tolist() == [1.0] * (n - 1) + [0.0]
    assert tab[:, 7].tolist() == [0.0] * n
    # a_prev of row i is the alpha of the NEXT schedule timestep, not of t - T // n
    for i in range(n - 1):
        a_next = s.alphas_cumprod[ts[i + 1]]
        assert tab[i, 2] == torch.sqrt(a_next.double()).float()
        assert tab[i, 3] == torch.sqrt((1 - a_next).double()).float()
    # a sub-schedule (the video-to-video pipeline's slice) takes its own next timesteps
    if n > 2:
        assert torch.equal(s.coefficient_table(s.timesteps[1:]), tab[1:])


def test_boundary_scalings_in_fp64_rounded_once():
    s = LCMScheduler()
    s.set_timesteps(4)
    tab = s.coefficient_table()
    for i, t in enumerate(s.timesteps.tolist()):
        st = t * 10.0
        assert tab[i, 4].item() == torch.tensor(0.25 / (st * st + 0.25), dtype=torch.float64).float().item()
        assert tab[i, 5].item() == torch.tensor(st / (st * st + 0.25) ** 0.5, dtype=torch.float64).float().item()


def test_add_noise_is_ddims():
    s, d = LCMScheduler(), vdiff.DDIMScheduler(beta_schedule="scaled_linear")
    x, n = torch.randn(2, 4, 3, 5, 5), torch.randn(2, 4, 3, 5, 5)
    assert torch.equal(s.add_noise(x, n, torch.tensor([999, 499])), d.add_noise(x, n, torch.tensor([999, 499])))


@pytest.mark.parametrize("kw, name", [(dict(prediction_type="v_prediction"), "prediction_type"),
                                      (dict(prediction_type="sample"), "prediction_type"),
                                      (dict(clip_sample=True), "clip_sample"),
                                      (dict(thresholding=True), "thresholding"),
                                      (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr")])
def test_refusals_raise_by_name(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        LCMScheduler(**kw)


def test_step_refuses_cpu_tensors_and_a_missing_schedule():
    s = LCMScheduler()
    x = torch.zeros(1, 4, 2, 8, 8)
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(x, 999, x)
    s.set_timesteps(4)
    with pytest.raises(ValueError, match="GPU"):
        s.step(x, 999, x)


def test_entry_point_validates_the_flag_before_any_launch():
    """VD_STEP_LCM rides on ncfg: the low byte stays 1 or 2, any other high bit is VD_EINVAL, an
    unaligned coef buffer is refused, and vd_euler_cfg_step refuses the flag.  No GPU needed:
    every call returns before a launch."""
    h = L.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    args = lambda ncfg, coef=p: (p, 8, ncfg, 1.0, p, 1, 4, 1, 2, 2, coef, 1, None, None, None, 0, None)  # noqa: E731
    assert h.vd_ddim_cfg_step(*args(1 | 0x200)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(2 | 0x100 | 0x200)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(3 | 0x100)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(0x100)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(1 | 0x100, coef=p + 4)) == L.VD_EINVAL
    assert h.vd_euler_cfg_step(*args(1 | 0x100)) == L.VD_EINVAL
    assert h.vd_euler_cfg_step(*args(2 | 0x100)) == L.VD_EINVAL


def test_ops_lcm_cfg_step_checks_the_buffer_size():
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.lcm_cfg_step(torch.zeros(4, 1), 1, 1.0, torch.zeros(1, 1, 1, 1, 4), torch.zeros(12))
    assert ops.lcm_buffer_numel(3, 10) == 3 * 18


def test_ddim_eta_refusal_points_at_lcm():
    s = vdiff.DDIMScheduler()
    s.set_timesteps(4)
    x = torch.zeros(1, 4, 2, 8, 8)
    with pytest.raises(NotImplementedError, match="LCMScheduler"):
        s.step(x, 1, x, eta=0.5)
