"""UniPCMultistepScheduler on the CPU: config and refusals, the entry point's argument checks
before any launch, timesteps / sigmas against DPMSolverMultistepScheduler's, the per-row corrector
and order decisions and the coefficient rows against the restatement of diffusers' scheduler
(tests/unipc_ref.py, unpinned), and the restatement itself against the analytic solution of a
Gaussian toy model, on its order of convergence.

Bars (none taken from a device):
  * timesteps, sigmas, flags and every slot but the corrector's two weights: equality.
  * the corrector's weights (rho0, rhot): closed form against torch.linalg.solve in fp64, 1e-12
    relative (a 2x2 system with rk < 0, condition number below 10: a few fp64 roundings); in the
    fp32 table one ulp (2^-23 relative), the two fp64 values rounding apart at worst.
  * the order of convergence, fp64, n = 40 -> 80 steps: the error falls by >= 6 with the corrector
    (third order: theory 8) and by a factor in [3, 6] without it (second order: theory 4).
    Measured on the CPU: 8.5 and 4.4 ("bh2"), through the restatement and through the host rows.
"""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import unipc_ref as R
import vdiff
import vdiff._lib as L
from vdiff import DPMSolverMultistepScheduler, UniPCMultistepScheduler, UniPCMultistepSchedulerOutput, ops
from vdiff.sched.unipc import unipc_row, unipc_row64

F32, F64 = torch.float32, torch.float64
SPACINGS = ["linspace", "leading", "trailing"]
FINALS = ["zero", "sigma_min"]
RHO = [6, 7]                                            # the corrector's weights' slots
REST = [j for j in range(16) if j not in RHO]


def sched(n=None, **kw):
    s = UniPCMultistepScheduler(**kw)
    if n is not None:
        s.set_timesteps(n)
    return s


def ref_for(s, **kw):
    c = s.config
    return R.UniPCRef(solver_order=c.solver_order, solver_type=c.solver_type, disable_corrector=c.disable_corrector,
                      use_karras_sigmas=c.use_karras_sigmas, final_sigmas_type=c.final_sigmas_type,
                      timestep_spacing=c.timestep_spacing, steps_offset=c.steps_offset, beta_schedule=c.beta_schedule,
                      beta_start=c.beta_start, beta_end=c.beta_end, trained_betas=c.trained_betas,
                      num_train_timesteps=c.num_train_timesteps, **kw)


def assert_rows_equal(got, want, case=None):
    assert got.shape == want.shape and got.dtype == want.dtype == F32, case
    assert torch.equal(got[:, REST], want[:, REST]), case
    g, w = got[:, RHO].double(), want[:, RHO].double()
    assert bool(((g - w).abs() <= 2.0 ** -23 * w.abs()).all()), case


# ---------------------------------------------------------------- config and wiring
def test_surface_and_defaults():
    s = UniPCMultistepScheduler()
    assert (s.kind, s.order, s.init_noise_sigma) == ("unipc", 1, 1.0)
    want = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                sample_max_value=1.0, predict_x0=True, solver_type="bh2", lower_order_final=True, disable_corrector=[],
                solver_p=None, use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False,
                use_flow_sigmas=False, timestep_spacing="linspace", steps_offset=0, final_sigmas_type="zero",
                rescale_betas_zero_snr=False)
    assert dict(s.config) == want
    s2 = UniPCMultistepScheduler.from_config(vdiff.DDIMScheduler().config, use_karras_sigmas=True)
    assert (s2.config.beta_schedule, s2.config.beta_start, s2.config.steps_offset) == ("scaled_linear", 0.00085, 1)
    assert s2.config.use_karras_sigmas and s2.config.solver_order == 2 and s2.bh2
    assert torch.equal(s2.alphas_cumprod, vdiff.DDIMScheduler().alphas_cumprod)
    assert L.VD_STEP_UNIPC == ops.STEP_UNIPC == 0x2000 and ops.UNIPC_ROW == 16
    assert ops.SCHED_STEP["unipc"] is ops.unipc_cfg_step
    assert vdiff.sched.UniPCMultistepScheduler is UniPCMultistepScheduler
    assert UniPCMultistepSchedulerOutput._fields == ("prev_sample",)
    x = torch.randn(2, 3)
    assert s.scale_model_input(x, 5) is x
    assert len(s) == 1000
    # the line that used to fail: another scheduler's config goes in, diffusers' fields it lacks default
    s3 = UniPCMultistepScheduler.from_config(DPMSolverMultistepScheduler(use_karras_sigmas=True).config)
    assert s3.config.use_karras_sigmas and s3.config.solver_type == "bh2"   # diffusers': "midpoint" becomes "bh2"


@pytest.mark.parametrize("kw, name", [
    (dict(solver_order=3), "solver_order=3"),
    (dict(predict_x0=False), "predict_x0=False"),
    (dict(lower_order_final=False), "lower_order_final=False"),
    (dict(solver_p=object()), "solver_p"),
    (dict(thresholding=True), "thresholding"),
    (dict(prediction_type="v_prediction"), "prediction_type"),
    (dict(prediction_type="sample"), "prediction_type"),
    (dict(prediction_type="flow_prediction"), "prediction_type"),
    (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"),
    (dict(use_exponential_sigmas=True), "use_exponential_sigmas"),
    (dict(use_beta_sigmas=True), "use_beta_sigmas"),
    (dict(use_flow_sigmas=True), "use_flow_sigmas"),
])
def test_refusals_raise_by_name(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        UniPCMultistepScheduler(**kw)


def test_bad_values_are_value_errors():
    for kw in (dict(solver_order=0), dict(solver_type="bh3"), dict(final_sigmas_type="one"),
               dict(timestep_spacing="log")):
        with pytest.raises(ValueError):
            UniPCMultistepScheduler(**kw)


def test_step_refuses_cpu_tensors_and_a_missing_schedule():
    s = UniPCMultistepScheduler()
    x = torch.zeros(1, 4, 2, 8, 8)
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(x, 999, x)
    with pytest.raises(ValueError, match="set_timesteps"):
        s.coefficient_table()
    s.set_timesteps(4)
    with pytest.raises(ValueError, match="GPU"):
        s.step(x, 999, x)
    with pytest.raises(ValueError, match="no run of the current schedule"):
        s.coefficient_table(torch.tensor([5, 3]))


def test_entry_point_validates_before_any_launch():
    """VD_STEP_UNIPC rides on ncfg: the low byte stays 1 or 2 (2 or 3 under VD_STEP_PAG), it does
    not combine with VD_STEP_LCM, VD_STEP_DPM, 0x200 or 0x1000, x0_out is required and its three
    slabs do not overlap the latents, coef is 16-byte aligned, and vd_euler_cfg_step refuses the
    flag.  Host pointers: every refused call returns before a launch, and each differs from a valid
    one in the argument named alone.  The valid word itself is only called where no GPU is
    visible — there the launch fails in the runtime, with a status that is not VD_EINVAL; with a
    GPU it runs on device operands in tests/test_gpu_unipc.py."""
    h = L.lib()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 15) & ~15
    lat, state, N = p + 2048, p + 4096, 4 * 1 * 4 * 1 * 2 * 2     # bytes of one slab
    U, PAG = L.VD_STEP_UNIPC, L.VD_STEP_PAG

    def args(ncfg, coef=p, x0=state):
        return (p, 8, ncfg, 1.0, lat, 1, 4, 1, 2, 2, coef, 1, None, x0, None, 0, None)
    for bad in (1 | U | L.VD_STEP_LCM, 1 | U | L.VD_STEP_DPM, 2 | U | L.VD_STEP_LCM | L.VD_STEP_DPM,
                1 | U | 0x200, 1 | U | 0x1000, 2 | U | 0x200, 2 | U | 0x1000,
                U, 3 | U, 4 | U, 0xFF | U,
                1 | U | PAG, 4 | U | PAG, U | PAG, 2 | U | PAG | L.VD_STEP_DPM, 3 | U | PAG | 0x1000):
        assert h.vd_ddim_cfg_step(*args(bad)) == L.VD_EINVAL, hex(bad)
    assert h.vd_ddim_cfg_step(*args(1 | 0x200)) == L.VD_EINVAL          # as before the flag existed
    assert h.vd_ddim_cfg_step(*args(1 | 0x1000)) == L.VD_EINVAL
    for word in (1 | U, 2 | U, 2 | U | PAG, 3 | U | PAG):
        assert h.vd_ddim_cfg_step(*args(word, x0=None)) == L.VD_EINVAL, hex(word)
        assert h.vd_ddim_cfg_step(*args(word, coef=p + 4)) == L.VD_EINVAL, hex(word)
        assert h.vd_ddim_cfg_step(*args(word, coef=None)) == L.VD_EINVAL, hex(word)
        # [x0_out, x0_out + 3N) against [latents, latents + N): equal, its tail on the latents' first
        # float, its head on their last, the latents inside the second slab
        for x0 in (lat, lat - 3 * N + 4, lat + N - 4, lat - N):
            assert h.vd_ddim_cfg_step(*args(word, x0=x0)) == L.VD_EINVAL, (hex(word), x0 - lat)
        assert h.vd_euler_cfg_step(*args(word)) == L.VD_EINVAL, hex(word)
    if not torch.cuda.is_available():
        for word in (1 | U, 2 | U, 2 | U | PAG, 3 | U | PAG):
            assert h.vd_ddim_cfg_step(*args(word)) != L.VD_EINVAL, hex(word)
            assert h.vd_ddim_cfg_step(*args(word, x0=lat + N)) != L.VD_EINVAL     # adjacent is no overlap
            assert h.vd_ddim_cfg_step(*args(word, x0=lat - 3 * N)) != L.VD_EINVAL
    assert h.vd_version() == 6


def test_ops_unipc_cfg_step_checks_its_operands():
    lat = torch.zeros(1, 1, 1, 1, 4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.unipc_cfg_step(torch.zeros(4, 1), 1, 1.0, lat, torch.zeros(1, 16), x0_out=torch.zeros(12))


# ---------------------------------------------------------------- the schedule
@pytest.mark.parametrize("n", [1, 4, 16, 25])
def test_timesteps_and_sigmas_equal_dpm_solvers(n):
    for karras, spacing, final, betas in itertools.product(
            [False, True], SPACINGS, FINALS,
            [{}, dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012, steps_offset=1),
             dict(trained_betas=torch.linspace(1e-4, 2e-2, 100).tolist(), num_train_timesteps=100)]):
        kw = dict(use_karras_sigmas=karras, timestep_spacing=spacing, final_sigmas_type=final, **betas)
        s = sched(n, **kw)
        d = DPMSolverMultistepScheduler(**kw)
        d.set_timesteps(n)
        assert s.timesteps.dtype == torch.int64 and s.num_inference_steps == n
        assert torch.equal(s.timesteps, d.timesteps), kw
        assert s.sigmas.dtype == F32 and s.sigmas.shape == (n + 1,)
        assert torch.equal(s.sigmas.view(torch.int32), d.sigmas.view(torch.int32)), kw
        ref = ref_for(s).set_timesteps(n)
        assert torch.equal(s.timesteps, ref.timesteps) and torch.equal(s.sigmas, ref.sigmas), kw


def test_index_for_timestep_and_add_noise():
    s = sched(5)
    ts = s.timesteps.tolist()
    assert [s.index_for_timestep(t) for t in ts] == list(range(5))
    assert s.index_for_timestep(12345) == 4                             # diffusers' fall-back: the last index
    x, nz = torch.randn(2, 4, 3, 5, 5), torch.randn(2, 4, 3, 5, 5)
    got = s.add_noise(x, nz, torch.tensor([ts[1], ts[3]]))
    sg = s.sigmas[[1, 3]].double()
    a = 1 / (sg * sg + 1).sqrt()
    want = a.float().view(2, 1, 1, 1, 1) * x + (sg * a).float().view(2, 1, 1, 1, 1) * nz
    assert torch.equal(got, want)
    s.set_begin_index(2)                                                # as diffusers: begin_index wins
    got = s.add_noise(x, nz, torch.tensor([ts[0], ts[0]]))
    sg = s.sigmas[[2, 2]].double()
    a = 1 / (sg * sg + 1).sqrt()
    assert torch.equal(got, a.float().view(2, 1, 1, 1, 1) * x + (sg * a).float().view(2, 1, 1, 1, 1) * nz)


# ---------------------------------------------------------------- flags and rows
def expected_flags(decisions):
    return [float((c > 0) + 2 * (c == 2) + 4 * (p == 2)) for c, p in decisions]


@pytest.mark.parametrize("n", [1, 2, 3, 10])
@pytest.mark.parametrize("kw", [{}, dict(disable_corrector=[0, 3]), dict(solver_order=1),
                                dict(solver_type="bh1", use_karras_sigmas=True, final_sigmas_type="sigma_min")],
                         ids=["default", "disable_corrector", "order1", "bh1_karras_sigma_min"])
def test_flags_and_rows_follow_the_restatements_decisions(n, kw):
    s = sched(n, **kw)
    ref = ref_for(s, coef="rows").set_timesteps(n)
    tab = s.coefficient_table()
    assert tab.shape == (n, 16) and tab.dtype == F32 and torch.isfinite(tab).all()
    dec = ref.decisions()
    assert tab[:, 12].tolist() == expected_flags(dec), (n, kw)
    assert_rows_equal(tab, ref.table(), (n, kw))
    assert tab[0, 12] == 0 and tab[0, 2:8].abs().max() == 0             # row 0: no corrector, first order
    assert tab[:, 13:].abs().max() == 0
    for i in range(n):
        r, fl = tab[i], int(tab[i, 12])
        assert torch.equal(s.coefficients(i), r)
        if not fl & 1:
            assert r[2:8].abs().max() == 0, (n, kw, i)
        if fl & 1 and not fl & 2:
            assert r[5] == 0 and r[6] == 0 and r[7] == 0.5, (n, kw, i)
        if fl & 2:
            assert fl & 1 and r[5] < 0, (n, kw, i)
        if not fl & 4:
            assert r[10] == 0 and r[11] == 0, (n, kw, i)
        else:
            assert r[11] < 0, (n, kw, i)
    # what the decisions are, spelled out
    so = s.config.solver_order
    for i, (c, p) in enumerate(dec):
        assert p == min(so, n - i, i + 1)
        assert c == (0 if i == 0 or (i - 1) in s.config.disable_corrector else min(so, i))
    if s.config.final_sigmas_type == "zero":
        assert tab[-1, 8:12].tolist() == [0.0, -1.0, 0.0, 0.0]          # x_next = m_t


def test_disable_corrector_and_order_one_spelled_out():
    f = sched(10, disable_corrector=[0, 3]).coefficient_table()[:, 12].tolist()
    assert f == [0.0, 4.0, 7.0, 7.0, 4.0, 7.0, 7.0, 7.0, 7.0, 3.0]
    f = sched(10).coefficient_table()[:, 12].tolist()
    assert f == [0.0, 5.0] + [7.0] * 7 + [3.0]
    f = sched(10, solver_order=1).coefficient_table()[:, 12].tolist()
    assert f == [0.0] + [1.0] * 9
    assert sched(2).coefficient_table()[:, 12].tolist() == [0.0, 1.0]
    assert sched(3).coefficient_table()[:, 12].tolist() == [0.0, 5.0, 3.0]


def test_a_sliced_schedule_starts_fresh():
    for kw in ({}, dict(disable_corrector=[0, 3]), dict(solver_order=1)):
        s = sched(10, use_karras_sigmas=True, **kw)
        full = s.coefficient_table()
        s.set_begin_index(3)
        cut = s.coefficient_table(s.timesteps[3:])
        assert cut.shape == (7, 16)
        assert cut[0, 12] == 0 and cut[0, 2:8].abs().max() == 0 and cut[0, 10:12].abs().max() == 0
        assert torch.equal(cut[0, [0, 1, 8, 9]], full[3, [0, 1, 8, 9]])
        ref = ref_for(s, coef="rows").set_timesteps(10)
        assert cut[:, 12].tolist() == expected_flags(ref.decisions(start=3))
        assert_rows_equal(cut, ref.table(start=3))
        # the corrector goes by the schedule's index: step 3 disabled means no corrector at index 4, row 1
        if kw.get("disable_corrector"):
            assert int(cut[1, 12]) & 1 == 0
        else:
            assert int(cut[1, 12]) & 3 == 1                             # first order: one step taken
        assert torch.equal(cut[2:], full[5:])                           # from the third step on, as the full run
        s.set_begin_index(None)
        assert torch.equal(s.coefficient_table(s.timesteps[3:]), cut)   # found by position without begin_index


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
def test_closed_form_rho_equals_linalg_solve(karras, solver_type):
    s = sched(20, use_karras_sigmas=karras, solver_type=solver_type)
    ref = ref_for(s, coef="rows").set_timesteps(20)
    sig = s.sigmas.tolist()
    seen = 0
    for i, (c, p) in enumerate(ref.decisions()):
        got = unipc_row64(sig, i, c, p, s.bh2)
        want = R.row(ref.sigmas, i, c, p, s.bh2, rounded=False)
        assert got.dtype == want.dtype == F64
        assert torch.equal(got[REST], want[REST]), i
        if c == 2:
            seen += 1
            assert bool(((got[RHO] - want[RHO]).abs() <= 1e-12 * want[RHO].abs()).all()), (i, got[RHO], want[RHO])
            # the system itself: rho0 + rhot = b1, rk rho0 + rhot = b2
            assert want[6] > 0 and want[7] > 0
        else:
            assert torch.equal(got[RHO], want[RHO])
    assert seen == 18


@pytest.mark.parametrize("n", [1, 2, 5, 20, 50])
def test_every_table_is_finite(n):
    for karras, spacing, final, st, so in itertools.product([False, True], SPACINGS, FINALS, ["bh1", "bh2"], [1, 2]):
        tab = sched(n, use_karras_sigmas=karras, timestep_spacing=spacing, final_sigmas_type=final, solver_type=st,
                    solver_order=so).coefficient_table()
        assert torch.isfinite(tab).all(), (n, karras, spacing, final, st, so)
        if final == "zero":
            assert float(tab[-1, 8]) == 0.0 and float(tab[-1, 9]) == -1.0
    sd = UniPCMultistepScheduler.from_config(vdiff.DDIMScheduler().config, use_karras_sigmas=True)
    sd.set_timesteps(n)
    assert torch.isfinite(sd.coefficient_table()).all()


def test_a_non_finite_row_is_refused():
    with pytest.raises(ValueError, match="not finite"):
        unipc_row64([2.0, 1.0, 0.0], 1, 0, 2, bh2=False)                # second-order "bh1" onto sigma 0: B_h = -inf
    with pytest.raises(ValueError, match="not finite"):
        unipc_row([2.0, 1.0, 1.0, 0.5], 2, 2, 1)                        # h = 0 in a second-order corrector


# ---------------------------------------------------------------- the restatement, pinned on its order
def _toy(sigma):
    a = 1.0 / math.sqrt(sigma * sigma + 1.0)
    return a, sigma * a


def _var(sigma):
    """The variance of x at noise level sigma for data of variance 0.25: a^2 0.25 + sig^2."""
    a, s = _toy(sigma)
    return a * a * 0.25 + s * s


def _x0(x, sigma):
    """E[x0 | x] of the Gaussian toy model."""
    a, _ = _toy(sigma)
    return a * 0.25 * x / _var(sigma)


def _eps(x, sigma):
    a, s = _toy(sigma)
    return (x - a * _x0(x, sigma)) / s


def _analytic(sig):
    """The probability-flow ODE keeps x / sqrt(var) fixed: its state at s[n-1] from x_T = 1.7 at
    s[0], mapped through x0(.) — what a final sigma of 0 returns."""
    n = len(sig) - 1
    return _x0(1.7 * math.sqrt(_var(sig[n - 1]) / _var(sig[0])), sig[n - 1])


def error_through_the_restatement(n, **kw):
    ref = R.UniPCRef(dtype=F64, use_karras_sigmas=True, **kw).set_timesteps(n)
    sig = [float(v) for v in ref.sigmas]
    x = torch.tensor([1.7], dtype=F64)
    for i in range(n):
        x = ref.step(_eps(x, sig[i]), x)
        assert x.dtype == F64
    return abs(float(x) - _analytic(sig))


def error_through_the_host_rows(n, **kw):
    """The scheduler's own fp32 table, its rows applied in the kernel's order in fp64 numpy."""
    s = sched(n, use_karras_sigmas=True, **kw)
    sig = s.sigmas.tolist()
    tab = s.coefficient_table().double().numpy()
    x = np.float64(1.7)
    S0 = S1 = S2 = np.float64(np.nan)
    for i in range(n):
        r, fl = tab[i], int(tab[i, 12])
        m_t = (x - r[1] * _eps(x, sig[i])) / r[0]
        m0 = S0 if fl else m_t
        xc = x
        if fl & 1:
            res = r[7] * (m_t - m0)
            if fl & 2:
                res = r[6] * ((S1 - m0) / r[5]) + res
            xc = (r[2] * S2 - r[3] * m0) - r[4] * res
        y = r[8] * xc - r[9] * m_t
        if fl & 4:
            y = y - r[10] * (0.5 * ((m0 - m_t) / r[11]))
        x, S1, S0, S2 = y, m0, m_t, xc
    return abs(float(x) - _analytic(sig))


@pytest.mark.parametrize("solver_type", ["bh2", "bh1"])
@pytest.mark.parametrize("through", [error_through_the_restatement, error_through_the_host_rows],
                         ids=["restatement", "host_rows"])
def test_order_of_convergence(through, solver_type):
    with_c = [through(n, solver_type=solver_type) for n in (40, 80)]
    without = [through(n, solver_type=solver_type, disable_corrector=list(range(n))) for n in (40, 80)]
    print(f"UniPC {solver_type} {through.__name__}: error at n = 40, 80 with the corrector {with_c[0]:.3e} "
          f"{with_c[1]:.3e} (x {with_c[0] / with_c[1]:.2f}), without {without[0]:.3e} {without[1]:.3e} "
          f"(x {without[0] / without[1]:.2f})")
    assert with_c[1] > 0 and without[1] > 0
    assert with_c[0] / with_c[1] >= 6
    assert 3 <= without[0] / without[1] <= 6
    assert with_c[1] < without[1]                                       # and the corrector helps outright
