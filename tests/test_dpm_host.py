"""DPMSolverMultistepScheduler on the CPU: config and refusals, the entry point's argument checks
before any launch, timesteps / sigmas / coefficient rows against the restatement of diffusers'
scheduler (tests/dpm_ref.py, unpinned), and the restatement itself against an analytic invariant.

Bars (none taken from a device):
  * tables: equality.
  * the analytic invariant (a point-mass data distribution, see test_point_mass_invariant): rel-L2
    1e-12 in fp64 and 1.2e-6 in fp32, with the SD-1.5 betas the pipelines here run (scaled_linear
    0.00085 .. 0.012, sigma_max 14.6).  Measured on the CPU: 5.4e-16 and 3.6e-7 (the fp32 bar was
    set at 4 x an earlier measurement of 3.0e-7, which covers libm differences).  With the scheduler's own
    default betas (linear 1e-4 .. 0.02) sigma_max is 157 and the x0 conversion's cancellation
    amplifies fp32 rounding by 1 / alpha = 157 (measured 2.8e-6), so that config is held to the
    fp64 bar alone (measured 5.8e-15).
  * the second-order term: fp64 against a closed form, 1e-12 (about ten roundings of 1.1e-16
    each and a cancellation of at most 100 in x(order 2) - x(order 1)); the rows' c_d1 * (1/r0)
    against it within three fp32 roundings (3 * 2^-24).
  * fp64-rounded rows against fp32-torch-op rows: 8 x the gap measured on the CPU (GAP below) —
    a consistency bound between two host restatements, never a device value.
"""
import ctypes
import itertools
import math

import pytest
import torch

import dpm_ref as R
import vdiff
import vdiff._lib as L
from vdiff import DPMSolverMultistepScheduler, DPMSolverMultistepSchedulerOutput, ops

F32, F64 = torch.float32, torch.float64
SD = dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012)   # DDIMScheduler().config's betas
TYPES = ["dpmsolver++", "sde-dpmsolver++"]
SPACINGS = ["linspace", "leading", "trailing"]
FINALS = ["zero", "sigma_min"]


def sched(n=None, **kw):
    s = DPMSolverMultistepScheduler.from_config(vdiff.DDIMScheduler().config, **kw)
    if n is not None:
        s.set_timesteps(n)
    return s


def ref_for(s, **kw):
    c = s.config
    return R.DPMRef(solver_order=c.solver_order, algorithm_type=c.algorithm_type, lower_order_final=c.lower_order_final,
                    euler_at_final=c.euler_at_final, use_karras_sigmas=c.use_karras_sigmas,
                    final_sigmas_type=c.final_sigmas_type, timestep_spacing=c.timestep_spacing,
                    steps_offset=c.steps_offset, beta_schedule=c.beta_schedule, beta_start=c.beta_start,
                    beta_end=c.beta_end, trained_betas=c.trained_betas, **kw)


# ---------------------------------------------------------------- config and wiring
def test_surface_and_defaults():
    s = DPMSolverMultistepScheduler()
    assert (s.kind, s.order, s.init_noise_sigma) == ("dpm", 1, 1.0)
    want = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                euler_at_final=False, use_karras_sigmas=False, use_lu_lambdas=False, final_sigmas_type="zero",
                lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0,
                rescale_betas_zero_snr=False)
    assert dict(s.config) == want
    s2 = DPMSolverMultistepScheduler.from_config(vdiff.DDIMScheduler().config, use_karras_sigmas=True)
    assert (s2.config.beta_schedule, s2.config.beta_start, s2.config.steps_offset) == ("scaled_linear", 0.00085, 1)
    assert s2.config.use_karras_sigmas and s2.config.solver_order == 2 and not s2.sde
    assert torch.equal(s2.alphas_cumprod, vdiff.DDIMScheduler().alphas_cumprod)
    assert L.VD_STEP_DPM == ops.STEP_DPM == 0x400 and ops.DPM_ROW == 8
    assert ops.SCHED_STEP["dpm"] is ops.dpm_cfg_step
    assert ops.dpm_buffer_numel(3, 10, True) == 3 * 18 and ops.dpm_buffer_numel(3, 10, False) == 24
    assert vdiff.sched.DPMSolverMultistepScheduler is DPMSolverMultistepScheduler
    assert DPMSolverMultistepSchedulerOutput._fields == ("prev_sample",)
    x = torch.randn(2, 3)
    assert s.scale_model_input(x, 5) is x
    assert len(s) == 1000


@pytest.mark.parametrize("kw, name", [
    (dict(solver_order=3), "solver_order=3"),
    (dict(algorithm_type="dpmsolver"), "dpmsolver"),
    (dict(algorithm_type="sde-dpmsolver"), "sde-dpmsolver"),
    (dict(solver_type="heun"), "heun"),
    (dict(thresholding=True), "thresholding"),
    (dict(use_lu_lambdas=True), "use_lu_lambdas"),
    (dict(lambda_min_clipped=-5.1), "lambda_min_clipped"),
    (dict(variance_type="learned_range"), "variance_type"),
    (dict(prediction_type="v_prediction"), "prediction_type"),
    (dict(prediction_type="sample"), "prediction_type"),
    (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"),
])
def test_refusals_raise_by_name(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        DPMSolverMultistepScheduler(**kw)


def test_step_refuses_cpu_tensors_and_a_missing_schedule():
    s = DPMSolverMultistepScheduler()
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
    """VD_STEP_DPM rides on ncfg: the low byte stays 1 or 2, it does not combine with VD_STEP_LCM
    or 0x200, x0_out is required and is not the latents, coef is 16-byte aligned, and
    vd_euler_cfg_step refuses the flag.  Host pointers: every call returns before a launch.  Each
    call differs from a valid one in the argument named alone (the valid one runs in
    tests/test_gpu_dpm.py)."""
    h = L.lib()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 15) & ~15
    hist = p + 4096

    def args(ncfg, coef=p, x0=hist):
        return (p, 8, ncfg, 1.0, p + 2048, 1, 4, 1, 2, 2, coef, 1, None, x0, None, 0, None)
    assert h.vd_ddim_cfg_step(*args(1 | 0x400 | 0x100)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(2 | 0x400 | 0x200)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(0x400)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(3 | 0x400)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(1 | 0x400 | 0x800)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(1 | 0x400, x0=None)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(2 | 0x400, x0=p + 2048)) == L.VD_EINVAL      # x0_out == latents
    assert h.vd_ddim_cfg_step(*args(1 | 0x400, coef=p + 4)) == L.VD_EINVAL
    assert h.vd_euler_cfg_step(*args(1 | 0x400)) == L.VD_EINVAL
    assert h.vd_euler_cfg_step(*args(2 | 0x400)) == L.VD_EINVAL
    assert h.vd_version() == 6


def test_ops_dpm_cfg_step_checks_its_operands():
    lat = torch.zeros(1, 1, 1, 1, 4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.dpm_cfg_step(torch.zeros(4, 1), 1, 1.0, lat, torch.zeros(1, 8), x0_out=torch.zeros(4))


# ---------------------------------------------------------------- tables
@pytest.mark.parametrize("alg", TYPES)
@pytest.mark.parametrize("n", [1, 4, 16, 25])
def test_schedule_and_rows_equal_the_restatement(n, alg):
    for karras, spacing, final in itertools.product([False, True], SPACINGS, FINALS):
        s = sched(n, algorithm_type=alg, use_karras_sigmas=karras, timestep_spacing=spacing, final_sigmas_type=final)
        ref = ref_for(s, coef="rows").set_timesteps(n)
        case = (n, alg, karras, spacing, final)
        assert s.timesteps.dtype == torch.int64 and s.num_inference_steps == n
        assert torch.equal(s.timesteps, ref.timesteps), case
        assert s.sigmas.dtype == F32 and s.sigmas.shape == (n + 1,)
        assert torch.equal(s.sigmas.view(torch.int32), ref.sigmas.view(torch.int32)), case
        if karras:
            assert len(set(s.timesteps.tolist())) == n, case
        tab = s.coefficient_table()
        assert tab.shape == (n, 8) and tab.dtype == F32
        assert torch.equal(tab, ref.table()), case
        assert torch.isfinite(tab).all(), case
        sde = alg.startswith("sde")
        for i in range(n):
            r = tab[i]
            assert torch.equal(s.coefficients(i), r)
            flags = int(r[7])
            assert float(r[7]) == flags and flags & 2 == 2 * sde
            assert flags & 1 == (0 if i == 0 else flags & 1)                   # row 0 is first order
            if not flags & 1:
                assert r[4] == 0 and r[5] == 0, case
            if not sde:
                assert r[6] == 0, case
        if final == "zero":
            assert tab[-1, 2:].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 2.0 * sde], case
        # every middle row of a second-order schedule is second order
        assert all(int(tab[i, 7]) & 1 for i in range(1, n - 1)), case


def test_solver_order_one_has_first_order_rows_only():
    s = sched(6, solver_order=1)
    tab = s.coefficient_table()
    assert tab[:, 7].tolist() == [0.0] * 6 and tab[:, 4:7].abs().max() == 0
    assert torch.equal(tab, ref_for(s).set_timesteps(6).table())


def test_trained_betas_and_linear_schedule():
    betas = torch.linspace(1e-4, 2e-2, 100).tolist()
    s = DPMSolverMultistepScheduler(trained_betas=betas, num_train_timesteps=100)
    s.set_timesteps(5)
    ref = ref_for(s).set_timesteps(5)
    assert torch.equal(s.timesteps, ref.timesteps) and torch.equal(s.sigmas, ref.sigmas)
    assert torch.equal(s.coefficient_table(), ref.table())
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(7)
    assert torch.equal(s.coefficient_table(), ref_for(s).set_timesteps(7).table())


def test_a_sliced_schedule_starts_first_order():
    for alg in TYPES:
        s = sched(6, algorithm_type=alg, use_karras_sigmas=True)
        full = s.coefficient_table()
        s.set_begin_index(2)
        cut = s.coefficient_table(s.timesteps[2:])
        assert cut.shape == (4, 8)
        assert int(cut[0, 7]) & 1 == 0 and int(full[2, 7]) & 1 == 1
        assert torch.equal(cut[0, :4], full[2, :4]) and cut[0, 4] == 0 and cut[0, 5] == 0
        assert torch.equal(cut[1:], full[3:])
        assert torch.equal(cut, ref_for(s).set_timesteps(6).table(start=2))
        s.set_begin_index(None)
        assert torch.equal(s.coefficient_table(s.timesteps[2:]), cut)   # found by position without begin_index


def test_last_step_order_of_a_16_step_sigma_min_schedule():
    s = sched(16, final_sigmas_type="sigma_min")
    assert int(s.coefficient_table()[-1, 7]) & 1 == 1                   # 16 >= 15: lower_order_final does not apply
    s = sched(16, final_sigmas_type="sigma_min", euler_at_final=True)
    assert int(s.coefficient_table()[-1, 7]) & 1 == 0
    s = sched(14, final_sigmas_type="sigma_min")
    assert int(s.coefficient_table()[-1, 7]) & 1 == 0                   # 14 < 15
    s = sched(14, final_sigmas_type="sigma_min", lower_order_final=False)
    assert int(s.coefficient_table()[-1, 7]) & 1 == 1
    s = sched(16)                                                       # "zero": always first order
    assert int(s.coefficient_table()[-1, 7]) & 1 == 0


def test_index_for_timestep_and_add_noise():
    s = sched(5)
    ts = s.timesteps.tolist()
    assert [s.index_for_timestep(t) for t in ts] == list(range(5))
    assert s.index_for_timestep(12345) == 4                             # diffusers' fall-back: the last index
    assert s.index_for_timestep(7, torch.tensor([9, 7, 7, 3])) == 2     # the second match
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


# ---------------------------------------------------------------- the restatement, pinned analytically
def point_mass_errors(ref, n, use_rows=False):
    """A point-mass data distribution at x0*: the exact eps of x is (x - alpha x0*) / sigma.  The
    deterministic solver is exact on it, x_i = alpha_i x0* + sigma_i e*; the SDE solver with zero
    noise keeps x_i = alpha_i x0* + sigma_i exp(-(lambda_i - lambda_0)) e*; a final sigma of 0
    returns x0*.  -> the worst rel-L2 over the steps, against fp64 closed forms."""
    ref.set_timesteps(n)
    dtype = ref.dtype
    g = torch.Generator().manual_seed(n)
    x0s, es = torch.randn(64, generator=g, dtype=F64), torch.randn(64, generator=g, dtype=F64)
    sig = ref.sigmas.double()
    al = 1 / (sig ** 2 + 1).sqrt()
    st = sig * al
    lam = torch.log(al) - torch.log(st)

    def expect(i):
        decay = torch.exp(-(lam[i] - lam[0])) if ref.sde else 1.0
        return al[i] * x0s + st[i] * decay * es
    x = expect(0).to(dtype)
    worst = 0.0
    for i in range(n):
        if use_rows:   # the alpha / sigma the step itself divides by
            r = R.row(ref.sigmas, i, False, ref.sde)
            a, s = r[0], r[1]
        else:
            a, s = R.sigma_to_alpha_sigma_t(ref.sigmas[i].to(dtype))
        eps = (x - a * x0s.to(dtype)) / s
        x = ref.step(eps, x, noise=torch.zeros(64, dtype=dtype) if ref.sde else None)
        assert x.dtype == dtype
        w = expect(i + 1)
        worst = max(worst, ((x.double() - w).norm() / w.norm()).item())
    if ref.final == "zero":
        assert ((x.double() - x0s).norm() / x0s.norm()).item() <= (1e-12 if dtype == F64 else 1.2e-6)
    return worst


CASES = list(itertools.product([4, 5, 16, 25], TYPES, [False, True], FINALS))


def test_point_mass_invariant():
    worst = {}
    for name, dtype, coef, betas, rows in [("fp64", F64, "ops", SD, False), ("fp32", F32, "ops", SD, False),
                                           ("fp32 rows", F32, "rows", SD, True), ("fp64 default betas", F64, "ops", {}, False)]:
        worst[name] = max(point_mass_errors(R.DPMRef(dtype=dtype, coef=coef, algorithm_type=alg, use_karras_sigmas=k,
                                                     final_sigmas_type=f, **betas), n, rows)
                          for n, alg, k, f in CASES)
    print("DPM point-mass invariant, worst rel-L2:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["fp64"] <= 1e-12 and worst["fp64 default betas"] <= 1e-12
    assert worst["fp32"] <= 1.2e-6
    assert worst["fp32 rows"] <= 1.2e-6


@pytest.mark.parametrize("alg", TYPES)
def test_second_order_term(alg):
    """The invariant never exercises D1 (m0 == m1 there).  With m0 - m1 = d constant:
    x(order 2) - x(order 1) = c_d1 * (1/r0) * d, c_d1 * (1/r0) written out here from the sigmas."""
    ref = R.DPMRef(dtype=F64, algorithm_type=alg, use_karras_sigmas=True, **SD).set_timesteps(8)
    d = 0.37
    g = torch.Generator().manual_seed(1)
    x, m0 = torch.randn(32, generator=g, dtype=F64), torch.randn(32, generator=g, dtype=F64)
    nz = torch.randn(32, generator=g, dtype=F64)
    for i in (1, 4, 6):
        ref.step_index = i
        one = ref.first_order_update(m0, x, nz)
        two = ref.second_order_update([m0 - d, m0], x, nz)
        lam = []
        for s in (float(ref.sigmas[i - 1]), float(ref.sigmas[i]), float(ref.sigmas[i + 1])):
            a = 1 / math.sqrt(s * s + 1)
            lam.append(math.log(a) - math.log(s * a))
        h, h_0 = lam[2] - lam[1], lam[1] - lam[0]
        a_t = 1 / math.sqrt(float(ref.sigmas[i + 1]) ** 2 + 1)
        half = 0.5 * a_t * (1 - math.exp(-2 * h)) if ref.sde else -0.5 * a_t * (math.exp(-h) - 1)
        want = half * (h / h_0) * d
        assert want > 1e-3
        assert ((two - one) - want).abs().max().item() <= 1e-12 * max(1.0, x.abs().max().item())
        r = R.row(ref.sigmas, i, True, ref.sde)
        assert abs(float(r[4]) * float(r[5]) - half * (h / h_0)) <= 3 * 2.0 ** -24 * abs(half * (h / h_0))
        # the kernel's operation order, in fp32: the same eps through a second- and a first-order
        # row differs by c_d1 * ((1/r0) * d) up to the roundings of two sums of size |x|
        r1 = R.row(ref.sigmas, i, False, ref.sde)
        eps = torch.randn(32, generator=g)
        lo, x0 = R.kernel_step(eps, x.float(), None, r1, nz.float())
        hi, x0b = R.kernel_step(eps, x.float(), x0 - torch.tensor(d), r, nz.float())
        assert torch.equal(x0, x0b)
        tol = 4 * 2.0 ** -24 * max(hi.abs().max().item(), x0.abs().max().item() * float(r[5]))
        assert ((hi - lo).double() - want).abs().max().item() <= tol


# measured on the CPU with the SD-1.5 betas, both algorithm types, Karras on and off, both final
# sigma types: max |rounded - torch-op| / |rounded| per slot {alpha_s, sigma_s, c_x, c_m0, c_d1, 1/r0, c_noise}
GAP = {4: [6.53e-08, 7.30e-08, 2.09e-07, 7.60e-08, 7.60e-08, 1.64e-07, 7.38e-08],
       25: [1.13e-07, 1.17e-07, 3.20e-07, 8.02e-07, 8.02e-07, 1.64e-06, 4.48e-07],
       50: [1.21e-07, 1.18e-07, 5.98e-07, 2.86e-06, 2.86e-06, 5.06e-06, 1.39e-06]}


@pytest.mark.parametrize("n", [4, 25, 50])
def test_rounded_rows_against_fp32_torch_op_rows(n):
    gap = [0.0] * 7
    for alg, karras, final in itertools.product(TYPES, [False, True], FINALS):
        ref = R.DPMRef(algorithm_type=alg, use_karras_sigmas=karras, final_sigmas_type=final, **SD).set_timesteps(n)
        tab = ref.table()
        for i in range(n):
            o = R.row_torch_ops(ref.sigmas, i, bool(int(tab[i, 7]) & 1), ref.sde)
            assert o[7] == tab[i, 7]
            for j in range(7):
                if tab[i, j] == 0:
                    assert o[j] == 0, (alg, karras, final, i, j, o[j].item())
                else:
                    gap[j] = max(gap[j], abs((o[j].double() - tab[i, j].double()) / tab[i, j].double()).item())
    print(f"DPM rows, n = {n}: max relative gap per slot", [f"{g:.2e}" for g in gap])
    for j in range(7):
        assert gap[j] <= 8 * GAP[n][j], (j, gap[j], GAP[n][j])
