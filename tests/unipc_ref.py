"""Test infrastructure only.  Never imported by the product path.

Restatement of `diffusers:UniPCMultistepScheduler` (schedulers/scheduling_unipc_multistep.py) from
its source, in plain torch ops on the CPU with a dtype parameter: `convert_model_output` for epsilon
prediction, `multistep_uni_p_bh_update` (UniP) and `multistep_uni_c_bh_update` (UniC) under
predict_x0 with the "bh1" / "bh2" B(h), their `rks` / `R` / `b` construction with
`torch.linalg.solve` for the corrector's rho, and `step`'s decisions (`this_order`,
`lower_order_nums`, `last_sample`, `disable_corrector`, `lower_order_final`).  Timesteps and sigmas
are the rules diffusers' two multistep schedulers share, taken from tests/dpm_ref.py.  Parity to
diffusers itself is UNPINNED: diffusers is not installed where this runs, so nothing here was
compared against it.  tests/test_unipc_host.py pins this restatement on its order of convergence
against an analytic solution instead.

`UniPCRef(dtype, coef="ops")` evaluates every coefficient with torch ops in `dtype`, as diffusers
does (in fp32 there).  `UniPCRef(coef="rows")` takes them from `row()` below — fp64 from the fp32
sigmas, rounded once to fp32, vdiff's convention — and applies them in the device kernel's
operation order, one fp32 torch op at a time: the reference the kernel is held to bit for bit.

Two places where this follows the kernel's contract (include/vdiff.h) and not diffusers to the
letter: a first-order predictor returns x_t_ itself (diffusers subtracts alpha_t * B_h * 0, which is
NaN for "bh1" on a final sigma of 0, where B_h = -inf), and the first step of a run, which has no
earlier x0 prediction, stores its own in both history places.
"""
from __future__ import annotations

import math

import torch

from dpm_ref import alphas_cumprod, cfg_combine, schedule, sigma_to_alpha_sigma_t  # noqa: F401

ROW = 16
F_CORR, F_CORR2, F_PRED2 = 1, 2, 4


# ---------------------------------------------------------------- rows: fp64, rounded once
def _lambda(sigma):
    alpha = 1.0 / math.sqrt(sigma * sigma + 1.0)
    sig = sigma * alpha
    return alpha, sig, (math.log(alpha) - math.log(sig)) if sig > 0.0 else math.inf


def _b_vector(hh, B_h, order):
    """diffusers' b, its loop as written: h_phi_k * factorial_i / B_h for i = 1 .. order."""
    h_phi_1 = math.expm1(hh)
    h_phi_k = h_phi_1 / hh - 1
    factorial_i = 1
    b = []
    for i in range(1, order + 1):
        b.append(h_phi_k * factorial_i / B_h)
        factorial_i *= i + 1
        h_phi_k = h_phi_k / hh - 1 / factorial_i
    return b


def corrector_rhos64(rk, hh, B_h):
    """The second-order corrector's rho in fp64: linalg.solve(R, b), R = [rks ** 0, rks ** 1], rks = [rk, 1]."""
    rks = torch.tensor([rk, 1.0], dtype=torch.float64)
    R = torch.stack([torch.pow(rks, 0), torch.pow(rks, 1)])
    b = torch.tensor(_b_vector(hh, B_h, 2), dtype=torch.float64)
    return torch.linalg.solve(R, b)


def row(sigmas, i, corr_order, pred_order, bh2=True, rounded=True):
    """The 16 fp32 coefficients of the step at index i in the device table's order (include/vdiff.h);
    rounded=False: in fp64, before their one rounding."""
    sig = [float(s) for s in sigmas]
    out = [0.0] * ROW
    a_i, s_i, l_i = _lambda(sig[i])
    out[0], out[1] = a_i, s_i
    flags = 0
    if corr_order:                      # the step i-1 -> i again
        _, s_s0, l_s0 = _lambda(sig[i - 1])
        hh = -(l_i - l_s0)
        h_phi_1 = math.expm1(hh)
        B_h = h_phi_1 if bh2 else hh
        out[2], out[3], out[4] = s_i / s_s0, a_i * h_phi_1, a_i * B_h
        flags |= F_CORR
        if corr_order == 1:
            out[7] = 0.5
        else:
            rk = (_lambda(sig[i - 2])[2] - l_s0) / (l_i - l_s0)
            rhos = corrector_rhos64(rk, hh, B_h)
            out[5], out[6], out[7] = rk, float(rhos[0]), float(rhos[1])
            flags |= F_CORR2
    a_t, s_t, l_t = _lambda(sig[i + 1])  # the step i -> i+1
    h = l_t - l_i
    h_phi_1 = math.expm1(-h)
    out[8], out[9] = s_t / s_i, a_t * h_phi_1
    if pred_order == 2:
        out[10] = a_t * (h_phi_1 if bh2 else -h)
        out[11] = (_lambda(sig[i - 1])[2] - l_i) / h
        flags |= F_PRED2
    out[12] = float(flags)
    out = torch.tensor(out, dtype=torch.float64)
    return out.float() if rounded else out


def kernel_step(eps, x, S0, S1, S2, r):
    """The device kernel's update with row r, one fp32 torch op at a time ->
    (prev_sample, new S0, new S1, new S2).  S0 / S2 are read by a corrector row (S0 by a
    second-order predictor too), S1 by a second-order corrector only; a flags-0 row reads none."""
    eps, x = eps.float(), x.float()
    flags = int(r[12])
    m_t = (x - r[1] * eps) / r[0]
    m0 = S0.float() if flags else m_t
    xc = x
    if flags & F_CORR:
        x_ = r[2] * S2.float() - r[3] * m0
        d_t = m_t - m0
        res = r[7] * d_t
        if flags & F_CORR2:
            res = r[6] * ((S1.float() - m0) / r[5]) + res
        xc = x_ - r[4] * res
    y = r[8] * xc - r[9] * m_t
    if flags & F_PRED2:
        y = y - r[10] * (0.5 * ((m0 - m_t) / r[11]))
    return y, m_t, m0, xc


# ---------------------------------------------------------------- the stateful scheduler
class UniPCRef:
    def __init__(self, dtype=torch.float32, coef="ops", solver_order=2, solver_type="bh2", disable_corrector=(),
                 use_karras_sigmas=False, final_sigmas_type="zero", timestep_spacing="linspace", steps_offset=0,
                 beta_schedule="linear", beta_start=0.0001, beta_end=0.02, num_train_timesteps=1000,
                 trained_betas=None):
        assert coef in ("ops", "rows") and solver_type in ("bh1", "bh2") and solver_order in (1, 2)
        assert coef == "ops" or dtype == torch.float32
        self.dtype, self.coef = dtype, coef
        self.solver_order, self.solver_type = solver_order, solver_type
        self.disable_corrector = list(disable_corrector)
        self.karras, self.final, self.spacing, self.steps_offset = (use_karras_sigmas, final_sigmas_type,
                                                                   timestep_spacing, steps_offset)
        self.acp = alphas_cumprod(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        self.timesteps = None

    def set_timesteps(self, n, begin_index=0):
        ts, self.sigmas = schedule(n, self.acp, self.spacing, self.steps_offset, self.karras, self.final)
        self.timesteps = torch.from_numpy(ts)
        self.model_outputs = [None] * self.solver_order
        self.lower_order_nums = 0
        self.last_sample = None
        self.this_order = None
        self.step_index = begin_index   # diffusers: set_begin_index(begin_index) before the first step
        return self

    # -- diffusers' methods, torch ops in self.dtype
    def _lambdas(self, *idx):
        out = []
        for i in idx:
            a, s = sigma_to_alpha_sigma_t(self.sigmas[i].to(self.dtype))
            out.append((a, s, torch.log(a) - torch.log(s)))
        return out

    def convert_model_output(self, model_output, sample):
        (alpha_t, sigma_t, _), = self._lambdas(self.step_index)
        return (sample - sigma_t * model_output) / alpha_t

    def _rks_D1s(self, first_si, order, lambda_s0, h, m0):
        """The loop both updates share: i = 1 .. order - 1, si = first_si - i, mi = model_outputs[-(i + 1)]."""
        rks, D1s = [], []
        for i in range(1, order):
            (_, _, lambda_si), = self._lambdas(first_si - i)
            mi = self.model_outputs[-(i + 1)]
            rk = (lambda_si - lambda_s0) / h
            rks.append(rk)
            D1s.append((mi - m0) / rk)
        rks.append(torch.ones((), dtype=self.dtype))
        return torch.stack(rks), D1s

    def _R_b(self, rks, hh, B_h, order):
        R, b = [], []
        h_phi_1 = torch.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1
        factorial_i = 1
        for i in range(1, order + 1):
            R.append(torch.pow(rks, i - 1))
            b.append(h_phi_k * factorial_i / B_h)
            factorial_i *= i + 1
            h_phi_k = h_phi_k / hh - 1 / factorial_i
        return torch.stack(R), torch.stack(b)

    def multistep_uni_p_bh_update(self, sample, order):
        m0, x = self.model_outputs[-1], sample
        (alpha_t, sigma_t, lambda_t), (_, sigma_s0, lambda_s0) = self._lambdas(self.step_index + 1, self.step_index)
        h = lambda_t - lambda_s0
        _, D1s = self._rks_D1s(self.step_index, order, lambda_s0, h, m0)
        hh = -h
        h_phi_1 = torch.expm1(hh)
        B_h = hh if self.solver_type == "bh1" else torch.expm1(hh)
        x_t_ = sigma_t / sigma_s0 * x - alpha_t * h_phi_1 * m0
        if not D1s:
            return x_t_
        assert order == 2                # diffusers: "for order 2, we use a simplified version": rhos_p = [0.5]
        pred_res = 0.5 * D1s[0]
        return x_t_ - alpha_t * B_h * pred_res

    def multistep_uni_c_bh_update(self, this_model_output, last_sample, this_sample, order):
        m0, x, model_t = self.model_outputs[-1], last_sample, this_model_output
        (alpha_t, sigma_t, lambda_t), (_, sigma_s0, lambda_s0) = self._lambdas(self.step_index, self.step_index - 1)
        h = lambda_t - lambda_s0
        rks, D1s = self._rks_D1s(self.step_index - 1, order, lambda_s0, h, m0)
        hh = -h
        h_phi_1 = torch.expm1(hh)
        B_h = hh if self.solver_type == "bh1" else torch.expm1(hh)
        if order == 1:                   # diffusers: "for order 1, we use a simplified version"
            rhos_c = torch.tensor([0.5], dtype=self.dtype)
        else:
            R, b = self._R_b(rks, hh, B_h, order)
            rhos_c = torch.linalg.solve(R, b)
        x_t_ = sigma_t / sigma_s0 * x - alpha_t * h_phi_1 * m0
        corr_res = rhos_c[0] * D1s[0] if D1s else 0
        D1_t = model_t - m0
        return x_t_ - alpha_t * B_h * (corr_res + rhos_c[-1] * D1_t)

    # -- step
    def uses_corrector(self):
        return (self.step_index > 0 and self.step_index - 1 not in self.disable_corrector
                and self.last_sample is not None)

    def next_order(self):
        """lower_order_final is True: this_order as step computes it for the predictor."""
        this_order = min(self.solver_order, len(self.timesteps) - self.step_index)
        return min(this_order, self.lower_order_nums + 1)

    def step(self, model_output, sample):
        """-> prev_sample"""
        model_output, sample = model_output.to(self.dtype), sample.to(self.dtype)
        use_corrector = self.uses_corrector()
        if self.coef == "rows":
            r = row(self.sigmas, self.step_index, self.this_order if use_corrector else 0, self.next_order(),
                    self.solver_type == "bh2")
            older = self.model_outputs[-2] if self.solver_order == 2 else None
            prev, m_t, m0, xc = kernel_step(model_output, sample, self.model_outputs[-1], older, self.last_sample, r)
            self.model_outputs = [m0, m_t][-self.solver_order:]
            self.this_order = self.next_order()
            self.last_sample = xc
        else:
            model_output_convert = self.convert_model_output(model_output, sample)
            if use_corrector:
                sample = self.multistep_uni_c_bh_update(model_output_convert, self.last_sample, sample, self.this_order)
            for i in range(self.solver_order - 1):
                self.model_outputs[i] = self.model_outputs[i + 1]
            self.model_outputs[-1] = model_output_convert
            self.this_order = self.next_order()
            assert self.this_order > 0
            self.last_sample = sample
            prev = self.multistep_uni_p_bh_update(sample, self.this_order)
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return prev

    def decisions(self, start=0):
        """[(corrector order or 0, predictor order)] of a run from schedule position `start` with a
        fresh state: this restatement's own step logic, replayed without data."""
        keep = (self.lower_order_nums, self.last_sample, self.this_order, self.step_index)
        self.lower_order_nums, self.last_sample, self.this_order, self.step_index = 0, None, None, start
        out = []
        for _ in range(start, len(self.timesteps)):
            corr = self.this_order if self.uses_corrector() else 0
            self.this_order = self.next_order()
            out.append((corr, self.this_order))
            self.last_sample = True
            self.lower_order_nums = min(self.lower_order_nums + 1, self.solver_order)
            self.step_index += 1
        self.lower_order_nums, self.last_sample, self.this_order, self.step_index = keep
        return out

    def table(self, start=0):
        bh2 = self.solver_type == "bh2"
        return torch.stack([row(self.sigmas, start + j, c, p, bh2) for j, (c, p) in enumerate(self.decisions(start))])
