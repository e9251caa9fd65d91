"""DPMSolverMultistepScheduler — drop-in for diffusers:DPMSolverMultistepScheduler as AnimateDiff
is usually run with it (DPM-Solver++ 2M, often with Karras sigmas, 20-25 steps):
`DPMSolverMultistepScheduler.from_config(pipe.scheduler.config, algorithm_type="dpmsolver++",
use_karras_sigmas=True)`.

Supported: solver_order 1 and 2, algorithm_type "dpmsolver++" and "sde-dpmsolver++", the midpoint
solver, lower_order_final / euler_at_final, final_sigmas_type "zero" and "sigma_min", Karras
sigmas, the three timestep spacings, steps_offset.  Everything else of diffusers' config is
refused by name.

Host side (numpy/torch-CPU, once per video): beta/alpha tables, diffusers' timestep and sigma
rules, and one coefficient row per step.  Device side: `step()` runs the fused HIP kernel
(vd_ddim_cfg_step with VD_STEP_DPM, ops.dpm_cfg_step); the pipeline's captured graph reads the
same rows by a device step counter.

It is a multistep scheduler: a second-order step reads the previous step's x0 prediction,
  x0 = (x - sigma_s eps) / alpha_s
  x <- c_x x + c_m0 x0 [+ c_d1 (1/r0) (x0 - x0_prev)] [+ c_noise noise]
The kernel keeps that history in its x0_out operand (in and out); which steps are second order
is decided here, per row, by diffusers' `lower_order_nums` / `lower_order_final` logic.

Rows go by POSITION in the current schedule, not by timestep value: row j of
`coefficient_table(ts)` uses sigmas[pos + j - 1 .. pos + j + 1], pos being where ts starts in
the schedule, and row 0 is first order — what diffusers' step does when a pipeline runs a slice
of the schedule (video-to-video) from a fresh `lower_order_nums`.

Coefficients are computed in fp64 from the fp32 sigmas and rounded once (the project's
host-independent convention, as `sqrt32`); diffusers computes them in fp32 torch ops.  Parity
to diffusers is UNPINNED (diffusers is not installed where this is tested); tests/dpm_ref.py
restates diffusers' scheduler in plain torch and the kernel is held to it bit for bit.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from .. import ops
from .ddim import _Cfg, sqrt32

DPMSolverMultistepSchedulerOutput = namedtuple("DPMSolverMultistepSchedulerOutput", ["prev_sample"])

# diffusers' DPMSolverMultistepScheduler.__init__ defaults
DEFAULT_CONFIG = dict(
    num_train_timesteps=1000,
    beta_start=0.0001,
    beta_end=0.02,
    beta_schedule="linear",
    trained_betas=None,
    solver_order=2,
    prediction_type="epsilon",
    thresholding=False,
    dynamic_thresholding_ratio=0.995,
    sample_max_value=1.0,
    algorithm_type="dpmsolver++",
    solver_type="midpoint",
    lower_order_final=True,
    euler_at_final=False,
    use_karras_sigmas=False,
    use_lu_lambdas=False,
    final_sigmas_type="zero",
    lambda_min_clipped=-float("inf"),
    variance_type=None,
    timestep_spacing="linspace",
    steps_offset=0,
    rescale_betas_zero_snr=False,
)

FLAG_SECOND, FLAG_SDE = 1, 2  # row slot 7 (include/vdiff.h)


def alpha_sigma(sigma):
    """diffusers' _sigma_to_alpha_sigma_t in fp64: alpha = 1 / sqrt(sigma^2 + 1), sigma_t = sigma alpha."""
    sigma = np.float64(sigma)
    alpha = 1.0 / np.sqrt(sigma * sigma + 1.0)
    return alpha, sigma * alpha


def dpm_row(sigma_prev, sigma_s, sigma_t, second: bool, sde: bool) -> torch.Tensor:
    """One fp32 row {alpha_s, sigma_s, c_x, c_m0, c_d1, 1/r0, c_noise, flags} of the step from
    sigma_s to sigma_t (sigma_prev: the step before, read for a second-order row only), in fp64
    from the fp32 sigmas and rounded once.  The deterministic type's c_m0 and c_d1 are the
    negated coefficients of diffusers' two subtracted terms.  sigma_t = 0 gives h = +inf:
    exp(-h) = 0, so c_x = 0 and c_m0 = 1 (alpha_t = 1), all finite."""
    # log and exp through Python's math (the C library's), not numpy's vectorised ones, whose last
    # bit depends on the host's instruction set
    lam = lambda a, s: math.log(a) - math.log(s) if s > 0.0 else math.inf  # noqa: E731
    a_t, s_t = map(float, alpha_sigma(sigma_t))
    a_s, s_s = map(float, alpha_sigma(sigma_s))
    lam_s = lam(a_s, s_s)
    h = lam(a_t, s_t) - lam_s
    if sde:
        e2 = 1.0 - math.exp(-2.0 * h)
        c_x = s_t / s_s * math.exp(-h)
        c_m0 = a_t * e2
        c_noise = s_t * math.sqrt(e2)
    else:
        c_x = s_t / s_s
        c_m0 = -(a_t * (math.exp(-h) - 1.0))
        c_noise = 0.0
    c_d1 = inv_r0 = 0.0
    if second:
        a_p, s_p = map(float, alpha_sigma(sigma_prev))
        h_0 = lam_s - lam(a_p, s_p)
        # h = 0 (a Karras ramp that ends on the final sigma_min): diffusers' r0 = h_0 / 0 = inf, 1 / r0 = 0
        inv_r0 = 1.0 / (h_0 / h) if h != 0.0 else 0.0
        c_d1 = 0.5 * c_m0
    flags = FLAG_SECOND * bool(second) + FLAG_SDE * bool(sde)
    row = torch.tensor([a_s, s_s, c_x, c_m0, c_d1, inv_r0, c_noise, float(flags)], dtype=torch.float64)
    if not torch.isfinite(row).all():
        raise ValueError(f"DPM-Solver row from sigmas ({sigma_prev}, {sigma_s}, {sigma_t}) is not finite: {row.tolist()}")
    return row.float()


def build_schedule(config, train_sigmas, num_inference_steps):
    """diffusers' set_timesteps, which DPMSolverMultistepScheduler and UniPCMultistepScheduler share:
    n + 1 points for "linspace" and "leading" with the last dropped, n for "trailing"; the sigmas of
    those timesteps (or Karras' ramp, whose timesteps are the rounded _sigma_to_t), and the final
    sigma appended -> (n timesteps, n + 1 fp32 sigmas)."""
    T = config.num_train_timesteps
    n = int(num_inference_steps)
    if n < 1 or n > T:
        raise ValueError(f"num_inference_steps {num_inference_steps}: 1..{T}")
    sp = config.timestep_spacing
    if sp == "linspace":
        ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
    elif sp == "leading":
        ratio = T // (n + 1)
        ts = (np.arange(0, n + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64)
        ts += config.steps_offset
    else:  # trailing
        ts = np.arange(T, 0, -(T / n)).round().copy().astype(np.int64)
        ts -= 1
    sigmas = train_sigmas.numpy()
    if config.use_karras_sigmas:
        log_sigmas = np.log(sigmas)
        sigmas = DPMSolverMultistepScheduler._convert_to_karras(np.flip(sigmas).copy(), n)
        ts = np.array([DPMSolverMultistepScheduler._sigma_to_t(s, log_sigmas) for s in sigmas]).round()
    else:
        sigmas = np.interp(ts, np.arange(0, len(sigmas)), sigmas)
    last = float(train_sigmas[0]) if config.final_sigmas_type == "sigma_min" else 0.0
    return ts, torch.from_numpy(np.concatenate([sigmas, [last]]).astype(np.float32))


class DPMSolverMultistepScheduler:
    kind = "dpm"  # selects the fused device update (ops.SCHED_STEP)
    order = 1     # diffusers' scheduler.order: one model call per step
    init_noise_sigma = 1.0

    def __init__(self, **kwargs):
        cfg = dict(DEFAULT_CONFIG)
        cfg.update({k: v for k, v in kwargs.items() if k in cfg})
        self.config = _Cfg(cfg)
        n = cfg["num_train_timesteps"]
        if cfg["trained_betas"] is not None:
            betas = torch.tensor(cfg["trained_betas"], dtype=torch.float32)
        elif cfg["beta_schedule"] == "linear":
            betas = torch.linspace(cfg["beta_start"], cfg["beta_end"], n, dtype=torch.float32)
        elif cfg["beta_schedule"] == "scaled_linear":
            betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, n, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"beta_schedule {cfg['beta_schedule']!r}")
        if cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("rescale_betas_zero_snr")
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError(f"prediction_type {cfg['prediction_type']!r}: only epsilon prediction")
        if cfg["thresholding"]:
            raise NotImplementedError("thresholding")
        if cfg["solver_order"] == 3:
            raise NotImplementedError("solver_order=3 (the third-order update, meant for unconditional sampling)")
        if cfg["solver_order"] not in (1, 2):
            raise ValueError(f"solver_order {cfg['solver_order']!r}: 1 or 2")
        if cfg["algorithm_type"] in ("dpmsolver", "sde-dpmsolver"):
            raise NotImplementedError(f"algorithm_type {cfg['algorithm_type']!r}: only 'dpmsolver++' and "
                                      "'sde-dpmsolver++'")
        if cfg["algorithm_type"] not in ("dpmsolver++", "sde-dpmsolver++"):
            raise ValueError(f"algorithm_type {cfg['algorithm_type']!r}")
        if cfg["solver_type"] == "heun":
            raise NotImplementedError("solver_type 'heun': only 'midpoint'")
        if cfg["solver_type"] != "midpoint":
            raise ValueError(f"solver_type {cfg['solver_type']!r}")
        if cfg["use_lu_lambdas"]:
            raise NotImplementedError("use_lu_lambdas")
        if cfg["lambda_min_clipped"] is not None and math.isfinite(cfg["lambda_min_clipped"]):
            raise NotImplementedError("lambda_min_clipped: only -inf (no clipping of the schedule's end)")
        if cfg["variance_type"] is not None:
            raise NotImplementedError("variance_type (a model that predicts its variance)")
        if cfg["final_sigmas_type"] not in ("zero", "sigma_min"):
            raise ValueError(f"final_sigmas_type {cfg['final_sigmas_type']!r}: 'zero' or 'sigma_min'")
        if cfg["timestep_spacing"] not in ("linspace", "leading", "trailing"):
            raise ValueError(f"timestep_spacing {cfg['timestep_spacing']!r}")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        # sigma of every training timestep, correctly rounded (diffusers: ((1 - a) / a) ** 0.5)
        self.train_sigmas = sqrt32((1 - self.alphas_cumprod) / self.alphas_cumprod)
        self.sigmas = self.train_sigmas
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, n)[::-1].copy().astype(np.int64))
        self.model_outputs = [None] * cfg["solver_order"]
        self.lower_order_nums = 0
        self._step_index = None
        self._begin_index = None

    @classmethod
    def from_config(cls, config, **kwargs):
        base = dict(config) if config is not None else {}
        base.update(kwargs)
        return cls(**base)

    @property
    def sde(self) -> bool:
        return self.config.algorithm_type == "sde-dpmsolver++"

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    # ------------------------------------------------------------------ the schedule
    @staticmethod
    def _convert_to_karras(in_sigmas, num_inference_steps):
        """diffusers' _convert_to_karras (rho 7) over sigma_max = in_sigmas[0] .. sigma_min = in_sigmas[-1]."""
        sigma_min, sigma_max = in_sigmas[-1].item(), in_sigmas[0].item()
        rho = 7.0
        ramp = np.linspace(0, 1, num_inference_steps)
        min_inv_rho, max_inv_rho = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
        return (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** rho

    @staticmethod
    def _sigma_to_t(sigma, log_sigmas):
        """diffusers' _sigma_to_t: the (fractional) training timestep whose log sigma interpolates to sigma's."""
        log_sigma = np.log(np.maximum(sigma, 1e-10))
        dists = log_sigma - log_sigmas[:, np.newaxis]
        low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
        high_idx = low_idx + 1
        low, high = log_sigmas[low_idx], log_sigmas[high_idx]
        w = np.clip((low - log_sigma) / (low - high), 0, 1)
        t = (1 - w) * low_idx + w * high_idx
        return t.reshape(sigma.shape)

    def set_timesteps(self, num_inference_steps: int, device=None):
        """diffusers' set_timesteps (build_schedule above): n timesteps, n + 1 fp32 sigmas."""
        ts, self.sigmas = build_schedule(self.config, self.train_sigmas, num_inference_steps)
        self.timesteps = torch.from_numpy(np.asarray(ts).astype(np.int64)).to(device)
        self.num_inference_steps = len(ts)
        self.model_outputs = [None] * self.config.solver_order
        self.lower_order_nums = 0
        self._step_index = None
        self._begin_index = None

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        """diffusers': the second match (an image-to-image restart never lands on a repeated first
        one), the only match, or — for a timestep the schedule does not hold — the last index."""
        st = self.timesteps if schedule_timesteps is None else schedule_timesteps
        idx = (torch.as_tensor(st).cpu() == int(timestep)).nonzero()
        if len(idx) == 0:
            return len(self.timesteps) - 1
        return int(idx[1 if len(idx) > 1 else 0])

    def _init_step_index(self, timestep):
        self._step_index = self.index_for_timestep(timestep) if self._begin_index is None else self._begin_index

    def scale_model_input(self, sample, timestep=None):
        return sample

    # ------------------------------------------------------------------ rows
    def _first_order_at(self, idx: int, fresh: bool) -> bool:
        """diffusers' step order logic at schedule index idx; fresh: no earlier x0 is held
        (lower_order_nums < 1)."""
        n = len(self.timesteps)
        c = self.config
        final = idx == n - 1 and (c.euler_at_final or (c.lower_order_final and n < 15) or
                                  c.final_sigmas_type == "zero")
        return c.solver_order == 1 or fresh or final

    def _row_at(self, idx: int, second: bool) -> torch.Tensor:
        s = self.sigmas
        return dpm_row(float(s[idx - 1]) if second else 0.0, float(s[idx]), float(s[idx + 1]), second, self.sde)

    def _position(self, ts) -> int:
        """Where the timesteps `ts` start in the current schedule: begin_index when it fits, else
        the first position at which the schedule continues as ts does."""
        full, ts = self.timesteps.cpu().tolist(), [int(t) for t in ts]
        n = len(ts)
        fits = lambda p: full[p:p + n] == ts  # noqa: E731
        if self._begin_index is not None and fits(self._begin_index):
            return self._begin_index
        for p in range(len(full) - n + 1):
            if fits(p):
                return p
        raise ValueError(f"timesteps {ts[:4]}{'...' if n > 4 else ''} are no run of the current schedule "
                         f"({len(full)} steps): call set_timesteps() with the schedule they come from")

    def coefficients(self, i: int) -> torch.Tensor:
        """The fp32 row of step index i of the current schedule (module docstring, include/vdiff.h)."""
        return self.coefficient_table(self.timesteps)[i]

    def coefficient_table(self, timesteps=None) -> torch.Tensor:
        """[n, 8] rows for a run of the current schedule (default: all of it).  Row 0 is first
        order; a later row is second order unless solver_order is 1 or diffusers' lower_order_final
        rule makes the schedule's last step first order."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        ts = (self.timesteps if timesteps is None else torch.as_tensor(timesteps)).cpu().tolist()
        pos = self._position(ts)
        return torch.stack([self._row_at(pos + j, not self._first_order_at(pos + j, fresh=j == 0))
                            for j in range(len(ts))])

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' add_noise: alpha x + sigma noise at the timesteps' schedule indices (begin_index
        / step_index when set, as diffusers), alpha and sigma from the fp32 schedule sigma in fp64,
        rounded once."""
        t = torch.as_tensor(timesteps).reshape(-1).cpu().tolist()
        if self._begin_index is None:
            idx = [self.index_for_timestep(v) for v in t]
        elif self._step_index is not None:
            idx = [self._step_index] * len(t)
        else:
            idx = [self._begin_index] * len(t)
        a, s = alpha_sigma(self.sigmas[idx].double().numpy())
        x = original_samples.float()
        shape = (-1,) + (1,) * (x.dim() - 1)
        a = torch.from_numpy(np.asarray(a)).float().to(x.device).reshape(shape)
        s = torch.from_numpy(np.asarray(s)).float().to(x.device).reshape(shape)
        return a * x + s * noise.to(x.device, torch.float32)

    # ------------------------------------------------------------------ step
    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict: bool = True):
        """diffusers' step on the HIP kernel with a one-row buffer.  `model_outputs` holds the x0
        predictions (the last solver_order of them) and `lower_order_nums` counts up as in
        diffusers.  The SDE type draws one randn_tensor(model_output.shape, generator, device,
        dtype=torch.float32) per call, on every step, unless variance_noise is given."""
        from ..pipeline import randn_tensor
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        if not (model_output.is_cuda and sample.is_cuda):
            raise ValueError("DPMSolverMultistepScheduler.step runs the HIP kernel; tensors must be on the GPU")
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        if i >= len(self.timesteps):
            raise ValueError(f"step {i} of a {len(self.timesteps)}-step schedule: call set_timesteps() to start over")
        second = not self._first_order_at(i, fresh=self.lower_order_nums < 1)
        row = self._row_at(i, second)
        numel = sample.numel()
        if self.sde:
            noise = variance_noise if variance_noise is not None else randn_tensor(
                model_output.shape, generator=generator, device=model_output.device, dtype=torch.float32)
            buf = torch.empty(ops.dpm_buffer_numel(1, numel, True), device=sample.device, dtype=torch.float32)
            buf[:ops.DPM_ROW].copy_(row)
            buf[ops.DPM_ROW:].copy_(noise.to(sample.device, torch.float32).reshape(-1))
        else:
            buf = row.to(sample.device).view(1, ops.DPM_ROW)
        x = sample.float().contiguous().clone()
        eps = model_output.float().contiguous()
        # the history operand: the previous x0 going in (read by a second-order row), this step's coming out
        hist = self.model_outputs[-1].float().contiguous().clone() if second else torch.empty_like(x)
        flat = lambda t: t.view(1, 1, 1, 1, t.numel())  # noqa: E731  elementwise view
        ops.dpm_cfg_step(eps.view(-1, 1), 1, 1.0, flat(x), buf, x0_out=flat(hist))
        self.model_outputs = self.model_outputs[1:] + [hist]
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        prev = x.to(model_output.dtype)
        if not return_dict:
            return (prev,)
        return DPMSolverMultistepSchedulerOutput(prev_sample=prev)

    def __len__(self):
        return self.config.num_train_timesteps
