"""UniPCMultistepScheduler — drop-in for diffusers:UniPCMultistepScheduler, the predictor-corrector
solver diffusers' ControlNet and video examples switch to for 10-20 step sampling:
`pipe.scheduler = UniPCMultistepScheduler.from_config(pipe.scheduler.config)`.

Supported: solver_order 1 and 2, solver_type "bh1" and "bh2", disable_corrector, Karras sigmas,
the three timestep spacings, steps_offset, final_sigmas_type "zero" and "sigma_min", linear /
scaled_linear / trained betas.  Everything else of diffusers' config is refused by name.

Timesteps and sigmas follow the rules diffusers' two multistep schedulers share (dpm.build_schedule).

One step at schedule index i (sigmas s[0..n], s[n] the appended final sigma; alpha = 1 / sqrt(s^2 + 1),
sig = s alpha, lambda = log alpha - log sig) does, on ONE model output:
  m_t = (x - sig_i eps) / alpha_i                                    the x0 prediction at x
  corrector (UniC, not on the first step of a run, not after a step in disable_corrector): redo the
    previous step i-1 -> i at one order more, now that m_t is known
      x <- sig_i/sig_{i-1} last - alpha_i h_phi_1 m0 - alpha_i B_h (rho0 (m_-2 - m0)/rk + rhot (m_t - m0))
  predictor (UniP): the step i -> i+1 from the corrected x
      x_next = sig_{i+1}/sig_i x - alpha_{i+1} h_phi_1 m_t - alpha_{i+1} B_h (0.5 (m0 - m_t)/rk)
with h the log-SNR step, hh = -h, h_phi_1 = expm1(hh), B_h = expm1(hh) ("bh2") or hh ("bh1"); the
rk / rho0 terms only at second order.  The corrector raises the order of accuracy by one with no
extra model call.  The device kernel (vd_ddim_cfg_step with VD_STEP_UNIPC, ops.unipc_cfg_step)
does all of it in one pass and keeps the state — m0, m_-2 and `last` — in its three-slab x0_out
operand, in and out, so the pipeline's captured graph replays over the whole schedule.

Rows go by POSITION in the current schedule, as DPMSolverMultistepScheduler's: row j of
`coefficient_table(ts)` is schedule index pos + j after j steps of the run.  Row 0 has no corrector
and a first-order predictor — what diffusers' step does on a video-to-video slice of the schedule,
from a fresh `lower_order_nums` and `last_sample`.

Coefficients are computed in fp64 from the fp32 sigmas (math.log / math.expm1, the C library's) and
rounded once; diffusers computes them in fp32 torch ops.  The second-order corrector's weights
(rho0, rhot) solve diffusers' 2x2 system [[1, 1], [rk, 1]] rho = b in closed form (rk < 0: never
singular).  Parity to diffusers is UNPINNED (diffusers is not installed where this is tested);
tests/unipc_ref.py restates diffusers' scheduler in plain torch, a convergence-order check pins that
restatement, and the kernel is held to it bit for bit.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from .. import ops
from .ddim import _Cfg, sqrt32
from .dpm import DPMSolverMultistepScheduler as _DPM
from .dpm import alpha_sigma, build_schedule

UniPCMultistepSchedulerOutput = namedtuple("UniPCMultistepSchedulerOutput", ["prev_sample"])

# diffusers' UniPCMultistepScheduler.__init__ defaults
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
    predict_x0=True,
    solver_type="bh2",
    lower_order_final=True,
    disable_corrector=[],
    solver_p=None,
    use_karras_sigmas=False,
    use_exponential_sigmas=False,
    use_beta_sigmas=False,
    use_flow_sigmas=False,
    timestep_spacing="linspace",
    steps_offset=0,
    final_sigmas_type="zero",
    rescale_betas_zero_snr=False,
)

FLAG_CORRECTOR, FLAG_CORRECTOR_SECOND, FLAG_PREDICTOR_SECOND = 1, 2, 4  # row slot 12 (include/vdiff.h)


def _lam(sigma):
    """(alpha, sig, lambda) of a schedule sigma in Python floats; sigma 0 -> lambda +inf."""
    a, s = map(float, alpha_sigma(sigma))
    return a, s, (math.log(a) - math.log(s)) if s > 0.0 else math.inf


def _bh(h, bh2: bool):
    """(hh, h_phi_1, B_h) of a log-SNR step h under predict_x0.  h = +inf (a final sigma of 0)
    gives h_phi_1 = -1."""
    hh = -h
    h_phi_1 = math.expm1(hh)
    return hh, h_phi_1, (h_phi_1 if bh2 else hh)


def unipc_row64(sigmas, i: int, corrector_order: int, predictor_order: int, bh2: bool = True) -> torch.Tensor:
    """The 16 coefficients of the step at index i of `sigmas` (floats, s[0..n]) in fp64, before
    their one rounding: {alpha_s, sigma_s, c_last, c_m, c_B, rk_c, rho0, rhot, p_x, p_m, p_B, rk_p,
    flags, 0, 0, 0}.  corrector_order 0: no corrector.  A slot the row does not use stays 0.0."""
    # log and expm1 through Python's math (the C library's), not numpy's vectorised ones, whose last
    # bit depends on the host's instruction set
    a_i, s_i, l_i = _lam(sigmas[i])
    row = [0.0] * 16
    row[0], row[1] = a_i, s_i
    flags = 0
    if corrector_order:
        _, s_p, l_p = _lam(sigmas[i - 1])
        h = l_i - l_p
        hh, h_phi_1, B_h = _bh(h, bh2)
        row[2], row[3], row[4] = s_i / s_p, a_i * h_phi_1, a_i * B_h
        flags |= FLAG_CORRECTOR
        if corrector_order == 1:
            row[7] = 0.5
        else:
            rk = (_lam(sigmas[i - 2])[2] - l_p) / h
            b1 = (h_phi_1 / hh - 1.0) / B_h
            b2 = 2.0 * ((h_phi_1 / hh - 1.0) / hh - 0.5) / B_h
            rho0 = (b1 - b2) / (1.0 - rk)
            row[5], row[6], row[7] = rk, rho0, b1 - rho0
            flags |= FLAG_CORRECTOR_SECOND
    a_n, s_n, l_n = _lam(sigmas[i + 1])
    h = l_n - l_i
    hh, h_phi_1, B_h = _bh(h, bh2)
    row[8], row[9] = s_n / s_i, a_n * h_phi_1
    if predictor_order == 2:
        row[10], row[11] = a_n * B_h, (_lam(sigmas[i - 1])[2] - l_i) / h
        flags |= FLAG_PREDICTOR_SECOND
    row[12] = float(flags)
    row = torch.tensor(row, dtype=torch.float64)
    if not torch.isfinite(row).all():
        raise ValueError(f"UniPC row {i} of sigmas {list(sigmas[max(i - 2, 0):i + 2])} is not finite: {row.tolist()}")
    return row


def unipc_row(sigmas, i: int, corrector_order: int, predictor_order: int, bh2: bool = True) -> torch.Tensor:
    """unipc_row64 rounded once to fp32: a row of the device table.  A schedule that repeats a
    sigma (a log-SNR step h = 0 that a coefficient divides by) is refused like a non-finite row."""
    try:
        return unipc_row64(sigmas, i, corrector_order, predictor_order, bh2).float()
    except ZeroDivisionError:
        raise ValueError(f"UniPC row {i} of sigmas {list(sigmas[max(i - 2, 0):i + 2])} is not finite: a repeated "
                         "sigma makes a log-SNR step of 0") from None


class UniPCMultistepScheduler:
    kind = "unipc"  # selects the fused device update (ops.SCHED_STEP)
    order = 1       # diffusers' scheduler.order: one model call per step
    init_noise_sigma = 1.0

    def __init__(self, **kwargs):
        cfg = dict(DEFAULT_CONFIG)
        cfg.update({k: v for k, v in kwargs.items() if k in cfg})
        cfg["disable_corrector"] = list(cfg["disable_corrector"])
        if cfg["solver_type"] in ("midpoint", "heun", "logrho"):
            cfg["solver_type"] = "bh2"  # diffusers': another multistep scheduler's config goes in
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
        if not cfg["predict_x0"]:
            raise NotImplementedError("predict_x0=False (the noise-prediction form of the solver)")
        if cfg["solver_type"] not in ("bh1", "bh2"):
            raise ValueError(f"solver_type {cfg['solver_type']!r}: 'bh1' or 'bh2'")
        if not cfg["lower_order_final"]:
            raise NotImplementedError("lower_order_final=False: a second-order last step onto a final sigma of 0 "
                                      "divides by its log-SNR step h = inf")
        if cfg["solver_p"] is not None:
            raise NotImplementedError("solver_p (another scheduler as the predictor)")
        for name in ("use_exponential_sigmas", "use_beta_sigmas", "use_flow_sigmas"):
            if cfg[name]:
                raise NotImplementedError(name)
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
        self._fresh()

    def _fresh(self):
        """No step of a run taken yet: no history, no last sample."""
        self.model_outputs = [None] * self.config.solver_order
        self.lower_order_nums = 0
        self.this_order = None
        self.last_sample = None
        self._step_index = None
        self._begin_index = None

    @classmethod
    def from_config(cls, config, **kwargs):
        base = dict(config) if config is not None else {}
        base.update(kwargs)
        return cls(**base)

    @property
    def bh2(self) -> bool:
        return self.config.solver_type == "bh2"

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    def set_timesteps(self, num_inference_steps: int, device=None):
        """diffusers' set_timesteps, the rules of DPMSolverMultistepScheduler's: n timesteps, n + 1 fp32 sigmas."""
        ts, self.sigmas = build_schedule(self.config, self.train_sigmas, num_inference_steps)
        self.timesteps = torch.from_numpy(np.asarray(ts).astype(np.int64)).to(device)
        self.num_inference_steps = len(ts)
        self._fresh()

    # the schedule lookups and add_noise are those of diffusers' other multistep scheduler
    index_for_timestep = _DPM.index_for_timestep
    _init_step_index = _DPM._init_step_index
    _position = _DPM._position
    add_noise = _DPM.add_noise

    def scale_model_input(self, sample, timestep=None):
        return sample

    # ------------------------------------------------------------------ rows
    def _orders_at(self, idx: int, taken: int):
        """diffusers' step decisions at schedule index idx after `taken` steps of this run ->
        (the corrector's order, 0 when it does not run; the predictor's order).  The corrector
        redoes the previous step at the order that step's predictor used."""
        n, so = len(self.timesteps), self.config.solver_order
        corrector = 0
        if taken > 0 and idx > 0 and (idx - 1) not in self.config.disable_corrector:
            corrector = min(so, n - (idx - 1), taken)
        return corrector, min(so, n - idx, taken + 1)

    def _row_at(self, idx: int, taken: int) -> torch.Tensor:
        return unipc_row(self.sigmas.tolist(), idx, *self._orders_at(idx, taken), self.bh2)

    def coefficients(self, i: int) -> torch.Tensor:
        """The fp32 row of step index i of the current schedule (module docstring, include/vdiff.h)."""
        return self.coefficient_table(self.timesteps)[i]

    def coefficient_table(self, timesteps=None) -> torch.Tensor:
        """[n, 16] rows for a run of the current schedule (default: all of it).  Row 0 has no
        corrector and a first-order predictor."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        ts = (self.timesteps if timesteps is None else torch.as_tensor(timesteps)).cpu().tolist()
        pos = self._position(ts)
        return torch.stack([self._row_at(pos + j, j) for j in range(len(ts))])

    # ------------------------------------------------------------------ step
    def step(self, model_output, timestep, sample, return_dict: bool = True):
        """diffusers' step on the HIP kernel with a one-row table and a three-slab state built from
        `model_outputs` (the last solver_order x0 predictions) and `last_sample`; `this_order` and
        `lower_order_nums` move as in diffusers."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        if not (model_output.is_cuda and sample.is_cuda):
            raise ValueError("UniPCMultistepScheduler.step runs the HIP kernel; tensors must be on the GPU")
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        if i >= len(self.timesteps):
            raise ValueError(f"step {i} of a {len(self.timesteps)}-step schedule: call set_timesteps() to start over")
        # lower_order_nums saturates at solver_order, where the count of steps taken no longer matters
        corrector, predictor = self._orders_at(i, self.lower_order_nums)
        assert corrector in (0, self.this_order)
        row = unipc_row(self.sigmas.tolist(), i, corrector, predictor, self.bh2)
        x = sample.float().contiguous().clone()
        eps = model_output.float().contiguous()
        # the state operand: {m0, m_-2, last} going in (each read only by the rows that need it),
        # {this step's x0, m0, the corrected sample} coming out
        state = torch.empty((3,) + tuple(x.shape), device=x.device, dtype=torch.float32)
        older = self.model_outputs[-2] if self.config.solver_order == 2 else None
        for slab, t in zip(state, (self.model_outputs[-1], older, self.last_sample)):
            if t is not None:
                slab.copy_(t)
        flat = lambda t: t.view(1, 1, 1, 1, t.numel())  # noqa: E731  elementwise view
        ops.unipc_cfg_step(eps.view(-1, 1), 1, 1.0, flat(x), row.to(x.device).view(1, ops.UNIPC_ROW), x0_out=state)
        had = self.model_outputs[-1] is not None
        self.model_outputs = [state[1] if had else None, state[0]][-self.config.solver_order:]
        self.last_sample = state[2]
        self.this_order = predictor
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        prev = x.to(model_output.dtype)
        if not return_dict:
            return (prev,)
        return UniPCMultistepSchedulerOutput(prev_sample=prev)

    def __len__(self):
        return self.config.num_train_timesteps
