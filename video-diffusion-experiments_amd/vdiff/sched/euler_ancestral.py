"""EulerAncestralDiscreteScheduler — drop-in for diffusers:EulerAncestralDiscreteScheduler ("Euler a",
k-diffusion's sample_euler_ancestral), epsilon prediction:
`pipe.scheduler = EulerAncestralDiscreteScheduler.from_config(pipe.scheduler.config)`.

Betas, training sigmas, the inference timesteps for the three spacings, the interpolated sigmas with
their trailing 0, `scale_model_input`, `add_noise` and the step-index rules are
EulerDiscreteScheduler's (sched/euler.py, `_EulerSchedule`).  What differs is the step: from sigma
s to the schedule's next sigma t it goes deterministically down to sigma_down < t and adds fresh
noise of standard deviation sigma_up, with sigma_down^2 + sigma_up^2 = t^2:

    up2        = t**2 * (s**2 - t**2) / s**2        fp32 torch ops, diffusers' order
    sigma_up   = sqrt(up2)
    sigma_down = sqrt(t**2 - sigma_up**2)
    x0 = x - s*eps;  d = (x - x0) / s;  x <- x + d*(sigma_down - s);  x <- x + noise*sigma_up

The per-step row is {s, sigma_down, sqrt(t^2 + 1), sigma_up}: Euler's row with sigma_next replaced
and its unused zero filled.  Device side: `step()` runs the fused HIP kernel (vd_euler_cfg_step
with VD_STEP_ANCESTRAL) on one row and one noise slab; the pipeline's captured graph reads a table
of rows and one slab per step by a device step counter (pipeline.DenoiseLoop).  The last step of
every schedule has t = 0, so sigma_up = sigma_down = 0 and its noise is drawn (diffusers' draw
order) but never read.

The radicands are fp32 torch arithmetic; the square roots are correctly rounded (`sqrt32`, via
fp64).  This is the same deliberate divergence from diffusers as in sched/euler.py: diffusers takes
torch fp32 `** 0.5` on the host CPU, which is host-dependent at 1 ulp.  The table's parity against
diffusers is therefore UNPINNED at that level; tests/euler_ancestral_ref.py restates the scheduler
and is the reference the kernel and this table are held to bit for bit.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from .. import ops
from .ddim import _Cfg, sqrt32
from .euler import _EulerSchedule

EulerAncestralDiscreteSchedulerOutput = namedtuple("EulerAncestralDiscreteSchedulerOutput",
                                                   ["prev_sample", "pred_original_sample"])

# diffusers' EulerAncestralDiscreteScheduler.__init__ keys and defaults
DEFAULT_CONFIG = dict(
    num_train_timesteps=1000,
    beta_start=0.0001,
    beta_end=0.02,
    beta_schedule="linear",
    trained_betas=None,
    prediction_type="epsilon",
    timestep_spacing="linspace",
    steps_offset=0,
    rescale_betas_zero_snr=False,
)


class EulerAncestralDiscreteScheduler(_EulerSchedule):
    kind = "euler_a"

    def __init__(self, **kwargs):
        cfg = dict(DEFAULT_CONFIG)
        cfg.update({k: v for k, v in kwargs.items() if k in cfg})  # another scheduler's keys are ignored
        self.config = _Cfg(cfg)
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError(f"EulerAncestralDiscreteScheduler: prediction_type="
                                      f"{cfg['prediction_type']!r} is not supported, only 'epsilon'")
        if cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("EulerAncestralDiscreteScheduler: rescale_betas_zero_snr=True is not "
                                      "supported (its first sigma is infinite)")
        if cfg["trained_betas"] is None and cfg["beta_schedule"] not in ("linear", "scaled_linear"):
            raise NotImplementedError(f"EulerAncestralDiscreteScheduler: beta_schedule={cfg['beta_schedule']!r} "
                                      "is not supported, only 'linear' and 'scaled_linear'")
        self._init_sigmas(cfg)

    def sigma_up_down(self, i: int):
        """(sigma_up, sigma_down) of step index i as fp32 torch scalars, diffusers' operation order."""
        s, t = self.sigmas[i], self.sigmas[i + 1]
        up = sqrt32(t ** 2 * (s ** 2 - t ** 2) / s ** 2)
        down = sqrt32(t ** 2 - up ** 2)
        return up, down

    def coefficients(self, i: int) -> torch.Tensor:
        """fp32 {sigma_i, sigma_down, sqrt(sigma_{i+1}^2 + 1), sigma_up} for step index i; the last
        step's row is {sigma, 0, 1, 0}."""
        s, t = self.sigmas[i], self.sigmas[i + 1]
        up, down = self.sigma_up_down(i)
        return torch.stack([s, down, sqrt32(t ** 2 + 1), up]).float()

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True):
        """diffusers EulerAncestralDiscreteScheduler.step on the HIP kernel, with a one-row, one-slab
        buffer.  The noise is one randn_tensor(model_output.shape, generator, device,
        dtype=model_output.dtype) draw on every step, the last included (diffusers' draw order)."""
        from ..pipeline import randn_tensor
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        if not (model_output.is_cuda and sample.is_cuda):
            raise ValueError("EulerAncestralDiscreteScheduler.step runs the HIP kernel; tensors must be on the GPU")
        if self._step_index is None:
            self._init_step_index(timestep)
        numel = sample.numel()
        buf = torch.empty(ops.euler_a_buffer_numel(1, numel), device=sample.device, dtype=torch.float32)
        buf[:ops.EULER_A_ROW].copy_(self.coefficients(self._step_index))
        noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device,
                             dtype=model_output.dtype)
        buf[ops.EULER_A_ROW:].copy_(noise.reshape(-1))
        x = sample.float().contiguous().clone()
        eps = model_output.float().contiguous()
        x0 = torch.empty_like(x)
        flat = lambda t: t.view(1, 1, 1, 1, t.numel())  # noqa: E731  elementwise view
        ops.euler_ancestral_cfg_step(eps.view(-1, 1), 1, 1.0, flat(x), buf, x0_out=flat(x0))
        self._step_index += 1
        prev = x.to(model_output.dtype)
        if not return_dict:
            return (prev,)
        return EulerAncestralDiscreteSchedulerOutput(prev_sample=prev, pred_original_sample=x0)
