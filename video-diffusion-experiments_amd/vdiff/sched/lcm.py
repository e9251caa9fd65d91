"""LCMScheduler — drop-in for diffusers:LCMScheduler (latent consistency models; with the
AnimateLCM LoRA it samples a video in 4-8 steps at guidance ~2):
`LCMScheduler.from_config(pipe.scheduler.config, beta_schedule="linear")`.

Host side (numpy/torch-CPU, once per video): beta/alpha tables, the LCM timestep rule
(a sub-sequence of the `original_inference_steps` training-time schedule) and the per-step
coefficient rows.  Device side: `step()` runs the fused HIP kernel (vd_ddim_cfg_step with
VD_STEP_LCM, ops.lcm_cfg_step); the pipeline's captured graph reads the same rows, and the
per-step noise that follows them in the same buffer, by a device step counter.

The step is stochastic: every step but the last re-noises the denoised sample,
  x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t);  denoised = c_out x0 + c_skip x
  x <- sqrt(a_prev) denoised + sqrt(1-a_prev) noise          (the last step: x <- denoised)
where a_prev is the alpha of the NEXT SCHEDULE TIMESTEP, not of t - T // n as in DDIM.

Square roots are correctly rounded (`sqrt32`), as in the other two schedulers.  Parity to
diffusers is UNPINNED (diffusers is not installed where this is tested); tests/lcm_ref.py
restates diffusers' LCMScheduler in plain torch and the kernel is held to it bit for bit.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .. import ops
from .ddim import DEFAULT_CONFIG as _SD15, _Cfg, sqrt32

LCMSchedulerOutput = namedtuple("LCMSchedulerOutput", ["prev_sample", "denoised"])

# diffusers' LCMScheduler.__init__ defaults
DEFAULT_CONFIG = dict(
    num_train_timesteps=1000,
    beta_start=_SD15["beta_start"],
    beta_end=_SD15["beta_end"],
    beta_schedule="scaled_linear",
    trained_betas=None,
    original_inference_steps=50,
    clip_sample=False,
    clip_sample_range=1.0,
    set_alpha_to_one=True,
    steps_offset=0,
    prediction_type="epsilon",
    thresholding=False,
    timestep_spacing="leading",
    timestep_scaling=10.0,
    rescale_betas_zero_snr=False,
)

SIGMA_DATA = 0.5  # diffusers' get_scalings_for_boundary_condition_discrete


class LCMScheduler:
    order = 1
    kind = "lcm"  # selects the fused device update (ops.SCHED_STEP)
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
            raise NotImplementedError(cfg["beta_schedule"])
        if cfg["rescale_betas_zero_snr"]:
            raise NotImplementedError("rescale_betas_zero_snr")
        if cfg["prediction_type"] != "epsilon":
            raise NotImplementedError(f"prediction_type {cfg['prediction_type']!r}: only epsilon prediction")
        if cfg["clip_sample"]:
            raise NotImplementedError("clip_sample")
        if cfg["thresholding"]:
            raise NotImplementedError("thresholding")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg["set_alpha_to_one"] else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, n)[::-1].copy().astype(np.int64))
        self._step_index = None
        self._begin_index = None

    @classmethod
    def from_config(cls, config, **kwargs):
        base = dict(config) if config is not None else {}
        base.update(kwargs)
        return cls(**base)

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    def set_timesteps(self, num_inference_steps: int, device=None, original_inference_steps=None,
                      strength: float = 1.0):
        """diffusers' rule: the training-time LCM schedule `origin` holds every k-th timestep,
        k = T // original_steps, counted down from int(original_steps * strength) * k - 1; the
        inference timesteps are its entries at floor(linspace(0, len(origin), n, endpoint=False))."""
        T = self.config.num_train_timesteps
        original_steps = (original_inference_steps if original_inference_steps is not None
                          else self.config.original_inference_steps)
        if original_steps > T:
            raise ValueError(f"`original_steps`: {original_steps} cannot be larger than "
                             f"`self.config.train_timesteps`: {T}")
        k = T // original_steps
        origin = np.asarray(list(range(1, int(original_steps * strength) + 1))) * k - 1
        if num_inference_steps > T:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                             f"`self.config.train_timesteps`: {T}")
        if len(origin) // max(num_inference_steps, 1) < 1:
            raise ValueError(f"The combination of `original_steps x strength`: {original_steps} x {strength} is "
                             f"smaller than `num_inference_steps`: {num_inference_steps}")
        if num_inference_steps > original_steps:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                             f"`original_inference_steps`: {original_steps}")
        self.num_inference_steps = num_inference_steps
        origin = origin[::-1].copy()
        idx = np.floor(np.linspace(0, len(origin), num=num_inference_steps, endpoint=False)).astype(np.int64)
        self.timesteps = torch.from_numpy(origin[idx].astype(np.int64)).to(device)
        self._step_index = None
        self._begin_index = None

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        st = self.timesteps if schedule_timesteps is None else schedule_timesteps
        idx = (torch.as_tensor(st).cpu() == int(timestep)).nonzero()
        if len(idx) == 0:
            raise ValueError(f"timestep {int(timestep)} is not in the schedule")
        return int(idx[1 if len(idx) > 1 else 0])  # diffusers: the second match for img2img restarts

    def _init_step_index(self, timestep):
        self._step_index = self.index_for_timestep(timestep) if self._begin_index is None else self._begin_index

    def scale_model_input(self, sample, timestep=None):
        return sample

    def get_scalings_for_boundary_condition_discrete(self, timestep):
        """(c_skip, c_out) as Python floats (fp64)."""
        s = float(int(timestep)) * float(self.config.timestep_scaling)
        c_skip = SIGMA_DATA ** 2 / (s ** 2 + SIGMA_DATA ** 2)
        c_out = s / (s ** 2 + SIGMA_DATA ** 2) ** 0.5
        return c_skip, c_out

    def _row(self, t, t_prev, last: bool) -> torch.Tensor:
        a_t = self.alphas_cumprod[int(t)]
        a_p = self.alphas_cumprod[int(t_prev)] if int(t_prev) >= 0 else self.final_alpha_cumprod
        c_skip, c_out = self.get_scalings_for_boundary_condition_discrete(t)
        cs = torch.tensor([c_skip, c_out], dtype=torch.float64).float()
        return torch.stack([sqrt32(a_t), sqrt32(1 - a_t), sqrt32(a_p), sqrt32(1 - a_p), cs[0], cs[1],
                            torch.tensor(0.0 if last else 1.0), torch.zeros(())]).float()

    def coefficients(self, i: int) -> torch.Tensor:
        """The fp32 row of step index i of the current schedule:
        {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev), c_skip, c_out, add_noise, 0}.
        a_prev is the alpha of timesteps[i + 1] (the last step: of t itself, as diffusers, where
        it is unused because add_noise = 0).  Square roots through `sqrt32`.  c_skip and c_out are
        computed in fp64 and rounded once to fp32: diffusers computes them in fp32 torch ops on
        the timestep tensor, so they may differ from it in the last bit (unpinned)."""
        return self.coefficient_table(self.timesteps)[i]

    def coefficient_table(self, timesteps=None) -> torch.Tensor:
        """[n, 8] rows for a schedule (default: the whole current one); the `next timestep` of a
        row is the next entry of `timesteps`, and the last row has add_noise = 0."""
        ts = (self.timesteps if timesteps is None else torch.as_tensor(timesteps)).cpu().tolist()
        n = len(ts)
        return torch.stack([self._row(ts[i], ts[i + 1] if i + 1 < n else ts[i], i == n - 1) for i in range(n)])

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers LCMScheduler.add_noise (DDIM's): sqrt(a_t) * x + sqrt(1 - a_t) * noise in fp32."""
        t = torch.as_tensor(timesteps).reshape(-1).long().cpu()
        x = original_samples.float()
        shape = (-1,) + (1,) * (x.dim() - 1)
        sa = sqrt32(self.alphas_cumprod[t]).to(x.device).reshape(shape)
        sb = sqrt32(1 - self.alphas_cumprod[t]).to(x.device).reshape(shape)
        return sa * x + sb * noise.to(x.device, torch.float32)

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True):
        """diffusers LCMScheduler.step on the HIP kernel, with a one-row, one-slab buffer.  The
        noise is one randn_tensor(model_output.shape, generator, device, dtype=model_output.dtype)
        draw on every step but the last, which draws nothing."""
        from ..pipeline import randn_tensor
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() first")
        if not (model_output.is_cuda and sample.is_cuda):
            raise ValueError("LCMScheduler.step runs the HIP kernel; tensors must be on the GPU")
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        n = len(self.timesteps)
        last = i == n - 1
        t_prev = self.timesteps[i + 1] if i + 1 < n else timestep
        row = self._row(timestep, t_prev, last)
        numel = sample.numel()
        buf = torch.empty(ops.lcm_buffer_numel(1, numel), device=sample.device, dtype=torch.float32)
        buf[:ops.LCM_ROW].copy_(row)
        if not last:
            noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device,
                                 dtype=model_output.dtype)
            buf[ops.LCM_ROW:].copy_(noise.reshape(-1))
        x = sample.float().contiguous().clone()
        eps = model_output.float().contiguous()
        den = torch.empty_like(x)
        flat = lambda t: t.view(1, 1, 1, 1, t.numel())  # noqa: E731  elementwise view
        ops.lcm_cfg_step(eps.view(-1, 1), 1, 1.0, flat(x), buf, x0_out=flat(den))
        self._step_index += 1
        prev, den = x.to(sample.dtype), den.to(sample.dtype)
        if not return_dict:
            return (prev, den)
        return LCMSchedulerOutput(prev_sample=prev, denoised=den)

    def __len__(self):
        return self.config.num_train_timesteps
