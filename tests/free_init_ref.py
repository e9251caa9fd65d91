"""FreeInit reference (test infrastructure, CPU): diffusers' `FreeInitMixin`
(diffusers.pipelines.free_init_utils: enable_free_init, _get_free_init_freq_filter,
_apply_freq_filter, _apply_free_init) restated with torch.fft.

PARITY STATUS: diffusers is not installed here, so this is a restatement from its published
source, unpinned like the rest of oracle/.  diffusers builds the mask with three Python loops in
a float32 tensor and runs the transforms on fp32 latents; here the mask is evaluated with the
same expressions on index grids, in `dtype` (fp64 for the kernel tests), and the transforms run
in the dtype of their input.
"""
from __future__ import annotations

import math

import torch
from torch import fft

FREE_INIT_DEFAULTS = dict(num_iters=3, use_fast_sampling=False, method="butterworth", order=4,
                          spatial_stop_frequency=0.25, temporal_stop_frequency=0.25)


def _get_free_init_freq_filter(shape, filter_type, order, spatial_stop_frequency, temporal_stop_frequency,
                               dtype=torch.float64):
    """The low-pass mask over shape[-3:] = (T, H, W), indexed in fftshift-ed order."""
    time, height, width = shape[-3], shape[-2], shape[-1]
    mask = torch.zeros(tuple(shape), dtype=dtype)
    if spatial_stop_frequency == 0 or temporal_stop_frequency == 0:
        return mask
    ds = spatial_stop_frequency
    if filter_type == "butterworth":
        def retrieve_mask(x):
            return 1 / (1 + (x / ds ** 2) ** order)
    elif filter_type == "gaussian":
        def retrieve_mask(x):
            return torch.exp(-1 / (2 * ds ** 2) * x)
    elif filter_type == "ideal":
        def retrieve_mask(x):
            return (x <= ds * 2).to(dtype)
    else:
        raise NotImplementedError("`filter_type` must be one of gaussian, butterworth or ideal")
    t = torch.arange(time, dtype=dtype)[:, None, None]
    h = torch.arange(height, dtype=dtype)[None, :, None]
    w = torch.arange(width, dtype=dtype)[None, None, :]
    d_square = ((ds / temporal_stop_frequency) * (2 * t / time - 1)) ** 2 + (2 * h / height - 1) ** 2 \
        + (2 * w / width - 1) ** 2
    return mask + retrieve_mask(d_square)


def _apply_freq_filter(x, noise, low_pass_filter):
    """diffusers' _apply_freq_filter: the low frequencies of x, the high ones of noise."""
    dims = (-3, -2, -1)
    x_freq = fft.fftshift(fft.fftn(x, dim=dims), dim=dims)
    noise_freq = fft.fftshift(fft.fftn(noise, dim=dims), dim=dims)
    high_pass_filter = 1 - low_pass_filter
    x_freq_mixed = x_freq * low_pass_filter + noise_freq * high_pass_filter
    return fft.ifftn(fft.ifftshift(x_freq_mixed, dim=dims), dim=dims).real


def fast_sampling_steps(num_inference_steps, num_iters, iteration):
    """The step count of one iteration under use_fast_sampling."""
    return max(1, int(num_inference_steps / num_iters * (iteration + 1)))


class FreeInit:
    """The mixin's state and _apply_free_init over a scheduler with add_noise and
    config.num_train_timesteps; randn is the draw (diffusers' randn_tensor)."""

    def __init__(self, scheduler, randn, num_iters=3, use_fast_sampling=False, method="butterworth", order=4,
                 spatial_stop_frequency=0.25, temporal_stop_frequency=0.25):
        self.scheduler, self.randn = scheduler, randn
        self.num_iters, self.use_fast_sampling = num_iters, use_fast_sampling
        self.method, self.order = method, order
        self.ds, self.dt = spatial_stop_frequency, temporal_stop_frequency
        self.initial_noise = None

    def apply(self, latents, iteration, num_inference_steps, generator, dtype=torch.float32):
        """-> (latents, the iteration's step count)."""
        if iteration == 0:
            self.initial_noise = latents.detach().clone()
        else:
            shape = latents.shape
            lpf = _get_free_init_freq_filter((1,) + tuple(shape[1:]), self.method, self.order, self.ds, self.dt,
                                             dtype=dtype)
            t = self.scheduler.config.num_train_timesteps - 1
            z_t = self.scheduler.add_noise(latents, self.initial_noise, torch.full((shape[0],), t)).to(torch.float32)
            z_rand = self.randn(shape, generator=generator, device=latents.device, dtype=torch.float32)
            latents = _apply_freq_filter(z_t.to(dtype), z_rand.to(dtype), lpf).to(latents.dtype)
        if self.use_fast_sampling:
            num_inference_steps = fast_sampling_steps(num_inference_steps, self.num_iters, iteration)
        return latents, num_inference_steps


def half_spectrum_filter(x, noise, table):
    """The identity the kernel rests on, with torch.fft: noise + irfftn(table * rfftn(x - noise)),
    table the Hermitian-even mask in DFT order cut to kw <= W / 2 (vdiff.ops.free_init_table)."""
    dims = (-3, -2, -1)
    return noise + fft.irfftn(fft.rfftn(x - noise, dim=dims) * table, s=x.shape[-3:], dim=dims)


def centre_value(filter_type, order, ds):
    """The mask at d^2 = 0."""
    return {"butterworth": 1.0, "gaussian": math.exp(0.0), "ideal": 1.0 if ds > 0 else 0.0}[filter_type]
