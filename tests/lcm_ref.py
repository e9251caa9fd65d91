"""Test infrastructure only.  Never imported by the product path.

Restatement of `diffusers:LCMScheduler` (schedulers/scheduling_lcm.py) from its source, in plain
torch fp32 ops on the CPU: the beta / alpha tables, `set_timesteps`' LCM rule, the boundary
condition scalings and `step` for epsilon prediction without clipping or thresholding.  Parity
to diffusers itself is UNPINNED: diffusers is not installed where this runs, so nothing here
was compared against it.

Two deliberate choices, shared with vdiff.LCMScheduler and stated there too:
  * square roots are correctly rounded fp32 (through fp64), as oracle/ddim_ref.py takes them;
  * c_skip and c_out are computed in fp64 from the integer timestep and rounded once to fp32
    (diffusers evaluates them in torch ops on the timestep tensor).
"""
from __future__ import annotations

import numpy as np
import torch

SIGMA_DATA = 0.5


def _sqrt(x):
    """fp32 sqrt, correctly rounded whatever the host's fp32 vector sqrt does (through fp64)."""
    return torch.sqrt(torch.as_tensor(x).double()).float()


def alphas_cumprod(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, schedule="scaled_linear"):
    if schedule == "linear":
        betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
    elif schedule == "scaled_linear":
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    else:
        raise ValueError(schedule)
    return torch.cumprod(1.0 - betas, dim=0)


def lcm_timesteps(num_inference_steps, num_train_timesteps=1000, original_steps=50, strength=1.0):
    """LCMScheduler.set_timesteps without custom timesteps."""
    if original_steps > num_train_timesteps:
        raise ValueError("original_steps > num_train_timesteps")
    k = num_train_timesteps // original_steps
    origin = np.asarray(list(range(1, int(original_steps * strength) + 1))) * k - 1
    if num_inference_steps > num_train_timesteps:
        raise ValueError("num_inference_steps > num_train_timesteps")
    skipping_step = len(origin) // num_inference_steps
    if skipping_step < 1:
        raise ValueError("original_steps x strength is smaller than num_inference_steps")
    if num_inference_steps > original_steps:
        raise ValueError("num_inference_steps > original_steps")
    origin = origin[::-1].copy()
    idx = np.linspace(0, len(origin), num=num_inference_steps, endpoint=False)
    idx = np.floor(idx).astype(np.int64)
    return origin[idx]


def scalings(t, timestep_scaling=10.0):
    """get_scalings_for_boundary_condition_discrete -> fp32 (c_skip, c_out), from fp64."""
    s = float(int(t)) * float(timestep_scaling)
    c_skip = SIGMA_DATA ** 2 / (s ** 2 + SIGMA_DATA ** 2)
    c_out = s / (s ** 2 + SIGMA_DATA ** 2) ** 0.5
    return (torch.tensor(c_skip, dtype=torch.float64).float(), torch.tensor(c_out, dtype=torch.float64).float())


def alpha_prev(ts, i, acp, final_alpha_cumprod=1.0):
    """alpha_prod_t_prev of step index i: the alpha of the NEXT schedule timestep (of t itself on
    the last step, where diffusers sets prev_timestep = timestep and never uses it)."""
    prev = int(ts[i + 1]) if i + 1 < len(ts) else int(ts[i])
    return acp[prev] if prev >= 0 else torch.tensor(final_alpha_cumprod, dtype=torch.float32)


def row(ts, i, acp, timestep_scaling=10.0):
    """The 8 fp32 coefficients of step index i, in the device table's order."""
    a_t, a_p = acp[int(ts[i])], alpha_prev(ts, i, acp)
    c_skip, c_out = scalings(ts[i], timestep_scaling)
    add = torch.tensor(0.0 if i == len(ts) - 1 else 1.0)
    return torch.stack([_sqrt(a_t), _sqrt(1 - a_t), _sqrt(a_p), _sqrt(1 - a_p), c_skip, c_out, add,
                        torch.zeros(())]).float()


def table(ts, acp, timestep_scaling=10.0):
    return torch.stack([row(ts, i, acp, timestep_scaling) for i in range(len(ts))])


def cfg_combine(eps_u, eps_c, g):
    """noise_pred_uncond + g * (noise_pred_text - noise_pred_uncond)."""
    return eps_u + g * (eps_c - eps_u)


def lcm_step(eps, x, r, noise=None):
    """LCMScheduler.step for epsilon prediction with the coefficients of row r (see `row`), in
    diffusers' operation order, one fp32 torch op at a time -> (prev_sample, denoised).
    noise is read only when the row's add_noise is set (every step but the last)."""
    eps, x = eps.float(), x.float()
    sat, s1at, sap, s1ap, c_skip, c_out, add = (r[j] for j in range(7))
    x0 = (x - s1at * eps) / sat
    denoised = c_out * x0 + c_skip * x
    if float(add) != 0.0:
        return sap * denoised + s1ap * noise.float(), denoised
    return denoised, denoised
