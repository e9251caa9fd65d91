"""FreeU reference (test infrastructure, CPU): diffusers' `fourier_filter` / `apply_freeu`
(diffusers.utils.torch_utils, called from UpBlockMotion / CrossAttnUpBlockMotion.forward before
each skip concat) restated with torch.fft, the closed form the HIP kernel evaluates, and
oracle/unet_ref.unet_forward's loop rebuilt from unet_ref's public pieces with apply_freeu
inserted before the torch.cat.

PARITY STATUS: diffusers is not installed here, so this is a restatement from its published
source, unpinned like the rest of oracle/.  diffusers up-casts non-power-of-two sizes and bf16
inputs to fp32 and runs the FFT of a power-of-two fp16 input in fp16; everything here runs in
the dtype of its input, fp64 for the kernel tests.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import fft

from oracle import unet_ref


def fourier_filter(x, threshold, scale):
    """diffusers.utils.torch_utils.fourier_filter on (N, C, H, W): fftn over (H, W), fftshift,
    the centred 2*threshold box times `scale`, ifftshift, ifftn, real part."""
    n, c, h, w = x.shape
    xf = fft.fftshift(fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((n, c, h, w), dtype=x.dtype)
    crow, ccol = h // 2, w // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    xf = xf * mask
    return fft.ifftn(fft.ifftshift(xf, dim=(-2, -1)), dim=(-2, -1)).real.to(x.dtype)


def closed_form(x, s):
    """fourier_filter(x, 1, s) without an FFT: the box holds the bins k_h, k_w in {-1, 0}, so
    per plane out = x + (s - 1) / (H W) * (A + B cos th + C sin th + D cos tw + E sin tw +
    P cos(th + tw) + Q sin(th + tw)), A .. Q = the plane's sums of x times the same factors."""
    n, c, h, w = x.shape
    th = (2 * math.pi * torch.arange(h, dtype=x.dtype) / h)[:, None].expand(h, w)
    tw = (2 * math.pi * torch.arange(w, dtype=x.dtype) / w)[None, :].expand(h, w)
    basis = torch.stack([torch.ones(h, w, dtype=x.dtype), th.cos(), th.sin(), tw.cos(), tw.sin(),
                         (th + tw).cos(), (th + tw).sin()])                     # (7, H, W)
    sums = torch.einsum("nchw,khw->nck", x, basis)
    corr = torch.einsum("nck,khw->nchw", sums, basis)
    return x + (s - 1) / (h * w) * corr


def apply_freeu(resolution_idx, hidden_states, res_hidden_states, s1, s2, b1, b2, filt=None):
    """diffusers.utils.torch_utils.apply_freeu (out of place).  filt: the filter to use, default
    fourier_filter(., threshold=1, .)."""
    filt = filt or (lambda r, s: fourier_filter(r, 1, s))
    if resolution_idx in (0, 1):
        b, s = (b1, s1) if resolution_idx == 0 else (b2, s2)
        half = hidden_states.shape[1] // 2
        hidden_states = torch.cat([hidden_states[:, :half] * b, hidden_states[:, half:]], 1)
        res_hidden_states = filt(res_hidden_states, s)
    return hidden_states, res_hidden_states


def unet_forward_freeu(sd, cfg, sample, timestep, encoder_hidden_states, freeu=None, act="fp32"):
    """oracle/unet_ref.unet_forward with FreeU: freeu = (s1, s2, b1, b2) or None.  The two results
    of apply_freeu pass through `rnd` (the device stores both as bf16).  With freeu=None every
    operation is unet_forward's, in its order: the outputs are equal bit for bit."""
    U = unet_ref
    rnd = U.ROUNDERS[act]
    g, eps = cfg["norm_num_groups"], cfg["norm_eps"]
    heads, mheads, mlen = cfg["num_attention_heads"], cfg["motion_num_attention_heads"], cfg["motion_max_seq_length"]
    sample = sample.float()
    b, _, nf, hh, ww = sample.shape
    t = torch.as_tensor(timestep)
    if t.ndim == 0:
        t = t[None]
    t = t.expand(b)
    temb = rnd(U.timestep_embedding(t, cfg["block_out_channels"][0]))
    temb = rnd(F.silu(U.linear(sd, "time_embedding.linear_1", temb)))
    temb = U.linear(sd, "time_embedding.linear_2", temb)
    temb_silu = rnd(F.silu(temb)).repeat_interleave(nf, 0)
    ehs = rnd(encoder_hidden_states.float()).repeat_interleave(nf, 0)

    x = rnd(sample).permute(0, 2, 1, 3, 4).reshape(b * nf, -1, hh, ww)
    x = rnd(U.conv(sd, "conv_in", x))
    skips = [x]
    for i, (ins, has_attn, down) in enumerate(U._down_plan(cfg)):
        p = f"down_blocks.{i}"
        for j in range(len(ins)):
            x = U.resnet(sd, f"{p}.resnets.{j}", x, temb_silu, g, eps, rnd)
            if has_attn:
                x = U.transformer2d(sd, f"{p}.attentions.{j}", x, ehs, heads, g, rnd)
            x = U.motion_module(sd, f"{p}.motion_modules.{j}", x, nf, mheads, g, mlen, rnd)
            skips.append(x)
        if down:
            x = rnd(U.conv(sd, f"{p}.downsamplers.0.conv", x, stride=2, padding=1))
            skips.append(x)
    x = U.resnet(sd, "mid_block.resnets.0", x, temb_silu, g, eps, rnd)
    x = U.transformer2d(sd, "mid_block.attentions.0", x, ehs, heads, g, rnd)
    if cfg.get("use_motion_mid_block", True):
        x = U.motion_module(sd, "mid_block.motion_modules.0", x, nf, mheads, g, mlen, rnd)
    x = U.resnet(sd, "mid_block.resnets.1", x, temb_silu, g, eps, rnd)
    for i, (ins, has_attn, up) in enumerate(U._up_plan(cfg)):
        p = f"up_blocks.{i}"
        for j in range(len(ins)):
            skip = skips.pop()
            if freeu is not None:
                x, skip = apply_freeu(i, x, skip, *freeu)
                x, skip = rnd(x), rnd(skip)
            x = torch.cat([x, skip], dim=1)
            x = U.resnet(sd, f"{p}.resnets.{j}", x, temb_silu, g, eps, rnd)
            if has_attn:
                x = U.transformer2d(sd, f"{p}.attentions.{j}", x, ehs, heads, g, rnd)
            x = U.motion_module(sd, f"{p}.motion_modules.{j}", x, nf, mheads, g, mlen, rnd)
        if up:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = rnd(U.conv(sd, f"{p}.upsamplers.0.conv", x))
    x = rnd(F.silu(U.group_norm(sd, "conv_norm_out", x, g, eps)))
    x = U.conv(sd, "conv_out", x)
    return x.reshape(b, nf, -1, hh, ww).permute(0, 2, 1, 3, 4).contiguous()
