"""fp64 plain-torch restatement of diffusers' AutoencoderKL.encode (SD-1.5's `vae`), the reference
of tests/test_vae_encoder_host.py and tests/test_gpu_vae_encoder.py.

diffusers is absent, so this restates its published algorithm (PARITY STATUS: unpinned against
diffusers, like oracle/vae_ref.py, whose `resnet` and `attention` it reuses read-only):
  * AutoencoderKL.encode: moments = quant_conv(encoder(x)) (1x1); latent_dist =
    DiagonalGaussianDistribution(moments): mean | logvar = chunk(moments, 2, dim=1);
  * Encoder: conv_in 3x3 (3 -> C_0); DownEncoderBlock2D per block_out_channels entry
    (layers_per_block resnets, Downsample2D(padding=0) on all but the last); UNetMidBlock2D
    (resnet, single-head attention, resnet); conv_norm_out GroupNorm(32, eps 1e-6), SiLU,
    conv_out 3x3 -> 2 * latent_channels;
  * Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)) then conv 3x3, stride 2, no padding.

`rnd` is applied wherever the device path stores an activation in bf16 (the packed input rows,
every conv / GroupNorm+SiLU / attention output; quant_conv's output stays fp32); the arithmetic
between the roundings stays fp64, so the emulation lacks the device's fp32 accumulation order and
the flash kernel's bf16 probabilities.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.vae_ref import attention, resnet


def ident(x):
    return x


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def downsample(x, w, b=None):
    """Downsample2D(padding=0): zeros past the far edges only, then the stride-2 conv."""
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)


def downsample_taps(x, w, b=None):
    """The same by direct tap summation: out[oh, ow] = sum over dy, dx of w[dy, dx] . x[2 oh + dy,
    2 ow + dx], a tap past the input contributing nothing; (H - 2) // 2 + 1 output rows."""
    N, C, H, W = x.shape
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    out = torch.zeros(N, w.shape[0], Ho, Wo, dtype=x.dtype)
    for oh in range(Ho):
        for ow in range(Wo):
            for dy in range(3):
                for dx in range(3):
                    ih, iw = 2 * oh + dy, 2 * ow + dx
                    if ih < H and iw < W:
                        out[:, :, oh, ow] += x[:, :, ih, iw] @ w[:, :, dy, dx].T
    return out if b is None else out + b[None, :, None, None]


def _conv(sd, p, x):
    return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], padding=1)


def encoder(sd, cfg, x, rnd=ident):
    g = cfg["norm_num_groups"]
    ch = list(cfg["block_out_channels"])
    x = rnd(_conv(sd, "encoder.conv_in", rnd(x)))
    for i in range(len(ch)):
        for j in range(cfg["layers_per_block"]):
            x = resnet(sd, f"encoder.down_blocks.{i}.resnets.{j}", x, g, rnd=rnd)
        if i < len(ch) - 1:
            p = f"encoder.down_blocks.{i}.downsamplers.0.conv"
            x = rnd(downsample(x, sd[p + ".weight"], sd[p + ".bias"]))
    x = resnet(sd, "encoder.mid_block.resnets.0", x, g, rnd=rnd)
    x = attention(sd, "encoder.mid_block.attentions.0", x, g, rnd=rnd)
    x = resnet(sd, "encoder.mid_block.resnets.1", x, g, rnd=rnd)
    x = rnd(F.silu(F.group_norm(x, g, sd["encoder.conv_norm_out.weight"], sd["encoder.conv_norm_out.bias"], 1e-6)))
    return rnd(_conv(sd, "encoder.conv_out", x))


def moments(sd, cfg, x, rnd=ident):
    """AutoencoderKL.encode's moments (N, 2 * latent_channels, h, w) in fp64 for x (N, 3, H, W);
    sd any float dtype (taken to fp64)."""
    sd = {k: v.double() for k, v in sd.items() if k.startswith(("encoder.", "quant_conv."))}
    with torch.no_grad():
        h = encoder(sd, cfg, x.double(), rnd=rnd)
        return F.conv2d(h, sd["quant_conv.weight"], sd["quant_conv.bias"])


def rel_l2(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).norm() / want.norm()).item()
