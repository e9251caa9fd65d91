"""FreeNoise reference (test infrastructure, CPU): diffusers' `FreeNoiseTransformerBlock`
(`_get_frame_indices`, `_get_frame_weights`, the windowed forward with its tail rule) and
`AnimateDiffFreeNoiseMixin._prepare_latents_free_noise`, restated on top of oracle/unet_ref.py,
and oracle/unet_ref.unet_forward's loop rebuilt from unet_ref's public pieces with the windowed
motion module in place of the plain one.

PARITY STATUS: diffusers is not installed here, so this is a restatement from its published
source, unpinned like the rest of oracle/.  Two known differences: diffusers accumulates the
weighted window outputs in the model's dtype, here the sums and the division run in fp64 and are
rounded to fp32 once (so one window returns the plain module's bits); and the odd-length
delayed_reverse_sawtooth weights follow the source's own comment (5 -> [0.01, 0.01, 3, 2, 1]).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import unet_ref

SCHEMES = ("flat", "pyramid", "delayed_reverse_sawtooth")


def frame_indices(num_frames, context_length, context_stride):
    """_get_frame_indices plus forward()'s tail rule: ([(start, end), ...], tail_len).  The tail
    window, when the regular ones leave frames uncovered, is (F - L, F) and contributes only its
    last tail_len frames."""
    if num_frames < context_length:
        raise ValueError(f"num_frames {num_frames} < context_length {context_length}")
    idx = [(i, i + context_length) for i in range(0, num_frames - context_length + 1, context_stride)]
    tail_len = num_frames - idx[-1][1]
    if tail_len:
        idx.append((num_frames - context_length, num_frames))
    return idx, tail_len


def frame_weights(num_frames, weighting_scheme="pyramid"):
    """_get_frame_weights."""
    if weighting_scheme == "flat":
        return [1.0] * num_frames
    if weighting_scheme == "pyramid":
        if num_frames % 2 == 0:  # 4 => [1, 2, 2, 1]
            mid = num_frames // 2
            w = list(range(1, mid + 1))
            return [float(v) for v in w + w[::-1]]
        mid = (num_frames + 1) // 2  # 5 => [1, 2, 3, 2, 1]
        w = list(range(1, mid))
        return [float(v) for v in w + [mid] + w[::-1]]
    if weighting_scheme == "delayed_reverse_sawtooth":
        if num_frames % 2 == 0:  # 4 => [0.01, 2, 2, 1]
            mid = num_frames // 2
            return [0.01] * (mid - 1) + [float(mid)] + [float(v) for v in range(mid, 0, -1)]
        mid = (num_frames + 1) // 2  # 5 => [0.01, 0.01, 3, 2, 1]
        return [0.01] * (mid - 1) + [float(v) for v in range(mid, 0, -1)]
    raise ValueError(f"unsupported weighting scheme {weighting_scheme!r}")


def merge_windows(chunks, idx, tail_len, weights, num_frames):
    """forward()'s accumulation over (tokens, L, C) window outputs -> (tokens, F, C): weighted
    sums and their normaliser per frame, the tail window adding only its last tail_len frames.
    The weights are taken at their fp32 values (what a device table holds); fp64 sums."""
    w = torch.tensor(weights, dtype=torch.float32).double()[None, :, None]
    acc = torch.zeros(chunks[0].shape[0], num_frames, chunks[0].shape[2], dtype=torch.float64)
    cnt = torch.zeros(1, num_frames, 1, dtype=torch.float64)
    for i, ((a, b), c) in enumerate(zip(idx, chunks)):
        if tail_len and i == len(idx) - 1:
            acc[:, -tail_len:] += c[:, -tail_len:].double() * w[:, -tail_len:]
            cnt[:, -tail_len:] += w[:, -tail_len:]
        else:
            acc[:, a:b] += c.double() * w
            cnt[:, a:b] += w
    return (acc / cnt).float()


def motion_module(sd, p, x, num_frames, heads, groups, max_len, free_noise=None, rnd=unet_ref._ident):
    """unet_ref.motion_module with the transformer block run per window: free_noise =
    (context_length, context_stride, weighting_scheme) or None (the plain module).  The norm,
    proj_in and proj_out span all frames; each window gets the positional encoding of its own
    frames 0 .. L - 1.  The merged rows pass through `rnd` (the device stores them as bf16)."""
    if free_noise is None:
        return unet_ref.motion_module(sd, p, x, num_frames, heads, groups, max_len, rnd)
    U = unet_ref
    L, s, scheme = free_noise
    bf, c, hh, ww = x.shape
    b = bf // num_frames
    h = x.reshape(b, num_frames, c, hh, ww).permute(0, 2, 1, 3, 4)
    h = rnd(U.group_norm(sd, p + ".norm", h, groups, 1e-6))
    h = h.permute(0, 3, 4, 2, 1).reshape(b * hh * ww, num_frames, c)
    h = rnd(U.linear(sd, p + ".proj_in", h))
    pe = U.sinusoidal_pe(max_len, c)
    idx, tail_len = frame_indices(num_frames, L, s)
    chunks = [U.basic_transformer_block(sd, p + ".transformer_blocks.0", h[:, a:e], None, heads, pe=pe,
                                        double_self=True, rnd=rnd) for a, e in idx]
    h = rnd(merge_windows(chunks, idx, tail_len, frame_weights(L, scheme), num_frames))
    h = U.linear(sd, p + ".proj_out", h)
    h = h.reshape(b, hh, ww, num_frames, c).permute(0, 3, 4, 1, 2).reshape(bf, c, hh, ww)
    return rnd(h + x)


def unet_forward_free_noise(sd, cfg, sample, timestep, encoder_hidden_states, free_noise=None, act="fp32"):
    """oracle/unet_ref.unet_forward with FreeNoise in every motion module: free_noise =
    (context_length, context_stride, weighting_scheme) or None.  With None every operation is
    unet_forward's, in its order: the outputs are equal bit for bit."""
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

    def motion(p, x):
        return motion_module(sd, p, x, nf, mheads, g, mlen, free_noise, rnd)

    x = rnd(sample).permute(0, 2, 1, 3, 4).reshape(b * nf, -1, hh, ww)
    x = rnd(U.conv(sd, "conv_in", x))
    skips = [x]
    for i, (ins, has_attn, down) in enumerate(U._down_plan(cfg)):
        p = f"down_blocks.{i}"
        for j in range(len(ins)):
            x = U.resnet(sd, f"{p}.resnets.{j}", x, temb_silu, g, eps, rnd)
            if has_attn:
                x = U.transformer2d(sd, f"{p}.attentions.{j}", x, ehs, heads, g, rnd)
            x = motion(f"{p}.motion_modules.{j}", x)
            skips.append(x)
        if down:
            x = rnd(U.conv(sd, f"{p}.downsamplers.0.conv", x, stride=2, padding=1))
            skips.append(x)
    x = U.resnet(sd, "mid_block.resnets.0", x, temb_silu, g, eps, rnd)
    x = U.transformer2d(sd, "mid_block.attentions.0", x, ehs, heads, g, rnd)
    if cfg.get("use_motion_mid_block", True):
        x = motion("mid_block.motion_modules.0", x)
    x = U.resnet(sd, "mid_block.resnets.1", x, temb_silu, g, eps, rnd)
    for i, (ins, has_attn, up) in enumerate(U._up_plan(cfg)):
        p = f"up_blocks.{i}"
        for j in range(len(ins)):
            x = torch.cat([x, skips.pop()], dim=1)
            x = U.resnet(sd, f"{p}.resnets.{j}", x, temb_silu, g, eps, rnd)
            if has_attn:
                x = U.transformer2d(sd, f"{p}.attentions.{j}", x, ehs, heads, g, rnd)
            x = motion(f"{p}.motion_modules.{j}", x)
        if up:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = rnd(U.conv(sd, f"{p}.upsamplers.0.conv", x))
    x = rnd(F.silu(U.group_norm(sd, "conv_norm_out", x, g, eps)))
    x = U.conv(sd, "conv_out", x)
    return x.reshape(b, nf, -1, hh, ww).permute(0, 2, 1, 3, 4).contiguous()


def prepare_latents_free_noise(shape, num_frames, context_length, context_stride, noise_type, generator=None,
                               dtype=torch.float32, latents=None):
    """_prepare_latents_free_noise on the generator's device.  shape = (B, C, ., H, W); the frame
    count drawn is context_length for repeat_context and num_frames otherwise."""
    L, s = context_length, context_stride
    dev = generator.device if generator is not None else torch.device("cpu")
    if latents is None:
        n = L if noise_type == "repeat_context" else num_frames
        latents = torch.randn((shape[0], shape[1], n, shape[3], shape[4]), generator=generator, device=dev, dtype=dtype)
        if noise_type == "random":
            return latents
    elif latents.shape[2] == num_frames:
        return latents
    elif latents.shape[2] != L:
        raise ValueError(f"latents hold {latents.shape[2]} frames, expected {num_frames} or {L}")
    if latents.shape[2] < num_frames:
        latents = torch.cat([latents] * ((num_frames + L - 1) // L), dim=2)[:, :, :num_frames].contiguous()
    if noise_type == "shuffle_context":
        for i in range(L, num_frames, s):
            window_start = max(0, i - L)
            window_end = min(num_frames, window_start + s)
            window_length = window_end - window_start
            if window_length == 0:
                break
            indices = torch.arange(window_start, window_end, device=dev)
            shuffled = indices[torch.randperm(window_length, generator=generator, device=dev)]
            current_end = min(num_frames, i + window_length)
            latents[:, :, i:current_end] = latents[:, :, shuffled[:current_end - i].to(latents.device)]
    return latents
