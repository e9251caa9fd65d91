"""Test infrastructure only.  Never imported by the product path.

CPU restatement of diffusers' ControlNetModel (SD-1.5 tree) and of UNetMotionModel.forward with
`down_block_additional_residuals` / `mid_block_additional_residual`, composed from
oracle/unet_ref.py's blocks, plus the AnimateDiffControlNetPipeline loop around them (DDIM and
LCM).  Parity to diffusers itself is UNPINNED: diffusers is not installed where this runs.

act: "fp32" (the reference semantics) or "bf16" (+ a bf16 rounding wherever the device stores an
activation), through unet_ref.ROUNDERS.
"""
from __future__ import annotations

import contextlib
import functools
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

import lcm_ref
from oracle import ddim_ref
from oracle import unet_ref as U

GOLD = Path(__file__).resolve().parent / "golden"


# ---------------------------------------------------------------- the ControlNet
def cond_embedding(sd, cond, rnd=U._ident, p="controlnet_cond_embedding"):
    """ControlNetConditioningEmbedding: (N, 3, H, W) in [0, 1] -> (N, C0, H/8, W/8)."""
    x = rnd(F.silu(U.conv(sd, f"{p}.conv_in", rnd(cond.float()))))
    i = 0
    while f"{p}.blocks.{i}.weight" in sd:
        x = rnd(F.silu(U.conv(sd, f"{p}.blocks.{i}", x, stride=1 + i % 2)))
        i += 1
    return rnd(U.conv(sd, f"{p}.conv_out", x))


def controlnet_forward(sd, cfg, sample, timestep, encoder_hidden_states, cond, act="fp32"):
    """sample (B, C, F, H, W), encoder_hidden_states (B, L, D), cond (B, 3, F, 8H, 8W) in [0, 1]
    -> the UNSCALED zero-conv outputs [(B*F, C_i, h_i, w_i)]: one per UNet skip, then the mid one."""
    rnd = U.ROUNDERS[act]
    g, eps, heads = cfg["norm_num_groups"], cfg["norm_eps"], cfg["num_attention_heads"]
    sample = sample.float()
    b, _, nf, hh, ww = sample.shape
    t = torch.as_tensor(timestep)
    t = (t[None] if t.ndim == 0 else t).expand(b)
    temb = rnd(U.timestep_embedding(t, cfg["block_out_channels"][0]))
    temb = rnd(F.silu(U.linear(sd, "time_embedding.linear_1", temb)))
    temb = U.linear(sd, "time_embedding.linear_2", temb)
    temb_silu = rnd(F.silu(temb)).repeat_interleave(nf, 0)
    ehs = rnd(encoder_hidden_states.float()).repeat_interleave(nf, 0)
    emb = cond_embedding(sd, cond.permute(0, 2, 1, 3, 4).reshape(b * nf, -1, 8 * hh, 8 * ww), rnd)
    x = rnd(sample).permute(0, 2, 1, 3, 4).reshape(b * nf, -1, hh, ww)
    x = rnd(U.conv(sd, "conv_in", x) + emb)
    outs = [x]
    for i, (ins, has_attn, down) in enumerate(U._down_plan(cfg)):
        for j in range(len(ins)):
            x = U.resnet(sd, f"down_blocks.{i}.resnets.{j}", x, temb_silu, g, eps, rnd)
            if has_attn:
                x = U.transformer2d(sd, f"down_blocks.{i}.attentions.{j}", x, ehs, heads, g, rnd)
            outs.append(x)
        if down:
            x = rnd(U.conv(sd, f"down_blocks.{i}.downsamplers.0.conv", x, stride=2, padding=1))
            outs.append(x)
    x = U.resnet(sd, "mid_block.resnets.0", x, temb_silu, g, eps, rnd)
    x = U.transformer2d(sd, "mid_block.attentions.0", x, ehs, heads, g, rnd)
    x = U.resnet(sd, "mid_block.resnets.1", x, temb_silu, g, eps, rnd)
    res = [rnd(U.conv(sd, f"controlnet_down_blocks.{i}", o, padding=0)) for i, o in enumerate(outs)]
    return res + [rnd(U.conv(sd, "controlnet_mid_block", x, padding=0))]


def guess_scales(n):
    return torch.logspace(-1, 0, n)


def scale_table(n_steps, n_res, scale=1.0, guess_mode=False, start=0.0, end=1.0):
    """diffusers' rule, written by hand: controlnet_keep[i] = 1 - float(i / n < start or
    (i + 1) / n > end); cond_scale = scale * keep; guess mode multiplies by logspace(-1, 0, n_res)."""
    rows = []
    for i in range(n_steps):
        keep = 1.0 - float(i / n_steps < start or (i + 1) / n_steps > end)
        s = scale * keep
        # diffusers: scales = torch.logspace(-1, 0, n) * conditioning_scale, an fp32 tensor product
        rows.append(guess_scales(n_res) * s if guess_mode else torch.full((n_res,), s))
    return torch.stack(rows).float()


# ---------------------------------------------------------------- the UNet with residuals
@contextlib.contextmanager
def module_rounding():
    """Inside the block oracle.unet_ref's leaf primitives round their outputs to bf16, as the
    hooked module path does (every module's output is a bf16 tensor there), except the two the
    device keeps wider: conv_out (fp32 eps) and the GEGLU projection (gelu and product are its
    GEMM's epilogue).  With act="bf16" on top this is the module path's emulation."""
    names = ("conv", "linear", "group_norm", "layer_norm")
    saved = {n: getattr(U, n) for n in names}

    def wrap(fn):
        def f(sd, p, *a, **k):
            out = fn(sd, p, *a, **k)
            return out if p == "conv_out" or p.endswith(".net.0.proj") else U._bf16_round(out)
        return f

    for n in names:
        setattr(U, n, wrap(saved[n]))
    try:
        yield
    finally:
        for n in names:
            setattr(U, n, saved[n])


def unet_forward_residuals(sd, cfg, sample, timestep, encoder_hidden_states, residuals=None, act="fp32",
                           return_skips=False, given=True):
    """oracle.unet_ref.unet_forward with diffusers' two residual arguments: `residuals` =
    [down residuals..., mid residual] as (B*F, C, h, w) maps, ALREADY scaled, added to the skips
    after the last down block and to the mid block's output.  return_skips: also the skips and
    the mid output before the addition.  act "bf16-modules": "bf16" under module_rounding().
    given=False (the denoising loop): the scaled residual is never stored, scale and add are one
    fused multiply-add with one rounding."""
    if act == "bf16-modules":
        with module_rounding():
            return unet_forward_residuals(sd, cfg, sample, timestep, encoder_hidden_states, residuals, "bf16",
                                          return_skips, given)
    rnd = U.ROUNDERS[act]
    rres = rnd if given else U._ident
    g, eps = cfg["norm_num_groups"], cfg["norm_eps"]
    heads, mheads, mlen = cfg["num_attention_heads"], cfg["motion_num_attention_heads"], cfg["motion_max_seq_length"]
    sample = sample.float()
    b, _, nf, hh, ww = sample.shape
    t = torch.as_tensor(timestep)
    t = (t[None] if t.ndim == 0 else t).expand(b)
    temb = rnd(U.timestep_embedding(t, cfg["block_out_channels"][0]))
    temb = rnd(F.silu(U.linear(sd, "time_embedding.linear_1", temb)))
    temb = U.linear(sd, "time_embedding.linear_2", temb)
    temb_silu = rnd(F.silu(temb)).repeat_interleave(nf, 0)
    ehs = rnd(encoder_hidden_states.float()).repeat_interleave(nf, 0)
    x = rnd(sample).permute(0, 2, 1, 3, 4).reshape(b * nf, -1, hh, ww)
    x = rnd(U.conv(sd, "conv_in", x))
    skips = [x]
    for i, (ins, has_attn, down) in enumerate(U._down_plan(cfg)):
        for j in range(len(ins)):
            p = f"down_blocks.{i}"
            x = U.resnet(sd, f"{p}.resnets.{j}", x, temb_silu, g, eps, rnd)
            if has_attn:
                x = U.transformer2d(sd, f"{p}.attentions.{j}", x, ehs, heads, g, rnd)
            x = U.motion_module(sd, f"{p}.motion_modules.{j}", x, nf, mheads, g, mlen, rnd)
            skips.append(x)
        if down:
            x = rnd(U.conv(sd, f"down_blocks.{i}.downsamplers.0.conv", x, stride=2, padding=1))
            skips.append(x)
    x = U.resnet(sd, "mid_block.resnets.0", x, temb_silu, g, eps, rnd)
    x = U.transformer2d(sd, "mid_block.attentions.0", x, ehs, heads, g, rnd)
    if cfg.get("use_motion_mid_block", True):
        x = U.motion_module(sd, "mid_block.motion_modules.0", x, nf, mheads, g, mlen, rnd)
    x = U.resnet(sd, "mid_block.resnets.1", x, temb_silu, g, eps, rnd)
    plain = list(skips) + [x]
    if residuals is not None:
        assert len(residuals) == len(skips) + 1, (len(residuals), len(skips))
        skips = [rnd(s + rres(r.float())) for s, r in zip(skips, residuals[:-1])]
        x = rnd(x + rres(residuals[-1].float()))
    for i, (ins, has_attn, up) in enumerate(U._up_plan(cfg)):
        p = f"up_blocks.{i}"
        for j in range(len(ins)):
            x = torch.cat([x, skips.pop()], dim=1)
            x = U.resnet(sd, f"{p}.resnets.{j}", x, temb_silu, g, eps, rnd)
            if has_attn:
                x = U.transformer2d(sd, f"{p}.attentions.{j}", x, ehs, heads, g, rnd)
            x = U.motion_module(sd, f"{p}.motion_modules.{j}", x, nf, mheads, g, mlen, rnd)
        if up:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = rnd(U.conv(sd, f"{p}.upsamplers.0.conv", x))
    x = rnd(F.silu(U.group_norm(sd, "conv_norm_out", x, g, eps)))
    x = U.conv(sd, "conv_out", x)
    out = x.reshape(b, nf, -1, hh, ww).permute(0, 2, 1, 3, 4).contiguous()
    return (out, plain) if return_skips else out


# ---------------------------------------------------------------- the pipeline's step
def controlled_eps(usd, csd, cfg, ccfg, x_in, t, ehs2, cond, scales, guess_mode, act="fp32"):
    """One step's eps of the ControlNet pipeline for x_in = [x; x] (CFG, uncond first): the
    ControlNet on both halves — on the conditional half alone in guess mode, the unconditional
    half's residuals then zero — its outputs times `scales` (one per residual) into the UNet."""
    b2 = x_in.shape[0]
    cond2 = torch.cat([cond, cond]) if cond.shape[0] * 2 == b2 else cond
    if guess_mode and cond.shape[0] * 2 == b2:
        h = b2 // 2
        res = controlnet_forward(csd, ccfg, x_in[h:], t, ehs2[h:], cond, act)
        nf = x_in.shape[2]
        res = [torch.cat([torch.zeros_like(r), r]) for r in res]  # rows (video, frame): uncond videos first
        assert res[0].shape[0] == b2 * nf
    else:
        res = controlnet_forward(csd, ccfg, x_in, t, ehs2, cond2, act)
    res = [float(s) * r for s, r in zip(scales, res)]
    return unet_forward_residuals(usd, cfg, x_in, t, ehs2, res, act, given=False)


def ddim_loop(usd, csd, cfg, ccfg, latents, ehs2, cond, table, guess_mode, n_steps, guidance, act="fp32"):
    """The DDIM pipeline loop (oracle.ddim_ref.denoise_loop) with step i's row of `table`."""
    acp = ddim_ref.alphas_cumprod()
    ts = ddim_ref.timesteps_leading(n_steps)
    x = latents.float()
    for i, t in enumerate(ts):
        eps = controlled_eps(usd, csd, cfg, ccfg, torch.cat([x, x]), int(t), ehs2, cond, table[i], guess_mode, act)
        x, _ = ddim_ref.ddim_step(ddim_ref.cfg_combine(eps, guidance), int(t), x, n_steps, acp)
    return x


def lcm_loop(usd, csd, cfg, ccfg, latents, ehs2, cond, table, guess_mode, n_steps, guidance, noise, act="fp32"):
    """The LCM pipeline loop (tests/lcm_ref.py), beta_schedule "linear"; noise [n_steps - 1, ...]."""
    acp = lcm_ref.alphas_cumprod(schedule="linear")
    ts = lcm_ref.lcm_timesteps(n_steps)
    x = latents.float()
    for i, t in enumerate(ts):
        eps = controlled_eps(usd, csd, cfg, ccfg, torch.cat([x, x]), int(t), ehs2, cond, table[i], guess_mode, act)
        u, c = eps.chunk(2)
        x, _ = lcm_ref.lcm_step(lcm_ref.cfg_combine(u, c, guidance), x, lcm_ref.row(ts, i, acp),
                                noise[i] if i < n_steps - 1 else None)
    return x


# ---------------------------------------------------------------- random weights and the shared case
ZERO_CONV_STD = 0.06  # the "zero" convs' weights: large enough that every residual matters (see tiny_case)


def random_controlnet(config="tiny", seed=1, zero_conv_std=ZERO_CONV_STD):
    """A vdiff.ControlNetModel on the CPU with init_synthetic_'s weights; the zero convs — zero in
    a freshly initialised ControlNet, which would make every test blind — are redrawn with
    zero_conv_std, rounded to bf16 once like every other weight."""
    from vdiff import ControlNetModel, init_synthetic_
    m = init_synthetic_(ControlNetModel(config), seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for z in [*m.controlnet_down_blocks, m.controlnet_mid_block]:
            z.weight.copy_((torch.randn(z.weight.shape, generator=g) * zero_conv_std).to(torch.bfloat16).float())
    return m


def rel_l2(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).norm() / want.norm()).item()


@functools.lru_cache(maxsize=None)
def tiny_case():
    """The tests' one case, computed once per process: the tiny UNet (seed 0) and ControlNet
    (seed 1), the golden latents cut to 2 frames x 8 x 8, the golden text embeddings (uncond,
    cond), 64 x 64 conditioning frames, and at t = 961 on x2 = [lat; lat]: the ControlNet's
    residuals and the UNet's output with them, in fp32 and bf16-emulating arithmetic."""
    from vdiff import UNetMotionModel, init_synthetic_
    from vdiff.config import TINY
    from vdiff.models.controlnet import controlnet_config
    unet = init_synthetic_(UNetMotionModel("tiny"), seed=0)
    cnet = random_controlnet("tiny", seed=1)
    usd = {k: v.float() for k, v in unet.state_dict().items()}
    csd = {k: v.float() for k, v in cnet.state_dict().items()}
    g = np.load(GOLD / "tiny_unet.npz")
    lat = torch.from_numpy(g["latents"])[:, :, :2, :8, :8].contiguous()
    ehs = torch.from_numpy(g["ehs"])
    cond = torch.rand(1, 3, 2, 64, 64, generator=torch.Generator().manual_seed(5))
    x2, cond2 = torch.cat([lat, lat]), torch.cat([cond, cond])
    ccfg = controlnet_config("tiny")
    c = dict(unet=unet, cnet=cnet, usd=usd, csd=csd, cfg=TINY, ccfg=ccfg, lat=lat, ehs=ehs, cond=cond, x2=x2,
             cond2=cond2, t=961)
    with torch.no_grad():
        for act in ("fp32", "bf16"):
            c[f"res_{act}"] = controlnet_forward(csd, ccfg, x2, 961, ehs, cond2, act)
        # the UNet tests take the fp32 residuals as GIVEN inputs (rounded to bf16, as a caller hands them over)
        c["given"] = [r.to(torch.bfloat16) for r in c["res_fp32"]]
        for act in ("fp32", "bf16"):
            c[f"out_{act}"], c[f"skips_{act}"] = unet_forward_residuals(usd, TINY, x2, 961, ehs, c["given"], act,
                                                                         return_skips=True)
        c["out_plain"] = unet_forward_residuals(usd, TINY, x2, 961, ehs, None, "fp32")
        c["out_bf16m"] = unet_forward_residuals(usd, TINY, x2, 961, ehs, c["given"], "bf16-modules")
    # the bars of the UNet-with-residuals checks: 1.3 x the bf16-emulating restatement's own rel-L2,
    # the fast path's and the hooked module path's (which rounds every module's output)
    c["unet_emulated"] = rel_l2(c["out_bf16"], c["out_fp32"])
    c["unet_bar"] = 1.3 * c["unet_emulated"]
    c["unet_emulated_modules"] = rel_l2(c["out_bf16m"], c["out_fp32"])
    c["unet_bar_modules"] = 1.3 * c["unet_emulated_modules"]
    return c
