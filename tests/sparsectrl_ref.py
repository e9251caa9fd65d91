"""Test infrastructure only.  Never imported by the product path.

CPU restatement of diffusers' SparseControlNetModel (SparseCtrl, SD-1.5 + AnimateDiff tree), of
AnimateDiffSparseControlNetPipeline.prepare_sparse_control_conditioning as plain torch index
assignment, and of the pipeline's DDIM loop, composed from oracle/unet_ref.py's blocks and
tests/controlnet_ref.py's UNet-with-residuals.  Written from memory of
diffusers.models.controlnets.controlnet_sparsectrl; parity to diffusers itself is UNPINNED:
diffusers is not installed where this runs.

act: "fp32" (the reference semantics) or "bf16" (+ a bf16 rounding wherever the device stores an
activation), through unet_ref.ROUNDERS.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import controlnet_ref as R
from oracle import ddim_ref
from oracle import unet_ref as U

rel_l2 = R.rel_l2


# ---------------------------------------------------------------- the condition
def prepare_sparse_control_conditioning(key_frames, num_frames, indices):
    """key_frames (B, C, K, h, w), K >= len(indices) -> controlnet_cond (B, C, F, h, w) and
    conditioning_mask (B, 1, F, h, w): zeros, then `cond[:, :, i] = key_frames[:, :, k]` and
    `mask[:, :, i] = 1` for k, i in enumerate(indices) — assignments in order, the last one to a
    frame wins; negative indices the Python way, anything else an IndexError (torch's)."""
    b, c, k, h, w = key_frames.shape
    assert len(indices) <= k
    cond = torch.zeros(b, c, num_frames, h, w, dtype=key_frames.dtype)
    mask = torch.zeros(b, 1, num_frames, h, w, dtype=key_frames.dtype)
    for j, i in enumerate(indices):
        cond[:, :, i] = key_frames[:, :, j]
        mask[:, :, i] = 1
    return cond, mask


# ---------------------------------------------------------------- the ControlNet
def is_simplified(sd):
    return "controlnet_cond_embedding.weight" in sd


def cond_embedding(sd, x, rnd=U._ident, p="controlnet_cond_embedding"):
    """The conditioning embedding WITHOUT its last rounding (the device adds conv_in's bias in the
    same epilogue): one conv (simplified), or conv_in, the six blocks, conv_out with SiLU between."""
    x = rnd(x.float())
    if is_simplified(sd):
        return U.conv(sd, p, x)
    x = rnd(F.silu(U.conv(sd, f"{p}.conv_in", x)))
    i = 0
    while f"{p}.blocks.{i}.weight" in sd:
        x = rnd(F.silu(U.conv(sd, f"{p}.blocks.{i}", x, stride=1 + i % 2)))
        i += 1
    return U.conv(sd, f"{p}.conv_out", x)


def sparse_controlnet_forward(sd, cfg, sample, timestep, encoder_hidden_states, cond, mask, act="fp32"):
    """sample (B, C, F, H, W) — replaced by zeros —, encoder_hidden_states (B, L, D), cond
    (B, cc, F, h, w) and mask (B, 1, F, h, w) -> the UNSCALED zero-conv outputs
    [(B*F, C_i, h_i, w_i)]: one per UNet skip, then the mid one."""
    rnd = U.ROUNDERS[act]
    g, eps = cfg["norm_num_groups"], cfg["norm_eps"]
    heads, mheads, mlen = cfg["num_attention_heads"], cfg["motion_num_attention_heads"], cfg["motion_max_seq_length"]
    sample = torch.zeros_like(sample.float())
    b, _, nf, hh, ww = sample.shape
    t = torch.as_tensor(timestep)
    t = (t[None] if t.ndim == 0 else t).expand(b)
    temb = rnd(U.timestep_embedding(t, cfg["block_out_channels"][0]))
    temb = rnd(F.silu(U.linear(sd, "time_embedding.linear_1", temb)))
    temb = U.linear(sd, "time_embedding.linear_2", temb)
    temb_silu = rnd(F.silu(temb)).repeat_interleave(nf, 0)
    ehs = rnd(encoder_hidden_states.float()).repeat_interleave(nf, 0)
    both = torch.cat([cond.float(), mask.float()], dim=1)
    both = both.permute(0, 2, 1, 3, 4).reshape(b * nf, both.shape[1], both.shape[3], both.shape[4])
    x = sample.permute(0, 2, 1, 3, 4).reshape(b * nf, -1, hh, ww)
    x = rnd(U.conv(sd, "conv_in", x) + cond_embedding(sd, both, rnd))
    assert tuple(x.shape[2:]) == (hh, ww)
    outs = [x]
    for i, (ins, has_attn, down) in enumerate(U._down_plan(cfg)):
        for j in range(len(ins)):
            p = f"down_blocks.{i}"
            x = U.resnet(sd, f"{p}.resnets.{j}", x, temb_silu, g, eps, rnd)
            if has_attn:
                x = U.transformer2d(sd, f"{p}.attentions.{j}", x, ehs, heads, g, rnd)
            x = U.motion_module(sd, f"{p}.motion_modules.{j}", x, nf, mheads, g, mlen, rnd)
            outs.append(x)
        if down:
            x = rnd(U.conv(sd, f"down_blocks.{i}.downsamplers.0.conv", x, stride=2, padding=1))
            outs.append(x)
    x = U.resnet(sd, "mid_block.resnets.0", x, temb_silu, g, eps, rnd)
    x = U.transformer2d(sd, "mid_block.attentions.0", x, ehs, heads, g, rnd)
    x = U.resnet(sd, "mid_block.resnets.1", x, temb_silu, g, eps, rnd)
    res = [rnd(U.conv(sd, f"controlnet_down_blocks.{i}", o, padding=0)) for i, o in enumerate(outs)]
    return res + [rnd(U.conv(sd, "controlnet_mid_block", x, padding=0))]


def scale_row(n_res, scale=1.0, guess_mode=False):
    """The sparse pipeline's scales of one step (every step's: there is no guidance window)."""
    return (R.guess_scales(n_res) * scale if guess_mode else torch.full((n_res,), float(scale))).float()


# ---------------------------------------------------------------- the pipeline's step
def controlled_eps(usd, csd, cfg, ccfg, x_in, t, ehs2, cond, mask, scales, guess_mode, act="fp32"):
    """One step's eps for x_in = [x; x] (CFG, uncond first): the sparse ControlNet on both halves —
    on the conditional half alone in guess mode, the unconditional half's residuals then zero —
    its outputs times `scales` into the UNet (tests/controlnet_ref.py)."""
    b2 = x_in.shape[0]
    if guess_mode:
        h = b2 // 2
        res = sparse_controlnet_forward(csd, ccfg, x_in[h:], t, ehs2[h:], cond, mask, act)
        res = [torch.cat([torch.zeros_like(r), r]) for r in res]
    else:
        res = sparse_controlnet_forward(csd, ccfg, x_in, t, ehs2, torch.cat([cond, cond]), torch.cat([mask, mask]), act)
    res = [float(s) * r for s, r in zip(scales, res)]
    return R.unet_forward_residuals(usd, cfg, x_in, t, ehs2, res, act, given=False)


def ddim_loop(usd, csd, cfg, ccfg, latents, ehs2, cond, mask, scales, guess_mode, n_steps, guidance, act="fp32"):
    """The DDIM pipeline loop (oracle.ddim_ref.denoise_loop) with the same scales at every step."""
    acp = ddim_ref.alphas_cumprod()
    x = latents.float()
    for t in ddim_ref.timesteps_leading(n_steps):
        eps = controlled_eps(usd, csd, cfg, ccfg, torch.cat([x, x]), int(t), ehs2, cond, mask, scales, guess_mode, act)
        x, _ = ddim_ref.ddim_step(ddim_ref.cfg_combine(eps, guidance), int(t), x, n_steps, acp)
    return x


# ---------------------------------------------------------------- random weights and the shared case
def random_sparse_controlnet(config="tiny", seed=1, simplified=True, zero_conv_std=R.ZERO_CONV_STD):
    """A vdiff.SparseControlNetModel on the CPU with init_synthetic_'s weights; simplified=False is
    the scribble variant (3 conditioning channels, the eight-conv embedding).  The zero convs are
    redrawn with zero_conv_std, as tests/controlnet_ref.py's random_controlnet does."""
    from vdiff import SparseControlNetModel, init_synthetic_
    extra = {} if simplified else dict(use_simplified_condition_embedding=False, conditioning_channels=3)
    m = init_synthetic_(SparseControlNetModel(config, **extra), seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for z in [*m.controlnet_down_blocks, m.controlnet_mid_block]:
            z.weight.copy_((torch.randn(z.weight.shape, generator=g) * zero_conv_std).to(torch.bfloat16).float())
    return m


NF, IDX = 4, [0, 3]


@functools.lru_cache(maxsize=None)
def tiny_case():
    """The tests' one case, computed once per process: the tiny UNet (seed 0), the tiny sparse
    ControlNets (seed 1 simplified, seed 2 full embedding), the golden latents cut to 4 frames x
    8 x 8 as two videos [lat; lat], the golden text embeddings (uncond, cond), two key frames per
    video at frames [0, 3] — 4 x 8 x 8 latents and 3 x 64 x 64 images — and at t = 961 each
    ControlNet's residuals in fp32 and bf16-emulating arithmetic."""
    from vdiff import UNetMotionModel, init_synthetic_
    from vdiff.config import TINY
    unet = init_synthetic_(UNetMotionModel("tiny"), seed=0)
    usd = {k: v.float() for k, v in unet.state_dict().items()}
    g = np.load(R.GOLD / "tiny_unet.npz")
    lat = torch.from_numpy(g["latents"])[:, :, :NF, :8, :8].contiguous()
    assert lat.shape[2] == NF
    ehs = torch.from_numpy(g["ehs"])
    gen = torch.Generator().manual_seed(7)
    c = dict(unet=unet, usd=usd, cfg=TINY, lat=lat, ehs=ehs, x2=torch.cat([lat, lat]), t=961)
    keys = {True: torch.randn(2, 4, 2, 8, 8, generator=gen), False: torch.rand(2, 3, 2, 64, 64, generator=gen)}
    for simplified in (True, False):
        m = random_sparse_controlnet("tiny", seed=1 if simplified else 2, simplified=simplified)
        sd = {k: v.float() for k, v in m.state_dict().items()}
        cond, mask = prepare_sparse_control_conditioning(keys[simplified], NF, IDX)
        v = dict(cnet=m, csd=sd, ccfg=dict(m.config), keys=keys[simplified], cond=cond, mask=mask)
        with torch.no_grad():
            for act in ("fp32", "bf16"):
                v[f"res_{act}"] = sparse_controlnet_forward(sd, v["ccfg"], c["x2"], 961, ehs, cond, mask, act)
        c[simplified] = v
    with torch.no_grad():
        out = {act: R.unet_forward_residuals(usd, TINY, c["x2"], 961, ehs, None, act) for act in ("fp32", "bf16")}
    c["unet_emulated"] = rel_l2(out["bf16"], out["fp32"])
    c["unet_bar"] = 1.3 * c["unet_emulated"]
    return c
