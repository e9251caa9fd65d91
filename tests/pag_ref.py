"""Test infrastructure only.  Never imported by the product path.

Restatement of diffusers' perturbed-attention guidance (`PAGMixin` in pipelines/pag/pag_utils.py,
`PAGIdentitySelfAttnProcessor2_0` / `PAGCFGIdentitySelfAttnProcessor2_0` in
models/attention_processor.py, and the denoising loop of `AnimateDiffPAGPipeline`) in plain torch
ops on the CPU, on top of oracle/unet_ref.py and tests/controlnet_ref.py's UNet forward:

  * `select_layers`: `_set_pag_attn_processor`'s rule — a layer id is a regular expression searched
    in a module's name, self-attentions only, and an id ending in digits must not be followed by
    another digit in the name;
  * `get_pag_scale`: `_get_pag_scale`, with the clamp at 0 under adaptive scaling;
  * `identity_attention`: inside the block every selected self-attention of oracle.unet_ref returns
    to_out(to_v(x)) — the identity attention map — for ALL rows it is given.  The loops below run
    the unperturbed branches outside the block, exactly as the existing references do, and the
    perturbed branch inside it, so at pag_scale 0 they are the existing loops bit for bit;
  * `combine`: `_apply_perturbed_attention_guidance`, one fp32 torch op at a time in the device
    kernel's order: (e_u + g (e_c - e_u)) + s (e_c - e_p), or e_c + s (e_c - e_p) without CFG;
  * `step`: the four schedulers' updates from one coefficient row, one fp32 op at a time (the
    references of tests/lcm_ref.py and tests/dpm_ref.py for those two).

Parity to diffusers itself is UNPINNED: diffusers is not installed where this runs, so nothing
here was compared against it.  This restatement is the reference the device is held to.
"""
from __future__ import annotations

import contextlib
import functools
import re

import torch
import torch.nn.functional as F

import controlnet_ref as C
import dpm_ref
import lcm_ref
from oracle import ddim_ref
from oracle import unet_ref as U


# ---------------------------------------------------------------- layer selection
def select_layers(layer_ids, self_attention_names):
    """The names selected by a layer id or a list of them, in the order of the names."""
    layer_ids = [layer_ids] if isinstance(layer_ids, str) else list(layer_ids)
    picked = []
    for layer_id in layer_ids:
        hit = []
        for name in self_attention_names:
            for m in re.finditer(layer_id, name):
                follows = name[m.end():m.end() + 1]
                if layer_id[-1].isdigit() and follows.isdigit():
                    continue  # "down_blocks.1" inside "down_blocks.10": a fake integral match
                hit.append(name)
                break
        if not hit:
            raise ValueError(f"Cannot find PAG layer to set attention processor for: {layer_id}")
        picked += hit
    return [n for n in self_attention_names if n in set(picked)]


def self_attention_names(sd):
    """Every self-attention of a UNetMotionModel state dict: attn1 of the spatial transformer
    blocks (their attn2 reads the text), attn1 and attn2 of the motion modules."""
    names = sorted({k[:-len(".to_q.weight")] for k in sd if k.endswith(".to_q.weight")})
    return [n for n in names if n.endswith(".attn1") or ".motion_modules." in n]


# ---------------------------------------------------------------- the scale
def get_pag_scale(pag_scale, pag_adaptive_scale, t):
    """PAGMixin._get_pag_scale; do_pag_adaptive_scaling is pag_adaptive_scale > 0 (with
    pag_scale > 0 and layers set, which every caller here has)."""
    if pag_adaptive_scale > 0:
        signal_scale = pag_scale - pag_adaptive_scale * (1000 - t)
        if signal_scale < 0:
            signal_scale = 0
        return signal_scale
    return pag_scale


def scale_table(pag_scale, pag_adaptive_scale, timesteps):
    return torch.tensor([get_pag_scale(pag_scale, pag_adaptive_scale, float(t)) for t in timesteps],
                        dtype=torch.float64).float()


def do_perturbed_attention_guidance(pag_scale, pag_adaptive_scale, layers):
    return pag_scale > 0 and pag_adaptive_scale >= 0 and len(layers) > 0


# ---------------------------------------------------------------- the combine
def combine(branches, g, s):
    """branches: [e_u, e_c, e_p] (CFG) or [e_c, e_p]; g, s python floats or fp32 scalars."""
    g = torch.tensor(float(g), dtype=torch.float32)
    s = torch.as_tensor(s, dtype=torch.float32)
    if len(branches) == 3:
        e_u, e_c, e_p = (b.float() for b in branches)
        e = e_u + g * (e_c - e_u)
        return e + s * (e_c - e_p)
    e_c, e_p = (b.float() for b in branches)
    return e_c + s * (e_c - e_p)


# ---------------------------------------------------------------- the schedulers' updates from a row
def step(kind, e, x, row, m1=None, noise=None):
    """-> (prev_sample, the x0_out the kernel writes, the value packed into next_in)."""
    e, x = e.float(), x.float()
    if kind == "ddim":      # {sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev)}
        x0 = (x - row[1] * e) / row[0]
        xn = row[2] * x0 + row[3] * e
        return xn, x0, xn
    if kind == "euler":     # {sigma, sigma_next, sqrt(sigma_next^2 + 1), 0}
        x0 = x - row[0] * e
        d = (x - x0) / row[0]
        xn = x + d * (row[1] - row[0])
        return xn, x0, xn / row[2]
    if kind == "lcm":
        xn, den = lcm_ref.lcm_step(e, x, row, noise)
        return xn, den, xn
    if kind == "dpm":
        xn, x0 = dpm_ref.kernel_step(e, x, m1, row, noise)
        return xn, x0, xn
    raise ValueError(kind)


# ---------------------------------------------------------------- identity attention
@contextlib.contextmanager
def identity_attention(layers):
    """Inside the block oracle.unet_ref.attention of a self-attention named in `layers` is the
    identity attention map: to_out(to_v(x)) for every row (no q, no k, no softmax)."""
    layers = set(layers)
    saved = U.attention

    def attention(sd, p, x, ctx, heads, rnd=U._ident, fold_norm=None, pe=None):
        if ctx is not None or p not in layers:
            return saved(sd, p, x, ctx, heads, rnd, fold_norm=fold_norm, pe=pe)
        if fold_norm is not None:  # the device leaves the fold for the perturbed rows: norm, then the plain GEMM
            n = U.layer_norm(sd, fold_norm, x)
            if pe is not None:
                n = n + pe[:, : x.shape[1]]
            x = rnd(n)
        v = rnd(F.linear(x, sd[p + ".to_v.weight"]))
        return U.linear(sd, p + ".to_out.0", v)

    U.attention = attention
    try:
        yield
    finally:
        U.attention = saved


def perturbed_eps(usd, cfg, x, t, ehs_pos, layers, act="fp32"):
    """The perturbed branch: the UNet on (x, conditional text) with identity attention in `layers`."""
    with identity_attention(layers):
        return C.unet_forward_residuals(usd, cfg, x, t, ehs_pos, None, act)


def guided_eps(usd, cfg, x, t, ehs2, g, s, layers, act="fp32"):
    """One step's eps: ehs2 = [neg; pos].  The unperturbed branches exactly as the existing loops
    run them ([x; x] under CFG, x alone without), the perturbed branch on its own."""
    b = x.shape[0]
    pos = ehs2[-b:]
    if g > 1:
        u, c = C.unet_forward_residuals(usd, cfg, torch.cat([x, x]), t, ehs2, None, act).chunk(2)
        return combine([u, c, perturbed_eps(usd, cfg, x, t, pos, layers, act)], g, s)
    c = C.unet_forward_residuals(usd, cfg, x, t, pos, None, act)
    return combine([c, perturbed_eps(usd, cfg, x, t, pos, layers, act)], g, s)


def ddim_loop(usd, cfg, latents, ehs2, n_steps, g, pag_scale, pag_adaptive_scale, layers, act="fp32"):
    """AnimateDiffPAGPipeline's loop with the DDIM scheduler of oracle.ddim_ref."""
    acp = ddim_ref.alphas_cumprod()
    ts = ddim_ref.timesteps_leading(n_steps)
    tab = scale_table(pag_scale, pag_adaptive_scale, ts)
    x = latents.float()
    for i, t in enumerate(ts):
        e = guided_eps(usd, cfg, x, int(t), ehs2, g, tab[i], layers, act)
        x, _ = ddim_ref.ddim_step(e, int(t), x, n_steps, acp)
    return x


# ---------------------------------------------------------------- the shared case
DEFAULT_LAYERS = "mid_block.*attn1"
# The selected attentions' to_out weights are multiplied by this (exact in bf16).  A block's output
# is x + attention + ..., and with init_synthetic_'s weights the attention term is so small that
# identity attention moves a block's output by only ~2 x the bar of the device checks; at 8 the
# reference alone separates perturbed from unperturbed output by > 10 x that bar
# (tests/test_pag_host.py asserts it), as ZERO_CONV_STD was chosen in tests/controlnet_ref.py.
TO_OUT_GAIN = 8.0
BAR_FACTOR, BAR_CEILING = 3.0, 0.1  # tests/test_gpu_controlnet.py's module bar: 3 x the emulated deviation


@functools.lru_cache(maxsize=None)
def pag_case():
    """tests/controlnet_ref.py's tiny case (UNet seed 0, 2 frames of 8 x 8 latents, the golden text
    embeddings) with the default PAG layers' to_out scaled by TO_OUT_GAIN."""
    from vdiff import UNetMotionModel
    c = C.tiny_case()
    unet = UNetMotionModel("tiny")
    unet.load_state_dict(c["unet"].state_dict())
    names = self_attention_names(unet.state_dict())
    layers = select_layers(DEFAULT_LAYERS, names)
    with torch.no_grad():
        sd = unet.state_dict()
        for name in layers:
            sd[name + ".to_out.0.weight"].mul_(TO_OUT_GAIN)
    usd = {k: v.float() for k, v in unet.state_dict().items()}
    return dict(unet=unet, usd=usd, cfg=c["cfg"], lat=c["lat"], ehs=c["ehs"], names=names, layers=layers)


def block_case(kind, batch=3, frames=3, h=5, w=3, seed=7):
    """One mid-block layer of pag_case on random bf16-exact input: `kind` "spatial" (the
    Transformer2DModel) or "motion" (its motion module), `batch` videos whose LAST one is
    perturbed.  -> x (batch*frames, 128, h, w), ehs (batch, 77, 64), and for act in fp32 / bf16 the
    plain block's output and the block's output under identity attention, on every video."""
    c = pag_case()
    sd, cfg = c["usd"], c["cfg"]
    g = torch.Generator().manual_seed(seed)
    ch = cfg["block_out_channels"][-1]
    x = torch.randn(batch * frames, ch, h, w, generator=g).to(torch.bfloat16).float()
    ehs = torch.randn(batch, 77, cfg["cross_attention_dim"], generator=g).to(torch.bfloat16).float()

    def run(rnd):
        if kind == "spatial":
            return U.transformer2d(sd, "mid_block.attentions.0", x, ehs.repeat_interleave(frames, 0),
                                   cfg["num_attention_heads"], cfg["norm_num_groups"], rnd)
        return U.motion_module(sd, "mid_block.motion_modules.0", x, frames, cfg["motion_num_attention_heads"],
                               cfg["norm_num_groups"], cfg["motion_max_seq_length"], rnd)
    out = dict(x=x, ehs=ehs, frames=frames, batch=batch, h=h, w=w)
    with torch.no_grad():
        for act in ("fp32", "bf16"):
            out[f"plain_{act}"] = run(U.ROUNDERS[act])
            with identity_attention(c["layers"]):
                out[f"pert_{act}"] = run(U.ROUNDERS[act])
    k = (batch - 1) * frames  # images of the kept videos
    out["want"] = torch.cat([out["plain_fp32"][:k], out["pert_fp32"][k:]])
    emu = torch.cat([out["plain_bf16"][:k], out["pert_bf16"][k:]])
    out["emulated_kept"] = C.rel_l2(emu[:k], out["want"][:k])
    out["emulated_pert"] = C.rel_l2(emu[k:], out["want"][k:])
    out["bar_kept"] = BAR_FACTOR * out["emulated_kept"]
    out["bar_pert"] = BAR_FACTOR * out["emulated_pert"]
    # how far the reference alone moves the perturbed video's output
    out["separation"] = C.rel_l2(out["pert_fp32"][k:], out["plain_fp32"][k:])
    return out
