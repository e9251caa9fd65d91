"""Test infrastructure only: random LoRAs for the tiny UNet, the four key layouts they are written
in, and the offline merge W0 + sum_a w_a * (alpha / r) * (B . A) in fp64, rounded once.  The key
layouts restate what diffusers' loaders accept from memory of its converters (unpinned)."""
from __future__ import annotations

import torch

# one of each target the GPU test asks for, and a few more
SPATIAL = "down_blocks.0.attentions.0.transformer_blocks.0."
MOTION = "down_blocks.0.motion_modules.0.transformer_blocks.0."
MODULES = (
    SPATIAL + "attn1.to_q", SPATIAL + "attn1.to_out.0",           # spatial self-attention
    SPATIAL + "attn2.to_k", SPATIAL + "attn2.to_v",               # cross-attention
    SPATIAL + "ff.net.0.proj", SPATIAL + "ff.net.2",              # GEGLU, ff.net.2
    "down_blocks.0.attentions.0.proj_in",                         # 1x1 conv
    MOTION + "attn1.to_q", MOTION + "attn2.to_out.0",             # motion-module attention
    "mid_block.motion_modules.0.transformer_blocks.0.attn1.to_v",
    "down_blocks.0.resnets.0.conv1", "up_blocks.1.resnets.0.conv2",  # 3x3 convs
    "mid_block.resnets.0.time_emb_proj",
    "down_blocks.0.downsamplers.0.conv", "up_blocks.0.upsamplers.0.conv",
)
MOTION_ATTN = tuple(m for m in MODULES if ".motion_modules." in m)


def make_lora(unet, modules=MODULES, r=4, alpha=2.0, seed=0, std=0.05):
    """{module: (A, B, alpha)}: fp32 on the CPU, A [r, in(, k, k)], B [out, r(, 1, 1)]."""
    g = torch.Generator().manual_seed(seed)
    mods = dict(unet.named_modules())
    out = {}
    for name in modules:
        w = mods[name].weight
        if w.dim() == 4:
            A = torch.randn((r,) + tuple(w.shape[1:]), generator=g) * std
            B = torch.randn((w.shape[0], r, 1, 1), generator=g) * std
        else:
            A = torch.randn(r, w.shape[1], generator=g) * std
            B = torch.randn(w.shape[0], r, generator=g) * std
        out[name] = (A, B, alpha)
    return out


def write_peft(lora, alpha=True):
    sd = {}
    for m, (A, B, al) in lora.items():
        sd[f"unet.{m}.lora_A.weight"], sd[f"unet.{m}.lora_B.weight"] = A, B
        if alpha:
            sd[f"unet.{m}.alpha"] = torch.tensor(al)
    return sd


def write_legacy(lora):
    """<module>.lora.down / .up; attention projections in the processor form."""
    sd = {}
    for m, (A, B, al) in lora.items():
        head, _, leaf = m.rpartition(".")
        if m.endswith(".to_out.0"):
            stem = m[:-len(".to_out.0")] + ".processor.to_out_lora"
        elif leaf in ("to_q", "to_k", "to_v"):
            stem = f"{head}.processor.{leaf}_lora"
        else:
            stem = f"unet.{m}.lora"
        sd[f"{stem}.down.weight"], sd[f"{stem}.up.weight"] = A, B
        sd[f"unet.{m}.alpha"] = torch.tensor(al)
    return sd


def write_kohya(lora):
    sd = {}
    for m, (A, B, al) in lora.items():
        k = "lora_unet_" + m.replace(".", "_")
        sd[f"{k}.lora_down.weight"], sd[f"{k}.lora_up.weight"], sd[f"{k}.alpha"] = A, B, torch.tensor(al)
    return sd


def write_motion(lora):
    """The original motion-LoRA names (motion-module attention projections only); no alpha key
    exists in that layout, so the LoRA must have alpha == r."""
    sd = {}
    for m, (A, B, al) in lora.items():
        assert ".motion_modules." in m and al == A.shape[0]
        head, attn, leaf = m.replace(".to_out.0", ".to_out").rsplit(".", 2)
        head = head.replace(".transformer_blocks.", ".temporal_transformer.transformer_blocks.")
        stem = f"{head}.attention_blocks.{int(attn[4:]) - 1}.processor.{leaf}_lora"
        sd[f"{stem}.down.weight"], sd[f"{stem}.up.weight"] = A, B
    return sd


def delta64(A, B, shape):
    return (B.flatten(1).double() @ A.flatten(1).double()).reshape(shape)


def merged_state_dict(base_sd, loras_and_weights):
    """base_sd with every touched weight replaced by the fp64 merge rounded once to its dtype."""
    sd = {k: v.clone() for k, v in base_sd.items()}
    touched = {m for lora, _ in loras_and_weights for m in lora}
    for m in touched:
        w0 = base_sd[m + ".weight"]
        acc = w0.double().cpu()
        for lora, wt in loras_and_weights:
            if m in lora:
                A, B, al = lora[m]
                acc = acc + (wt * (al / A.shape[0])) * delta64(A, B, w0.shape)
        sd[m + ".weight"] = acc.to(w0.dtype).to(w0.device)
    return sd
