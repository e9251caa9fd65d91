"""Local diffusers-layout checkpoints: `MotionAdapter.from_pretrained` and
`AnimateDiffPipeline.from_pretrained` as the reference calls them
(experiments/05_grid_search_ablation.py:121-147, also 01:60-75, 02:17-30, 03:39-50):

    adapter = MotionAdapter.from_pretrained(<adapter dir>, torch_dtype=...)
    pipe = AnimateDiffPipeline.from_pretrained(<sd-1.5 dir>, motion_adapter=adapter, torch_dtype=...)
    pipe.scheduler = DDIMScheduler.from_config(pipe.scheduler.config, beta_schedule="linear", ...)

There is no network here, so the model names of the reference become local directory paths
with diffusers' own layout: `<adapter>/config.json` + `diffusion_pytorch_model[.<variant>].
safetensors` (or a `.safetensors.index.json` shard index); `<pipe>/unet/`, `<pipe>/vae/` (same
files) and `<pipe>/scheduler/scheduler_config.json`.  The UNet checkpoint holds the SD-1.5
UNet2DConditionModel keys and the adapter the `*.motion_modules.*` keys; diffusers'
UNetMotionModel.from_unet2d joins the two under exactly those names, which are the names of
vdiff.UNetMotionModel's parameters, so the join is a dict union.  The adapter's
`pos_embed.pe` buffers are recomputed (they are fixed sinusoids).  The VAE's encoder half
(`encoder.*`, `quant_conv.*`) is not on the text-to-video path: it is built when the checkpoint
holds every one of its tensors (the video-to-video pipeline needs it) and skipped otherwise.
Weights are
stored in bf16 on the device: the kernels compute in bf16, whatever `torch_dtype` the caller
passes (the reference's float16 is recorded in `.torch_dtype`).
"""
from __future__ import annotations

import json
from pathlib import Path

import torch

from .config import get_config

WEIGHTS_NAME = "diffusion_pytorch_model"
_DOWN = {"CrossAttnDownBlock2D": "CrossAttnDownBlockMotion", "DownBlock2D": "DownBlockMotion",
         "CrossAttnDownBlockMotion": "CrossAttnDownBlockMotion", "DownBlockMotion": "DownBlockMotion"}
_UP = {"CrossAttnUpBlock2D": "CrossAttnUpBlockMotion", "UpBlock2D": "UpBlockMotion",
       "CrossAttnUpBlockMotion": "CrossAttnUpBlockMotion", "UpBlockMotion": "UpBlockMotion"}


def _local_dir(path, what: str) -> Path:
    p = Path(path)
    if not p.is_dir():
        raise FileNotFoundError(f"{what}: {path!r} is not a local directory (hub checkpoints are "
                                "unreachable offline: pass a diffusers-layout directory)")
    return p


def read_json(path: Path) -> dict:
    with open(path) as f:
        return json.load(f)


def load_weights(folder: Path, variant=None) -> dict:
    """All tensors of a diffusers model folder: `diffusion_pytorch_model[.variant].safetensors`
    or its sharded form (`….safetensors.index.json` naming the shard files)."""
    from safetensors.torch import load_file

    stem = WEIGHTS_NAME + (f".{variant}" if variant else "")
    single = folder / f"{stem}.safetensors"
    index = folder / f"{stem}.safetensors.index.json"
    if single.exists():
        return load_file(str(single))
    if index.exists():
        sd = {}
        for shard in sorted(set(read_json(index)["weight_map"].values())):
            sd.update(load_file(str(folder / shard)))
        return sd
    raise FileNotFoundError(f"no {stem}.safetensors (or its .index.json) in {folder}")


class MotionAdapter:
    """diffusers.MotionAdapter as the reference uses it: a config plus the motion-module weights
    (`down_blocks.i.motion_modules.j.*`, `up_blocks.i.motion_modules.j.*`,
    `mid_block.motion_modules.0.*`) that AnimateDiffPipeline.from_pretrained joins to the UNet."""

    def __init__(self, config: dict, state_dict: dict, torch_dtype=None):
        self.config = dict(config)
        self.torch_dtype = torch_dtype
        self._state = {k: v for k, v in state_dict.items() if not k.endswith(".pos_embed.pe")}
        bad = [k for k in self._state if ".motion_modules." not in k]
        if bad:
            raise KeyError(f"not motion-module keys: {bad[:4]}")

    @classmethod
    def from_pretrained(cls, path, torch_dtype=None, variant=None, **unused):
        d = _local_dir(path, "MotionAdapter.from_pretrained")
        return cls(read_json(d / "config.json"), load_weights(d, variant), torch_dtype)

    def state_dict(self) -> dict:
        return dict(self._state)


def motion_unet_config(unet_cfg: dict, adapter_cfg: dict) -> dict:
    """diffusers UNet2DConditionModel config.json + MotionAdapter config.json -> the
    vdiff.UNetMotionModel config (what UNetMotionModel.from_unet2d builds)."""
    boc = tuple(unet_cfg["block_out_channels"])
    heads = unet_cfg.get("num_attention_heads") or unet_cfg.get("attention_head_dim", 8)  # diffusers' legacy name
    if isinstance(heads, (list, tuple)):
        if len(set(heads)) != 1:
            raise NotImplementedError(f"per-block attention heads {heads}")
        heads = heads[0]
    lpb = unet_cfg.get("layers_per_block", 2)
    if isinstance(lpb, (list, tuple)):
        raise NotImplementedError("per-block layers_per_block")
    if tuple(adapter_cfg.get("block_out_channels", boc)) != boc:
        raise ValueError("motion adapter block_out_channels differ from the UNet's")
    if adapter_cfg.get("motion_layers_per_block", lpb) != lpb:
        raise NotImplementedError("motion_layers_per_block != the UNet's layers_per_block")
    if adapter_cfg.get("motion_norm_num_groups", unet_cfg.get("norm_num_groups", 32)) != unet_cfg.get("norm_num_groups", 32):
        raise NotImplementedError("motion_norm_num_groups != norm_num_groups")
    if unet_cfg.get("time_cond_proj_dim"):
        raise NotImplementedError("time_cond_proj_dim (the guidance-scale embedding of a fully distilled LCM UNet) is "
                                  "not built: load the base UNet and the LCM LoRA (pipe.load_lora_weights)")
    if adapter_cfg.get("conv_in_channels"):
        raise NotImplementedError("motion adapters with their own conv_in (PIA / SparseCtrl) are not on 05's path")
    cfg = get_config("full")
    cfg.update(
        in_channels=unet_cfg.get("in_channels", 4), out_channels=unet_cfg.get("out_channels", 4),
        sample_size=unet_cfg.get("sample_size", 64), block_out_channels=boc, layers_per_block=lpb,
        down_block_types=tuple(_DOWN[t] for t in unet_cfg["down_block_types"]),
        up_block_types=tuple(_UP[t] for t in unet_cfg["up_block_types"]),
        norm_num_groups=unet_cfg.get("norm_num_groups", 32), norm_eps=unet_cfg.get("norm_eps", 1e-5),
        cross_attention_dim=unet_cfg.get("cross_attention_dim", 768), num_attention_heads=heads,
        motion_num_attention_heads=adapter_cfg.get("motion_num_attention_heads", 8),
        motion_max_seq_length=adapter_cfg.get("motion_max_seq_length", 32),
        use_motion_mid_block=adapter_cfg.get("use_motion_mid_block", True),
    )
    return cfg


def vae_config(cfg: dict) -> dict:
    """diffusers AutoencoderKL config.json -> the vdiff.AutoencoderKL (decoder) config."""
    from .models.vae import VAE_FULL
    out = dict(VAE_FULL)
    for k in ("in_channels", "out_channels", "latent_channels", "layers_per_block", "norm_num_groups",
              "sample_size", "scaling_factor"):
        if cfg.get(k) is not None:
            out[k] = cfg[k]
    out["block_out_channels"] = tuple(cfg.get("block_out_channels", out["block_out_channels"]))
    return out


def _empty_on(cls, cfg, device, **kw):
    """Build on the meta device, then allocate on `device` (no fp32 CPU copy of 1.3B params)."""
    from .models.layers import SinusoidalPositionalEmbedding
    with torch.device("meta"):
        m = cls(cfg, **kw)
    m = m.to_empty(device=device)
    for mod in m.modules():
        if isinstance(mod, SinusoidalPositionalEmbedding):
            mod.reset_buffers()
    return m.to(dtype=torch.bfloat16)


@torch.no_grad()
def _assign(model, sd: dict, skip=lambda k: False, what="model"):
    own = model.state_dict()
    keep = {k: v for k, v in sd.items() if not skip(k) and not k.endswith(".pos_embed.pe")}
    missing = [k for k in own if k not in keep and not k.endswith(".pos_embed.pe")]
    unexpected = [k for k in keep if k not in own]
    if missing or unexpected:
        raise KeyError(f"{what}: state dict mismatch: missing={missing[:6]} unexpected={unexpected[:6]}")
    for k, v in keep.items():
        if tuple(own[k].shape) != tuple(v.shape):
            raise ValueError(f"{what}: {k} has shape {tuple(v.shape)}, the model {tuple(own[k].shape)}")
        own[k].copy_(v.to(own[k].dtype))
    return model


def load_unet_motion(unet_dir, adapter: MotionAdapter, device="cuda", variant=None):
    """UNetMotionModel.from_unet2d(unet, motion_adapter) over local files."""
    from .models import UNetMotionModel
    d = _local_dir(unet_dir, "unet")
    cfg = motion_unet_config(read_json(d / "config.json"), adapter.config)
    unet = _empty_on(UNetMotionModel, cfg, device)
    sd = load_weights(d, variant)
    clash = [k for k in adapter.state_dict() if k in sd]
    if clash:
        raise KeyError(f"UNet checkpoint already holds motion keys: {clash[:4]}")
    return _assign(unet, {**sd, **adapter.state_dict()}, what="UNetMotionModel")


def load_vae(vae_dir, device="cuda", variant=None):
    from .models.vae import AutoencoderKL
    d = _local_dir(vae_dir, "vae")
    cfg = vae_config(read_json(d / "config.json"))
    sd = load_weights(d, variant)
    # the encoder is built only from a checkpoint that holds all of it; a partial one (or none) gives
    # the decoder-only model, whose encode() says so
    enc = ("encoder.", "quant_conv.")
    with torch.device("meta"):
        want = {k for k in AutoencoderKL(cfg, encoder=True).state_dict() if k.startswith(enc)}
    whole = want <= set(sd)
    vae = _empty_on(AutoencoderKL, cfg, device, encoder=whole)
    return _assign(vae, sd, skip=(lambda k: False) if whole else (lambda k: k.startswith(enc)), what="AutoencoderKL")


def load_text_encoder(enc_dir, device="cuda", variant=None):
    """transformers' `text_encoder/` folder: config.json (CLIPTextConfig) + model[.variant].safetensors
    -> vdiff.CLIPTextModel in bf16 on `device` (not prepared)."""
    from safetensors.torch import load_file

    from .models.clip import CLIPTextModel
    d = _local_dir(enc_dir, "text_encoder")
    cfg = read_json(d / "config.json")
    if "CLIPTextModelWithProjection" in (cfg.get("architectures") or []):
        raise NotImplementedError("CLIPTextModelWithProjection (SDXL's second encoder) is not built")
    f = d / ("model" + (f".{variant}" if variant else "") + ".safetensors")
    if not f.exists():
        raise FileNotFoundError(f"no {f.name} in {d}")
    with torch.device("meta"):
        m = CLIPTextModel(cfg)
    m = m.to_empty(device=device).to(dtype=torch.bfloat16)
    sd = {k: v.to(torch.bfloat16) for k, v in load_file(str(f)).items()}
    m.load_state_dict(sd, strict=True)
    return m.eval()


def load_tokenizer(tok_dir):
    """The `tokenizer/` folder (vocab.json + merges.txt [+ tokenizer_config.json]) -> vdiff.CLIPTokenizer."""
    from .tokenizer import CLIPTokenizer
    return CLIPTokenizer.from_pretrained(_local_dir(tok_dir, "tokenizer"))


def load_scheduler(sched_dir):
    """The pipeline's scheduler from scheduler_config.json.  SD-1.5 ships PNDMScheduler, which the
    reference immediately replaces (05:136-141 DDIM, 01/03 Euler) from `pipe.scheduler.config`;
    DDIM / Euler / Euler-ancestral / LCM configs build that class, anything else a DDIMScheduler holding the same config
    (its unknown keys are kept in `.config` so the reference's from_config(...) sees them)."""
    from .sched import DDIMScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, LCMScheduler
    cfg = read_json(Path(sched_dir) / "scheduler_config.json")
    cls = {"EulerDiscreteScheduler": EulerDiscreteScheduler, "LCMScheduler": LCMScheduler,
           "EulerAncestralDiscreteScheduler": EulerAncestralDiscreteScheduler}.get(
        cfg.get("_class_name"), DDIMScheduler)
    s = cls.from_config({k: v for k, v in cfg.items() if not k.startswith("_")})
    s.source_config = cfg
    return s


# ---------------------------------------------------------------------------- IP-Adapter
# An IP-Adapter checkpoint numbers its per-attention weights `ip_adapter.{id}.to_k_ip.weight` /
# `.to_v_ip.weight` with id = 1, 3, 5, ...: diffusers walks the UNet's attention processors in
# module order, counts every one, and the cross-attentions are the odd ones — motion modules
# skipped.  For UNetMotionModel that order is the blocks below, each block's attentions[i].
# transformer_blocks[j].attn2 in turn.  This table is the ONE place the order is written down
# (UNetMotionModel.spatial_cross_attentions follows it); it restates diffusers'
# _convert_ip_adapter_attn_to_diffusers and is not pinned by any file in this repository.
IP_ADAPTER_BLOCK_ORDER = ("down_blocks", "up_blocks", "mid_block")
IP_ADAPTER_WEIGHT_NAME = "ip-adapter_sd15.safetensors"


def ip_adapter_key_ids(n_cross: int) -> list:
    """The checkpoint ids of the n_cross spatial cross-attentions, in IP_ADAPTER_BLOCK_ORDER."""
    return [2 * i + 1 for i in range(n_cross)]


def read_ip_adapter(path, subfolder=None, weight_name=IP_ADAPTER_WEIGHT_NAME):
    """(image_proj, ip_adapter): the two key groups of a LOCAL adapter file, prefixes stripped.
    `.safetensors` holds flat `image_proj.*` / `ip_adapter.*` keys, `.bin` (torch.load with
    weights_only=True) the two groups as nested dicts."""
    if isinstance(path, (list, tuple)) or isinstance(weight_name, (list, tuple)):
        raise NotImplementedError("a list of IP-Adapters (multiple image prompts) is not supported: load one")
    if isinstance(path, dict):
        sd = path
    else:
        f = _local_dir(path, "load_ip_adapter")
        if subfolder:
            f = f / subfolder
        f = f / weight_name
        if not f.exists():
            raise FileNotFoundError(f"no {weight_name} in {f.parent} (local files only)")
        if f.suffix == ".safetensors":
            from safetensors.torch import load_file
            sd = load_file(str(f))
        elif f.suffix == ".bin":
            sd = torch.load(str(f), map_location="cpu", weights_only=True)
        else:
            raise ValueError(f"{f.name}: an IP-Adapter file is .safetensors or .bin")
    groups = {"image_proj": {}, "ip_adapter": {}}
    for k, v in sd.items():
        if k in groups and isinstance(v, dict):
            groups[k].update(v)
            continue
        g, _, rest = k.partition(".")
        if g not in groups:
            raise KeyError(f"IP-Adapter checkpoint: key {k!r} is in neither the image_proj nor the ip_adapter group")
        groups[g][rest] = v
    return groups["image_proj"], groups["ip_adapter"]


def check_ip_adapter_variant(image_proj: dict, ip_adapter: dict):
    """Only the plain adapter (image_proj.proj + image_proj.norm, to_k_ip / to_v_ip) is built."""
    if any(k == "latents" or k.startswith("latents.") for k in image_proj):
        raise NotImplementedError("IP-Adapter Plus (image_proj.latents: the Resampler projection) is not supported")
    if any(k.startswith("proj.0.") for k in image_proj):
        raise NotImplementedError("IP-Adapter Full Face / FaceID (image_proj.proj.0.*: an MLP projection) is not supported")
    if any("to_k_lora" in k or "to_q_lora" in k or "to_v_lora" in k or "to_out_lora" in k for k in ip_adapter):
        raise NotImplementedError("IP-Adapter FaceID (ip_adapter.*.to_k_lora*: LoRA attention weights) is not supported")
    want = {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}
    if set(image_proj) != want:
        raise KeyError(f"IP-Adapter image_proj keys {sorted(image_proj)}: expected {sorted(want)}")


def ip_adapter_kv_weights(ip_adapter: dict, n_cross: int) -> list:
    """[(to_k_ip.weight, to_v_ip.weight)] per spatial cross-attention, by ip_adapter_key_ids."""
    want = {f"{i}.to_{kv}_ip.weight" for i in ip_adapter_key_ids(n_cross) for kv in "kv"}
    missing, unexpected = sorted(want - set(ip_adapter)), sorted(set(ip_adapter) - want)
    if missing or unexpected:
        raise KeyError(f"IP-Adapter ip_adapter keys do not fit {n_cross} cross-attentions: "
                       f"missing={missing[:4]} unexpected={unexpected[:4]}")
    return [(ip_adapter[f"{i}.to_k_ip.weight"], ip_adapter[f"{i}.to_v_ip.weight"]) for i in ip_adapter_key_ids(n_cross)]


def load_image_encoder(enc_dir, device="cuda", variant=None):
    """transformers' `image_encoder/` folder (config.json of a CLIPVisionConfig + model[.variant].
    safetensors) -> vdiff.CLIPVisionModelWithProjection in bf16 on `device` (not prepared)."""
    from safetensors.torch import load_file

    from .models.clip import CLIPVisionModelWithProjection
    d = _local_dir(enc_dir, "image_encoder")
    cfg = read_json(d / "config.json")
    cfg = cfg.get("vision_config", cfg) if "hidden_size" not in cfg else cfg
    f = d / ("model" + (f".{variant}" if variant else "") + ".safetensors")
    if not f.exists():
        raise FileNotFoundError(f"no {f.name} in {d}")
    with torch.device("meta"):
        m = CLIPVisionModelWithProjection(cfg)
    m = m.to_empty(device=device).to(dtype=torch.bfloat16)
    m.load_state_dict({k: v.to(torch.bfloat16) for k, v in load_file(str(f)).items()}, strict=True)
    return m.eval()
