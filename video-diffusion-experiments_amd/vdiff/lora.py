"""LoRA loading for UNetMotionModel: `pipe.load_lora_weights(...)` and the adapter calls around
it (`set_adapters`, `get_active_adapters`, `delete_adapters`, `unload_lora_weights`, `fuse_lora`,
`unfuse_lora`) — motion LoRAs (zoom, pan, tilt) and the AnimateLCM LoRA.

Host-only.  The HIP kernels read packed operands that `prepare()` builds from the module
parameters, so a LoRA is always MERGED into the parameters:

    W_eff = W0 + sum over active adapters of  weight * fuse_scale * (alpha / r) * (B . A)

computed on the CPU, accumulated in fp64 and rounded ONCE to the parameter's dtype (bf16 on the
device); then the whole UNet is re-packed (`UNetMotionModel.prepare()`).  The untouched base
tensor W0 of every parameter a LoRA touches is kept, so weight 0, `delete_adapters` and
`unload_lora_weights` restore the parameters bit for bit.  Adapters are set BEFORE the pipeline
call, like `enable_freeu`: a DenoiseLoop (and its captured graph and cross-attention K/V cache)
holds the operands of the weights it was built with; the pipelines build a new loop per call.

Targets: the Linear, 1x1-conv and 3x3-conv weights of the spatial transformers, the motion
transformers, the resnets (time_emb_proj included) and the down / up samplers.  A conv LoRA is
A [r, Cin, k, k] then B [Cout, r, 1, 1]; its merged form is B.flatten(1) @ A.flatten(1) reshaped
to the conv's weight.

Key layouts (local `.safetensors`, or `.bin` through torch.load(weights_only=True), or a dict):
  (a) PEFT / diffusers   unet.<module>.lora_A.weight / .lora_B.weight [, unet.<module>.alpha]
  (b) legacy diffusers   [unet.]<module>.lora.down.weight / .lora.up.weight, and the attention
                         processor form <attn>.processor.to_q_lora.down.weight
  (c) kohya              lora_unet_<module with '.' as '_'>.lora_down.weight / .lora_up.weight /
                         .alpha — un-mangled through a table of the model's own module names
  (d) motion LoRA        the original AnimateDiff motion-LoRA names
                         (...motion_modules.0.temporal_transformer.transformer_blocks.0.
                         attention_blocks.0.processor.to_q_lora.down.weight), mapped onto the
                         diffusers tree by MOTION_LORA_RENAMES below
alpha defaults to r (scale 1).  Parity of (b), (c) and (d) to diffusers' converters is UNPINNED:
they are written from memory of those converters; no checkpoint of either kind is in this
repository.
"""
from __future__ import annotations

import re
from pathlib import Path

import torch
from torch import nn

# the parts of the module tree a LoRA may touch
TARGET_PARTS = (".attentions.", ".motion_modules.", ".resnets.", ".downsamplers.", ".upsamplers.")

# (d) original motion-LoRA key -> diffusers tree, applied in order (regex, replacement).
# Unpinned: restated from memory of diffusers' _convert_non_diffusers / motion-LoRA handling.
MOTION_LORA_RENAMES = (
    (r"\.temporal_transformer(?=\.)", ""),                                           # the wrapper level is dropped
    (r"\.attention_blocks\.(\d+)(?=\.|$)", lambda m: f".attn{int(m.group(1)) + 1}"),  # attention_blocks.N -> attnN+1
    (r"\.processor(?=\.|$)", ""),                                                    # the processor level is dropped
    (r"\.to_out$", ".to_out.0"),                                                     # to_out_lora -> to_out.0
)

_SUFFIXES = (  # (suffix, kind): A = down, B = up
    (".lora_A.weight", "A"), (".lora_B.weight", "B"),
    (".lora.down.weight", "A"), (".lora.up.weight", "B"),
    ("_lora.down.weight", "A"), ("_lora.up.weight", "B"),   # the processor form: to_q_lora.down.weight
    (".lora_down.weight", "A"), (".lora_up.weight", "B"),
    (".alpha", "alpha"),
)
_TEXT_PREFIXES = ("text_encoder.", "text_encoder_2.", "lora_te_", "lora_te1_", "lora_te2_")


def target_modules(unet) -> dict:
    """{module name: module} of every weight a LoRA may touch."""
    out = {}
    for name, m in unet.named_modules():
        if isinstance(m, (nn.Linear, nn.Conv2d)) and any(p in "." + name for p in TARGET_PARTS) \
                and not name.endswith("_ip"):
            out[name] = m
    return out


def read_lora_file(src, weight_name=None, subfolder=None) -> dict:
    """A state dict from a dict, a LOCAL file, or a LOCAL directory (+ subfolder) holding
    weight_name (default: its only .safetensors file, else pytorch_lora_weights.bin)."""
    if isinstance(src, dict):
        return dict(src)
    p = Path(src)
    if p.is_dir():
        if subfolder:
            p = p / subfolder
        if weight_name is None:
            cands = sorted(p.glob("*.safetensors"))
            if len(cands) == 1:
                weight_name = cands[0].name
            elif (p / "pytorch_lora_weights.safetensors").exists():
                weight_name = "pytorch_lora_weights.safetensors"
            elif (p / "pytorch_lora_weights.bin").exists():
                weight_name = "pytorch_lora_weights.bin"
            else:
                raise FileNotFoundError(f"load_lora_weights: {len(cands)} .safetensors files in {p}: pass weight_name=")
        p = p / weight_name
    if not p.is_file():
        raise FileNotFoundError(f"load_lora_weights: {str(src)!r} is not a local file or directory (hub "
                                "checkpoints are unreachable offline)")
    if p.suffix == ".safetensors":
        from safetensors.torch import load_file
        return load_file(str(p))
    if p.suffix in (".bin", ".pt", ".pth"):
        return torch.load(str(p), map_location="cpu", weights_only=True)
    raise ValueError(f"{p.name}: a LoRA file is .safetensors or .bin")


def _split_key(key: str):
    for suf, kind in _SUFFIXES:
        if key.endswith(suf):
            return key[:-len(suf)], kind
    return None, None


def parse_lora_state_dict(sd: dict, names) -> dict:
    """{module name: {"A": down, "B": up, "alpha": float or None}} from any of the four layouts;
    `names` are the model's target module names.  KeyError lists keys that map to no module,
    NotImplementedError names text-encoder keys, ValueError an ambiguous kohya name."""
    names = set(names)
    kohya, clash = {}, set()
    for n in names:
        k = n.replace(".", "_")
        if k in kohya:
            clash.add(k)
        kohya[k] = n
    text = [k for k in sd if k.startswith(_TEXT_PREFIXES)]
    if text:
        raise NotImplementedError(f"text-encoder LoRA keys are not supported (e.g. {text[0]!r}): only the UNet's "
                                  "weights are merged")
    out, unknown = {}, []
    for key, v in sd.items():
        mod, kind = _split_key(key)
        if mod is None:
            unknown.append(key)
            continue
        if mod.startswith("lora_unet_"):                     # (c)
            k = mod[len("lora_unet_"):]
            if k in clash:
                raise ValueError(f"kohya LoRA key {key!r}: {k!r} is the mangled name of more than one module")
            mod = kohya.get(k)
        else:
            if mod.startswith("unet."):                      # (a), (b)
                mod = mod[len("unet."):]
            for pat, rep in MOTION_LORA_RENAMES:             # (b) processor form and (d)
                mod = re.sub(pat, rep, mod)
        if mod not in names:
            unknown.append(key)
            continue
        e = out.setdefault(mod, {"A": None, "B": None, "alpha": None})
        e[kind] = float(v) if kind == "alpha" else v
    if unknown:
        raise KeyError(f"LoRA keys that map to no module of the UNet ({len(unknown)}): {unknown[:4]}")
    half = [m for m, e in out.items() if e["A"] is None or e["B"] is None]
    if half:
        raise KeyError(f"LoRA modules with only one of the down / up weights: {half[:4]}")
    return out


def lora_delta(A: torch.Tensor, B: torch.Tensor, shape, dtype=torch.float64) -> torch.Tensor:
    """B . A in `dtype`, in the shape of the weight it is added to: Linear [out, r] @ [r, in];
    conv [Cout, r, 1, 1] after [r, Cin, k, k] as B.flatten(1) @ A.flatten(1) reshaped."""
    r = A.shape[0]
    if B.dim() != A.dim() or B.shape[1] != r or any(s != 1 for s in B.shape[2:]):
        raise ValueError(f"LoRA pair down {tuple(A.shape)} / up {tuple(B.shape)}: expected [r, in, ...] and [out, r, 1...]")
    d = B.flatten(1).to("cpu", dtype) @ A.flatten(1).to("cpu", dtype)
    if d.numel() != torch.Size(shape).numel() or d.shape[0] != shape[0]:
        raise ValueError(f"LoRA pair down {tuple(A.shape)} / up {tuple(B.shape)} does not fit a weight of shape "
                         f"{tuple(shape)}")
    return d.reshape(shape)


class LoraState:
    """What UNetMotionModel keeps once a LoRA is loaded."""

    def __init__(self):
        self.base = {}       # module name -> the untouched weight (a clone, on the weight's device)
        self.adapters = {}   # adapter name -> {module name: (A, B, alpha / r)}
        self.active = {}     # adapter name -> weight, in activation order
        self.fuse_scale = 1.0


def _state(unet) -> LoraState:
    st = getattr(unet, "_lora", None)
    if st is None:
        st = unet._lora = LoraState()
    return st


@torch.no_grad()
def merge(unet, touched=None):
    """Rewrite every touched weight from its base and the active adapters, then re-pack."""
    st = _state(unet)
    mods = target_modules(unet)
    for name in (st.base if touched is None else touched):
        w = mods[name].weight
        acc = st.base[name].to("cpu", torch.float64)
        for ad, weight in st.active.items():
            ent = st.adapters[ad].get(name)
            if ent is not None and weight != 0:
                A, B, scale = ent
                acc = acc + (weight * st.fuse_scale * scale) * lora_delta(A, B, w.shape)
        w.copy_(acc.to(w.dtype))
    used = {n for ad in st.adapters.values() for n in ad}
    for name in [n for n in st.base if n not in used]:  # no adapter left on it: drop the kept base
        del st.base[name]
    if getattr(unet, "_prepared", False):
        unet.prepare()


@torch.no_grad()
def load_lora_state_dict(unet, state_dict, adapter_name=None, weight: float = 1.0):
    """Parse, check every shape, keep the bases, activate the adapter and merge."""
    st = _state(unet)
    mods = target_modules(unet)
    parsed = parse_lora_state_dict(state_dict, mods)
    if adapter_name is None:
        i = 0
        while f"default_{i}" in st.adapters:
            i += 1
        adapter_name = f"default_{i}"
    if adapter_name in st.adapters:
        raise ValueError(f"adapter {adapter_name!r} is already loaded: delete_adapters({adapter_name!r}) first")
    ent = {}
    for name, e in parsed.items():
        A, B = e["A"].detach().to("cpu"), e["B"].detach().to("cpu")
        if B.shape[0] != mods[name].weight.shape[0] or A.flatten(1).shape[1] != mods[name].weight[0].numel():
            raise ValueError(f"LoRA for {name}: down {tuple(A.shape)} / up {tuple(B.shape)} do not fit the weight "
                             f"{tuple(mods[name].weight.shape)}")
        if B.shape[1] != A.shape[0]:
            raise ValueError(f"LoRA for {name}: rank of down {tuple(A.shape)} and up {tuple(B.shape)} differ")
        r = A.shape[0]
        ent[name] = (A, B, (e["alpha"] if e["alpha"] is not None else r) / r)
    for name in ent:
        if name not in st.base:
            st.base[name] = mods[name].weight.detach().clone()
    st.adapters[adapter_name] = ent
    st.active[adapter_name] = float(weight)
    merge(unet, touched=[n for n in st.base if n in ent])
    return adapter_name


def set_adapters(unet, names, adapter_weights=None):
    st = _state(unet)
    names = [names] if isinstance(names, str) else list(names)
    if adapter_weights is None:
        adapter_weights = [1.0] * len(names)
    elif isinstance(adapter_weights, (int, float)):
        adapter_weights = [float(adapter_weights)] * len(names)
    if len(adapter_weights) != len(names):
        raise ValueError(f"{len(adapter_weights)} adapter weights for {len(names)} adapters")
    for n in names:
        if n not in st.adapters:
            raise ValueError(f"adapter {n!r} is not loaded (loaded: {sorted(st.adapters)})")
    for w in adapter_weights:
        if w is not None and not isinstance(w, (int, float)):
            raise NotImplementedError("per-block adapter weights (a dict) are not supported: one float per adapter")
    st.active = {n: 1.0 if w is None else float(w) for n, w in zip(names, adapter_weights)}
    merge(unet)


def get_active_adapters(unet) -> list:
    return list(_state(unet).active)


def delete_adapters(unet, names):
    st = _state(unet)
    names = [names] if isinstance(names, str) else list(names)
    for n in names:
        if n not in st.adapters:
            raise ValueError(f"adapter {n!r} is not loaded (loaded: {sorted(st.adapters)})")
    touched = list(st.base)
    for n in names:
        del st.adapters[n]
        st.active.pop(n, None)
    merge(unet, touched=touched)


def unload(unet):
    st = _state(unet)
    touched = list(st.base)
    st.adapters.clear()
    st.active.clear()
    st.fuse_scale = 1.0
    merge(unet, touched=touched)


def set_fuse_scale(unet, scale: float):
    st = _state(unet)
    st.fuse_scale = float(scale)
    merge(unet)
