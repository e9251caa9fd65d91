"""CLIP text encoder (transformers.CLIPTextModel as SD-1.5's `text_encoder/` ships it and as
diffusers' `encode_prompt` drives it): token ids -> (B, S, H) hidden states on the HIP kernels.

The module tree, parameter names and config keys are transformers' own, so real state dicts
load unchanged (both spellings: SD-1.5's checkpoint prefixes every key with `text_model.`,
transformers 5.x's own `state_dict()` does not) and inspection tooling sees the names it knows:

    text_model.embeddings.{token_embedding, position_embedding}
    text_model.encoder.layers.N.{layer_norm1, self_attn.{q_proj,k_proj,v_proj,out_proj},
                                 layer_norm2, mlp.{fc1,fc2}}
    text_model.final_layer_norm

Device path (after prepare(), rows [(b, s)][H] in bf16, no host sync, no CPU fallback):
embedding rows by torch indexing (token row + position row, added in fp32, rounded once);
per layer one fused q|k|v GEMM, the causal flash attention (ops.attention(causal=True)) on
column slices of that buffer, the out-proj GEMM with the residual and the next LayerNorm in
its epilogue call (ops.gemm_ln: fused where the plan has it, else GEMM + vd_layernorm), fc1
with the QuickGELU (or erf-GELU) epilogue, fc2 with the residual and the following LayerNorm.
Padding is attended to, causally, exactly as SD-1.5's pipeline does (it passes no mask).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from .layers import LayerNorm, Linear, bf, f32

CLIP_SD15 = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                 num_attention_heads=12, max_position_embeddings=77, hidden_act="quick_gelu",
                 layer_norm_eps=1e-5, eos_token_id=2)
CLIP_TINY = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=3,
                 num_attention_heads=2, max_position_embeddings=77, hidden_act="quick_gelu",
                 layer_norm_eps=1e-5, eos_token_id=2)
CLIP_CONFIGS = {"sd15": CLIP_SD15, "tiny": CLIP_TINY}
_ACTS = {"quick_gelu": ops.ACT_QUICK_GELU, "gelu": ops.ACT_GELU}


def clip_config(config) -> dict:
    """A named config ("sd15", "tiny") or a transformers CLIPTextConfig dict (unknown keys kept)."""
    if isinstance(config, str):
        if config not in CLIP_CONFIGS:
            raise KeyError(f"unknown CLIP config {config!r}: one of {sorted(CLIP_CONFIGS)} or a dict")
        return dict(CLIP_CONFIGS[config])
    cfg = dict(CLIP_SD15)
    cfg.update({k: v for k, v in dict(config).items() if v is not None})
    return cfg


class CLIPTextModelOutput:
    """transformers' BaseModelOutputWithPooling as encode_prompt reads it: attributes, and
    [0] = last_hidden_state, [1] = pooler_output, [2] = hidden_states (when asked for)."""

    def __init__(self, last_hidden_state, pooler_output, hidden_states=None):
        self.last_hidden_state = last_hidden_state
        self.pooler_output = pooler_output
        self.hidden_states = hidden_states

    def to_tuple(self):
        t = (self.last_hidden_state, self.pooler_output)
        return t if self.hidden_states is None else t + (self.hidden_states,)

    def __getitem__(self, i):
        return self.to_tuple()[i]

    def __iter__(self):
        return iter(self.to_tuple())

    def __len__(self):
        return len(self.to_tuple())


class CLIPTextEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg["vocab_size"], cfg["hidden_size"])
        self.position_embedding = nn.Embedding(cfg["max_position_embeddings"], cfg["hidden_size"])

    def rows(self, input_ids):
        """bf16 rows [(b, s)][H]: token row + position row, added in fp32 and rounded once."""
        B, S = input_ids.shape
        x = self.token_embedding.weight[input_ids].float() + self.position_embedding.weight[:S].float()
        return x.to(torch.bfloat16).reshape(B * S, -1)


class CLIPAttention(nn.Module):
    def __init__(self, cfg, causal: bool = True):
        super().__init__()
        H = cfg["hidden_size"]
        self.num_heads = cfg["num_attention_heads"]
        self.head_dim = H // self.num_heads
        self.causal = causal  # the text tower; the vision tower attends to every patch
        takes = (32, 64) if causal else (32, 40, 64, 80, 128, 160)
        if self.head_dim * self.num_heads != H or self.head_dim not in takes:
            raise NotImplementedError(f"CLIP head_dim {H} / {self.num_heads}: the {'causal ' if causal else ''}flash "
                                      f"kernel takes one of {takes}")
        self.k_proj = Linear(H, H)
        self.v_proj = Linear(H, H)
        self.q_proj = Linear(H, H)
        self.out_proj = Linear(H, H)

    def prepare(self):
        self._wqkv = bf(torch.cat([self.q_proj.weight, self.k_proj.weight, self.v_proj.weight], 0))
        self._bqkv = f32(torch.cat([self.q_proj.bias, self.k_proj.bias, self.v_proj.bias], 0))
        self._wo, self._bo = bf(self.out_proj.weight), f32(self.out_proj.bias)

    def attend(self, n, B, S):
        """Self-attention (causal in the text tower) of the normed rows n: the fused q|k|v GEMM,
        then the flash kernel on column slices of its output (q unscaled in bf16; the kernel
        applies head_dim^-1/2)."""
        H = self.num_heads * self.head_dim
        qkv = ops.gemm(n, self._wqkv, bias=self._bqkv)
        if not self.causal:
            return ops.attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], B, self.num_heads, S, S, self.head_dim)
        return ops.attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], B, self.num_heads, S, S, self.head_dim,
                             causal=True)


class CLIPMLP(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        if cfg["hidden_act"] not in _ACTS:
            raise NotImplementedError(f"CLIP hidden_act {cfg['hidden_act']!r}: one of {sorted(_ACTS)}")
        self.act = _ACTS[cfg["hidden_act"]]
        self.fc1 = Linear(cfg["hidden_size"], cfg["intermediate_size"])
        self.fc2 = Linear(cfg["intermediate_size"], cfg["hidden_size"])

    def prepare(self):
        self._w1, self._b1 = bf(self.fc1.weight), f32(self.fc1.bias)
        self._w2, self._b2 = bf(self.fc2.weight), f32(self.fc2.bias)


class CLIPEncoderLayer(nn.Module):
    def __init__(self, cfg, causal: bool = True):
        super().__init__()
        eps = cfg["layer_norm_eps"]
        self.self_attn = CLIPAttention(cfg, causal=causal)
        self.layer_norm1 = LayerNorm(cfg["hidden_size"], eps=eps)
        self.mlp = CLIPMLP(cfg)
        self.layer_norm2 = LayerNorm(cfg["hidden_size"], eps=eps)

    def run(self, h, n, B, S, next_norm: LayerNorm):
        """(h', n'): h the residual stream, n = layer_norm1(h); n' = next_norm(h') (the next
        layer's layer_norm1, or the final LayerNorm after the last layer)."""
        a = self.self_attn.attend(n, B, S)
        ln2 = self.layer_norm2
        h, n = ops.gemm_ln(a, self.self_attn._wo, ln2._g, ln2._b, eps=ln2.eps, bias=self.self_attn._bo, res=h)
        m = ops.gemm(n, self.mlp._w1, bias=self.mlp._b1, act=self.mlp.act)
        return ops.gemm_ln(m, self.mlp._w2, next_norm._g, next_norm._b, eps=next_norm.eps, bias=self.mlp._b2, res=h)


class CLIPEncoder(nn.Module):
    def __init__(self, cfg, causal: bool = True):
        super().__init__()
        self.layers = nn.ModuleList([CLIPEncoderLayer(cfg, causal=causal) for _ in range(cfg["num_hidden_layers"])])


class CLIPTextTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = CLIPTextEmbeddings(cfg)
        self.encoder = CLIPEncoder(cfg)
        self.final_layer_norm = LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])


class CLIPTextModel(nn.Module):
    """transformers.CLIPTextModel: CLIPTextModel("sd15" | "tiny" | config dict)."""

    def __init__(self, config="sd15"):
        super().__init__()
        self.config = clip_config(config)
        self.text_model = CLIPTextTransformer(self.config)
        self._prepared = False

    @property
    def device(self):
        return self.text_model.final_layer_norm.weight.device

    @property
    def dtype(self):
        return self.text_model.final_layer_norm.weight.dtype

    def prepare(self):
        """Derive the packed device operands (fused q|k|v, bf16 weights, fp32 biases / affines)."""
        for m in self.modules():  # not the Linear leaves: their weights are packed by their owners
            if isinstance(m, (CLIPAttention, CLIPMLP, LayerNorm)):
                m.prepare()
        self._prepared = True
        return self

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Accepts `text_model.`-prefixed keys (SD-1.5's checkpoint) and unprefixed ones
        (transformers 5.x's own state_dict()); an `embeddings.position_ids` buffer is skipped."""
        sd = {}
        for k, v in state_dict.items():
            if k.endswith("embeddings.position_ids"):
                continue
            sd[k if k.startswith("text_model.") else "text_model." + k] = v
        out = super().load_state_dict(sd, strict=strict, assign=assign)
        self._prepared = False
        return out

    def forward(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=True, **unused):
        if attention_mask is not None:
            raise NotImplementedError("attention_mask: SD-1.5's pipeline passes none (padding is attended to, causally)")
        if not input_ids.is_cuda:
            raise ValueError("vdiff modules run on the GPU only (got a CPU tensor); no CPU fallback")
        if input_ids.dim() != 2 or input_ids.shape[1] > self.config["max_position_embeddings"]:
            raise ValueError(f"input_ids must be (B, S <= {self.config['max_position_embeddings']}), "
                             f"got {tuple(input_ids.shape)}")
        if not self._prepared:
            self.prepare()
        tm = self.text_model
        B, S = input_ids.shape
        ids = input_ids.long()
        h = tm.embeddings.rows(ids)
        layers = list(tm.encoder.layers)
        hidden = [h]
        first = layers[0].layer_norm1 if layers else tm.final_layer_norm
        n = ops.layer_norm(h, first._g, first._b, eps=first.eps)
        for i, layer in enumerate(layers):
            nxt = layers[i + 1].layer_norm1 if i + 1 < len(layers) else tm.final_layer_norm
            h, n = layer.run(h, n, B, S, nxt)
            hidden.append(h)
        last = n.view(B, S, -1)  # final_layer_norm of the last layer's output
        eos = self.config["eos_token_id"]
        # transformers' rule: the legacy config (eos_token_id == 2) pools at the highest id of
        # each row, a corrected one at the first eos; device indexing, no host sync
        at = ids.argmax(-1) if eos == 2 else (ids == eos).int().argmax(-1)
        pooled = last[torch.arange(B, device=ids.device), at]
        hs = tuple(t.view(B, S, -1) for t in hidden) if output_hidden_states else None
        out = CLIPTextModelOutput(last, pooled, hs)
        return out if return_dict else out.to_tuple()


# ---------------------------------------------------------------------------- vision tower
# transformers.CLIPVisionModelWithProjection, the IP-Adapter's image encoder (ViT-H/14 in the
# SD-1.5 adapters: hidden 1280, 16 heads of d = 80, 257 tokens; ViT-L/14 has d = 64).  Parameter
# names are transformers' own, `pre_layrnorm` included:
#
#     vision_model.embeddings.{class_embedding, patch_embedding.weight, position_embedding.weight}
#     vision_model.pre_layrnorm, vision_model.encoder.layers.N.*, vision_model.post_layernorm
#     visual_projection.weight
#
# Device path: the patch embedding (a stride-p p x p convolution without bias) is the patch rows
# [(b, gy, gx)][3 p^2] times one GEMM with fp32 output, K zero-padded to a multiple of 8; class
# token and position rows are added in fp32 and the sum is rounded once; then the text tower's
# encoder layers with the non-causal flash attention.  Runs once per video.
CLIP_VIT_H14 = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16,
                    image_size=224, patch_size=14, num_channels=3, hidden_act="gelu", layer_norm_eps=1e-5,
                    projection_dim=1024)
CLIP_VISION_TINY = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                        image_size=56, patch_size=14, num_channels=3, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                        projection_dim=48)
CLIP_VISION_CONFIGS = {"vit_h14": CLIP_VIT_H14, "tiny": CLIP_VISION_TINY}


def clip_vision_config(config) -> dict:
    """A named config ("vit_h14", "tiny") or a transformers CLIPVisionConfig dict (unknown keys kept)."""
    if isinstance(config, str):
        if config not in CLIP_VISION_CONFIGS:
            raise KeyError(f"unknown CLIP vision config {config!r}: one of {sorted(CLIP_VISION_CONFIGS)} or a dict")
        return dict(CLIP_VISION_CONFIGS[config])
    cfg = dict(CLIP_VIT_H14)
    cfg.update({k: v for k, v in dict(config).items() if v is not None})
    return cfg


class CLIPVisionModelOutput:
    """transformers' CLIPVisionModelOutput: image_embeds, last_hidden_state, hidden_states."""

    def __init__(self, image_embeds, last_hidden_state, hidden_states=None):
        self.image_embeds = image_embeds
        self.last_hidden_state = last_hidden_state
        self.hidden_states = hidden_states

    def to_tuple(self):
        t = (self.image_embeds, self.last_hidden_state)
        return t if self.hidden_states is None else t + (self.hidden_states,)

    def __getitem__(self, i):
        return self.to_tuple()[i]


class CLIPVisionEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        H, p = cfg["hidden_size"], cfg["patch_size"]
        self.patch_size, self.image_size, self.num_channels = p, cfg["image_size"], cfg["num_channels"]
        self.class_embedding = nn.Parameter(torch.zeros(H))
        self.patch_embedding = nn.Conv2d(self.num_channels, H, kernel_size=p, stride=p, bias=False)
        self.num_positions = (self.image_size // p) ** 2 + 1
        self.position_embedding = nn.Embedding(self.num_positions, H)

    def prepare(self):
        w = self.patch_embedding.weight
        k = w[0].numel()
        self._kpad = (k + 7) // 8 * 8
        wp = torch.zeros(w.shape[0], self._kpad, device=w.device, dtype=torch.float32)
        wp[:, :k] = w.reshape(w.shape[0], k).float()
        self._wp = bf(wp)

    def rows(self, pixel_values):
        """bf16 rows [(b, token)][H]: [class ; patch GEMM] + position rows, summed in fp32, rounded once."""
        B, Cc, Hh, Ww = pixel_values.shape
        p = self.patch_size
        if Cc != self.num_channels or Hh != self.image_size or Ww != self.image_size:
            raise ValueError(f"pixel_values of shape {tuple(pixel_values.shape)}: expected "
                             f"(B, {self.num_channels}, {self.image_size}, {self.image_size})")
        g = Hh // p
        x = pixel_values.to(torch.bfloat16).reshape(B, Cc, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, -1)
        a = torch.zeros(B * g * g, self._kpad, device=x.device, dtype=torch.bfloat16)
        a[:, :x.shape[1]] = x
        patches = ops.gemm(a, self._wp, out_f32=True).view(B, g * g, -1)
        cls = self.class_embedding.float().expand(B, 1, -1)
        h = torch.cat([cls, patches], 1) + self.position_embedding.weight.float()
        return h.to(torch.bfloat16).reshape(B * (g * g + 1), -1)


class CLIPVisionTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        eps = cfg["layer_norm_eps"]
        self.embeddings = CLIPVisionEmbeddings(cfg)
        self.pre_layrnorm = LayerNorm(cfg["hidden_size"], eps=eps)  # transformers' spelling
        self.encoder = CLIPEncoder(cfg, causal=False)
        self.post_layernorm = LayerNorm(cfg["hidden_size"], eps=eps)


class CLIPVisionModelWithProjection(nn.Module):
    """transformers.CLIPVisionModelWithProjection("vit_h14" | "tiny" | config dict): pixel values
    (B, 3, S, S) -> image_embeds (B, projection_dim), last_hidden_state and, on request, the
    hidden states (the encoder's input after pre_layrnorm first, as transformers lists them)."""

    def __init__(self, config="vit_h14"):
        super().__init__()
        self.config = clip_vision_config(config)
        self.vision_model = CLIPVisionTransformer(self.config)
        self.visual_projection = Linear(self.config["hidden_size"], self.config["projection_dim"], bias=False)
        self._prepared = False

    @property
    def device(self):
        return self.visual_projection.weight.device

    @property
    def dtype(self):
        return self.visual_projection.weight.dtype

    def prepare(self):
        for m in self.modules():
            if isinstance(m, (CLIPAttention, CLIPMLP, LayerNorm, CLIPVisionEmbeddings)):
                m.prepare()
        self._wproj = bf(self.visual_projection.weight)
        self._prepared = True
        return self

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        sd = {k: v for k, v in state_dict.items() if not k.endswith("embeddings.position_ids")}
        out = super().load_state_dict(sd, strict=strict, assign=assign)
        self._prepared = False
        return out

    def forward(self, pixel_values, output_hidden_states=False, return_dict=True, **unused):
        if not pixel_values.is_cuda:
            raise ValueError("vdiff modules run on the GPU only (got a CPU tensor); no CPU fallback")
        if not self._prepared:
            self.prepare()
        vm = self.vision_model
        B = pixel_values.shape[0]
        e = vm.embeddings.rows(pixel_values)
        S = e.shape[0] // B
        pre = vm.pre_layrnorm
        h = ops.layer_norm(e, pre._g, pre._b, eps=pre.eps)
        layers = list(vm.encoder.layers)
        hidden = [h]
        first = layers[0].layer_norm1 if layers else vm.post_layernorm
        n = ops.layer_norm(h, first._g, first._b, eps=first.eps)
        for i, layer in enumerate(layers):
            nxt = layers[i + 1].layer_norm1 if i + 1 < len(layers) else vm.post_layernorm
            h, n = layer.run(h, n, B, S, nxt)
            hidden.append(h)
        pooled = n.view(B, S, -1)[:, 0].contiguous()  # post_layernorm of the class token
        embeds = ops.gemm(pooled, self._wproj)
        hs = tuple(t.view(B, S, -1) for t in hidden) if output_hidden_states else None
        out = CLIPVisionModelOutput(embeds, h.view(B, S, -1), hs)
        return out if return_dict else out.to_tuple()


class ImageProjection(nn.Module):
    """diffusers' ImageProjection (the plain IP-Adapter's image_proj): Linear(clip_dim ->
    n * cross_dim), reshape to (B, n, cross_dim), LayerNorm.  State-dict keys as the adapter
    checkpoint's `image_proj.` group: proj.{weight,bias}, norm.{weight,bias}."""

    def __init__(self, image_embed_dim: int, cross_attention_dim: int, num_image_text_embeds: int):
        super().__init__()
        self.num_image_text_embeds, self.cross_attention_dim = num_image_text_embeds, cross_attention_dim
        self.proj = Linear(image_embed_dim, num_image_text_embeds * cross_attention_dim)
        self.norm = LayerNorm(cross_attention_dim)

    @classmethod
    def from_state_dict(cls, sd: dict, cross_attention_dim: int):
        """The token count comes from the checkpoint: proj.weight.shape[0] // cross_attention_dim."""
        w = sd["proj.weight"]
        if w.shape[0] % cross_attention_dim:
            raise ValueError(f"image_proj.proj.weight has {w.shape[0]} rows: no multiple of cross_attention_dim "
                             f"{cross_attention_dim}")
        m = cls(w.shape[1], cross_attention_dim, w.shape[0] // cross_attention_dim)
        m.load_state_dict(sd, strict=True)
        return m

    def prepare(self):
        self._w, self._b = bf(self.proj.weight), f32(self.proj.bias)
        self.norm.prepare()
        return self

    def forward(self, image_embeds):
        """(B, clip_dim) or (B, 1, clip_dim) -> bf16 (B, n, cross_dim) on the HIP GEMM + LayerNorm."""
        if not image_embeds.is_cuda:
            raise ValueError("vdiff modules run on the GPU only (got a CPU tensor); no CPU fallback")
        if getattr(self, "_w", None) is None:
            self.prepare()
        x = image_embeds.reshape(image_embeds.shape[0], -1).to(torch.bfloat16).contiguous()
        y = ops.gemm(x, self._w, bias=self._b).view(x.shape[0] * self.num_image_text_embeds, self.cross_attention_dim)
        y = ops.layer_norm(y, self.norm._g, self.norm._b, eps=self.norm.eps)
        return y.view(x.shape[0], self.num_image_text_embeds, self.cross_attention_dim)
