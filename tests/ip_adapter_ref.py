"""fp64 / fp32 torch restatements of the IP-Adapter path (tests/test_ip_adapter_host.py,
tests/test_gpu_ip_adapter.py).  Nothing here imports vdiff: these are the independent side of
every comparison.

  two_softmax_attention  what VD_ATTN_TAIL(n) computes: one softmax over the first skv - n keys,
                         a second over the last n, the two normalised results summed
  ip_block_attn2         diffusers' IPAdapterAttnProcessor2_0 for one image-prompt adapter:
                         hidden + s * sdpa(q, k_ip, v_ip) before to_out
  image_projection       diffusers' ImageProjection: Linear -> (B, n, cross_dim) -> LayerNorm
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def _heads(x, heads):  # [B, S, H*d] -> [B, H, S, d]
    B, S, C = x.shape
    return x.reshape(B, S, heads, C // heads).transpose(1, 2)


def sdpa(q, k, v, heads, scale=None):
    """softmax(q k^T scale) v on [B, S, H*d] tensors, in the tensors' own precision."""
    qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    scale = qh.shape[-1] ** -0.5 if scale is None else scale
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(q.shape)


def two_softmax_attention(q, k, v, heads, n, kv_div=1, scale=None):
    """q [B, sq, H*d]; k, v [B / kv_div, skv, H*d], the last n rows of each key batch being the
    second segment.  fp64 throughout."""
    q, k, v = q.double(), k.double(), v.double()
    k = k.repeat_interleave(kv_div, 0)
    v = v.repeat_interleave(kv_div, 0)
    main = k.shape[1] - n
    assert main >= 1 and n >= 1
    return sdpa(q, k[:, :main], v[:, :main], heads, scale) + sdpa(q, k[:, main:], v[:, main:], heads, scale)


def image_projection(image_embeds, proj_w, proj_b, norm_w, norm_b, n, eps=1e-5):
    """[B, clip_dim] -> [B, n, cross_dim]"""
    x = F.linear(image_embeds, proj_w, proj_b)
    x = x.reshape(x.shape[0], n, -1)
    return F.layer_norm(x, (x.shape[-1],), norm_w, norm_b, eps)


def ip_block_attn2(hidden, ehs, ip_tokens, wq, wk, wv, wk_ip, wv_ip, wo, bo, heads, ip_scale):
    """The cross-attention of a transformer block with one image-prompt adapter.  hidden [B, S, C]
    is the normed input, ehs [B, L, cross], ip_tokens [B, n, cross]; returns to_out of
    sdpa(q, k, v) + ip_scale * sdpa(q, k_ip, v_ip) (no residual)."""
    q = F.linear(hidden, wq)
    a = sdpa(q, F.linear(ehs, wk), F.linear(ehs, wv), heads)
    b = sdpa(q, F.linear(ip_tokens, wk_ip), F.linear(ip_tokens, wv_ip), heads)
    return F.linear(a + ip_scale * b, wo, bo)


# ---------------------------------------------------------------- CLIP vision tower / preprocessing
def _act(name):
    return {"quick_gelu": lambda x: x * torch.sigmoid(1.702 * x), "gelu": F.gelu}[name]


def vision_tower(sd, cfg, pixel_values, emulate_bf16=False, causal=False):
    """transformers.CLIPVisionModelWithProjection restated on its own state dict (keys
    vision_model.* / visual_projection.weight), in the dtype of pixel_values.
    Returns (image_embeds, last_hidden_state, hidden_states).
    emulate_bf16 rounds to bf16 what the device path stores in bf16, where it stores it: the
    matrices and the pixel values, the embedding sum, every LayerNorm output, q|k|v, the attention
    output, both residual updates, the activated fc1 output, the pooled row and the embeds; the
    arithmetic between the roundings stays in pixel_values' dtype (use fp64).
    causal masks the attention as the text tower's (the host precondition: it must matter)."""
    p, H, heads, eps = cfg["patch_size"], cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    act = _act(cfg["hidden_act"])
    dt = pixel_values.dtype
    r = (lambda t: t.to(torch.bfloat16).to(dt)) if emulate_bf16 else (lambda t: t)
    g = lambda k: sd["vision_model." + k].to(dt)  # noqa: E731
    w = lambda k: r(g(k))  # noqa: E731  (a matrix: bf16 on the device)
    x = F.conv2d(r(pixel_values), w("embeddings.patch_embedding.weight"), stride=p).flatten(2).transpose(1, 2)
    cls = g("embeddings.class_embedding").expand(x.shape[0], 1, H)
    x = r(torch.cat([cls, x], 1) + g("embeddings.position_embedding.weight"))
    h = r(F.layer_norm(x, (H,), g("pre_layrnorm.weight"), g("pre_layrnorm.bias"), eps))
    hidden = [h]
    S = h.shape[1]
    mask = torch.full((S, S), float("-inf"), dtype=dt).triu(1) if causal else None
    for i in range(cfg["num_hidden_layers"]):
        L = f"encoder.layers.{i}."
        n = r(F.layer_norm(h, (H,), g(L + "layer_norm1.weight"), g(L + "layer_norm1.bias"), eps))
        q, k, v = (r(F.linear(n, w(L + f"self_attn.{c}_proj.weight"), g(L + f"self_attn.{c}_proj.bias"))) for c in "qkv")
        qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
        sc = qh @ kh.transpose(-1, -2) * qh.shape[-1] ** -0.5
        a = r((torch.softmax(sc if mask is None else sc + mask, -1) @ vh).transpose(1, 2).reshape(q.shape))
        h = r(h + F.linear(a, w(L + "self_attn.out_proj.weight"), g(L + "self_attn.out_proj.bias")))
        n = r(F.layer_norm(h, (H,), g(L + "layer_norm2.weight"), g(L + "layer_norm2.bias"), eps))
        m = r(act(F.linear(n, w(L + "mlp.fc1.weight"), g(L + "mlp.fc1.bias"))))
        h = r(h + F.linear(m, w(L + "mlp.fc2.weight"), g(L + "mlp.fc2.bias")))
        hidden.append(h)
    pooled = r(F.layer_norm(h[:, 0], (H,), g("post_layernorm.weight"), g("post_layernorm.bias"), eps))
    return r(F.linear(pooled, r(sd["visual_projection.weight"].to(dt)))), h, tuple(hidden)


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def preprocess(pil_image, size=224):
    """CLIP's preprocessing by the PIL formulas: RGB, bicubic resize of the shortest edge to `size`
    (long edge int(size * long / short)), centre crop, / 255, (x - mean) / std -> (3, size, size)."""
    import numpy as np
    from PIL import Image
    img = pil_image.convert("RGB")
    w, h = img.size
    if w <= h:
        nw, nh = size, int(size * h / w)
    else:
        nw, nh = int(size * w / h), size
    img = img.resize((nw, nh), Image.BICUBIC)
    left, top = (nw - size) // 2, (nh - size) // 2
    a = np.asarray(img.crop((left, top, left + size, top + size)), np.float64) / 255.0
    a = (a - np.asarray(CLIP_MEAN)) / np.asarray(CLIP_STD)
    return torch.from_numpy(a.transpose(2, 0, 1).copy())


VISION_TINY = {
    "d32": dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=56,
                patch_size=14, num_channels=3, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=48),
    "d80": dict(hidden_size=160, intermediate_size=320, num_hidden_layers=2, num_attention_heads=2, image_size=28,
                patch_size=14, num_channels=3, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=32),
}


def vision_synthetic_state_dict(cfg, seed=0):
    """Deterministic fp32 weights under transformers' key names: matrices N(0, 1/fan_in), LayerNorm
    affines near (1, 0), embeddings N(0, 0.5) — activations of order one through both layers."""
    g = torch.Generator().manual_seed(seed)
    H, I, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"]
    P = (cfg["image_size"] // p) ** 2 + 1
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g) * std  # noqa: E731
    sd = {"vision_model.embeddings.class_embedding": rn(H, std=0.5),
          "vision_model.embeddings.patch_embedding.weight": rn(H, 3, p, p, std=(3 * p * p) ** -0.5),
          "vision_model.embeddings.position_embedding.weight": rn(P, H, std=0.5)}

    def ln(name):
        sd[name + ".weight"] = 1 + rn(H, std=0.1)
        sd[name + ".bias"] = rn(H, std=0.1)

    def lin(name, o, i):
        sd[name + ".weight"] = rn(o, i, std=i ** -0.5)
        sd[name + ".bias"] = rn(o, std=0.1)

    ln("vision_model.pre_layrnorm")
    for i in range(cfg["num_hidden_layers"]):
        L = f"vision_model.encoder.layers.{i}."
        for c in "kvq":
            lin(L + f"self_attn.{c}_proj", H, H)
        lin(L + "self_attn.out_proj", H, H)
        ln(L + "layer_norm1")
        lin(L + "mlp.fc1", I, H)
        lin(L + "mlp.fc2", H, I)
        ln(L + "layer_norm2")
    ln("vision_model.post_layernorm")
    sd["visual_projection.weight"] = rn(cfg["projection_dim"], H, std=H ** -0.5)
    return sd


def vision_fixture_pixels(cfg, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, cfg["image_size"], cfg["image_size"], generator=g)


# ---------------------------------------------------------------- the transformer block with an adapter
def block_synthetic_state_dict(dim, heads, dim_head, cross, seed=0, ip_gain=3.0):
    """fp32 weights of a BasicTransformerBlock (its own state_dict keys) plus attn2.to_k_ip /
    to_v_ip.  to_v_ip carries ip_gain so that the image prompt moves the block output by far
    more than any parity bar (tests/test_ip_adapter_host.py asserts >= 0.2)."""
    g = torch.Generator().manual_seed(seed)
    inner = heads * dim_head
    rn = lambda o, i, gain=1.0: torch.randn(o, i, generator=g) * gain * i ** -0.5  # noqa: E731
    sd = {}
    for i in (1, 2, 3):
        sd[f"norm{i}.weight"] = 1 + 0.1 * torch.randn(dim, generator=g)
        sd[f"norm{i}.bias"] = 0.1 * torch.randn(dim, generator=g)
    for a, kvd in (("attn1", dim), ("attn2", cross)):
        sd[f"{a}.to_q.weight"] = rn(inner, dim, 2.0)
        sd[f"{a}.to_k.weight"] = rn(inner, kvd, 2.0)
        sd[f"{a}.to_v.weight"] = rn(inner, kvd)
        sd[f"{a}.to_out.0.weight"] = rn(dim, inner)
        sd[f"{a}.to_out.0.bias"] = 0.1 * torch.randn(dim, generator=g)
    sd["attn2.to_k_ip.weight"] = rn(inner, cross, 2.0)
    sd["attn2.to_v_ip.weight"] = rn(inner, cross, ip_gain)
    sd["ff.net.0.proj.weight"] = rn(8 * dim, dim)
    sd["ff.net.0.proj.bias"] = 0.1 * torch.randn(8 * dim, generator=g)
    sd["ff.net.2.weight"] = rn(dim, 4 * dim)
    sd["ff.net.2.bias"] = 0.1 * torch.randn(dim, generator=g)
    return sd


def transformer_block(sd, h, ehs, ip_tokens, heads, ip_scale=1.0):
    """diffusers' BasicTransformerBlock (layer_norm, GEGLU) on tokens h [N, S, C] with text ehs
    [N, L, cross]; ip_tokens [N, n, cross] or None (then the plain block).  In h's dtype."""
    w = {k: v.to(h.dtype) for k, v in sd.items()}
    C = h.shape[-1]
    ln = lambda x, i: F.layer_norm(x, (C,), w[f"norm{i}.weight"], w[f"norm{i}.bias"], 1e-5)  # noqa: E731
    n = ln(h, 1)
    a = sdpa(F.linear(n, w["attn1.to_q.weight"]), F.linear(n, w["attn1.to_k.weight"]), F.linear(n, w["attn1.to_v.weight"]), heads)
    h = h + F.linear(a, w["attn1.to_out.0.weight"], w["attn1.to_out.0.bias"])
    n = ln(h, 2)
    if ip_tokens is None:
        q = F.linear(n, w["attn2.to_q.weight"])
        a = sdpa(q, F.linear(ehs, w["attn2.to_k.weight"]), F.linear(ehs, w["attn2.to_v.weight"]), heads)
        h = h + F.linear(a, w["attn2.to_out.0.weight"], w["attn2.to_out.0.bias"])
    else:
        h = h + ip_block_attn2(n, ehs, ip_tokens, w["attn2.to_q.weight"], w["attn2.to_k.weight"], w["attn2.to_v.weight"],
                               w["attn2.to_k_ip.weight"], w["attn2.to_v_ip.weight"], w["attn2.to_out.0.weight"],
                               w["attn2.to_out.0.bias"], heads, ip_scale)
    n = ln(h, 3)
    x, gate = F.linear(n, w["ff.net.0.proj.weight"], w["ff.net.0.proj.bias"]).chunk(2, -1)
    return h + F.linear(x * F.gelu(gate), w["ff.net.2.weight"], w["ff.net.2.bias"])


# (dim, heads, dim_head, cross, hw, frames, L, n): the tiny config's two levels and one block of
# the full config's level-1 shape; two videos (the CFG pair) each
BLOCK_CASES = {"tiny_d32": (64, 2, 32, 64, 64, 2, 77, 4), "tiny_d64": (128, 2, 64, 64, 16, 2, 77, 4),
               "level1_d40": (320, 8, 40, 768, 64, 2, 77, 4)}


def block_inputs(case, seed=0):
    """(sd, h [2, frames * hw... as images: 2 * frames, hw, dim], ehs [2, L, cross], ip [2, n, cross]):
    both videos share the latents-side input h (the CFG pair), the text and image tokens differ."""
    dim, heads, dh, cross, hw, frames, L, n = BLOCK_CASES[case]
    g = torch.Generator().manual_seed(100 + seed)
    sd = block_synthetic_state_dict(dim, heads, dh, cross, seed)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()  # noqa: E731
    h_half = r(frames, hw, dim)
    return sd, h_half, r(2, L, cross), r(2, n, cross)
