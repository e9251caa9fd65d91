"""fp64 plain-torch restatement of transformers.CLIPTextModel (the text encoder of SD-1.5), the
reference of tests/test_clip_host.py and tests/test_gpu_clip.py, and the seeded synthetic
weights both sides of the parity tests load.

clip_ref(sd, cfg, ids) is pinned to transformers' own CLIPTextModel by the committed fixture
tests/golden/clip_tiny.npz (written by tests/golden/make_clip_golden.py from transformers'
outputs) and, where transformers is importable, by a live model.

Two switches exist for the tests' conditioning checks, never for the reference itself:
  causal=False   drops the causal mask (the fixture must be sensitive to it),
  emulate_bf16   rounds to bf16 every tensor the device path stores in bf16, at the point it
                 stores it (embedding rows, every LayerNorm output, q|k|v, the attention output,
                 both residual-stream updates, the activated fc1 output).  The arithmetic between
                 the roundings stays fp64, so the emulation lacks the device's fp32 accumulation
                 order, its bf16 P in the flash kernel and the hardware exp2 / reciprocal.
"""
from __future__ import annotations

import math
import zlib

import torch

TINY = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_hidden_layers=3,
            num_attention_heads=2, max_position_embeddings=77, hidden_act="quick_gelu",
            layer_norm_eps=1e-5, eos_token_id=2)
BOS, EOS = 510, 511  # the fixture's framing ids (the two highest of the tiny vocabulary, as CLIP's are)


def param_shapes(cfg) -> dict:
    """Every parameter of CLIPTextModel under SD-1.5's `text_model.`-prefixed names."""
    H, I, V, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["max_position_embeddings"]
    out = {"text_model.embeddings.token_embedding.weight": (V, H),
           "text_model.embeddings.position_embedding.weight": (P, H),
           "text_model.final_layer_norm.weight": (H,), "text_model.final_layer_norm.bias": (H,)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[p + f"self_attn.{n}.weight"], out[p + f"self_attn.{n}.bias"] = (H, H), (H,)
        for n in ("layer_norm1", "layer_norm2"):
            out[p + n + ".weight"], out[p + n + ".bias"] = (H,), (H,)
        out[p + "mlp.fc1.weight"], out[p + "mlp.fc1.bias"] = (I, H), (I,)
        out[p + "mlp.fc2.weight"], out[p + "mlp.fc2.bias"] = (H, I), (H,)
    return out


def synthetic_state_dict(cfg, seed: int = 0) -> dict:
    """bf16-representable fp32 weights: a seeded draw per key, in sorted key order.  Linear weights
    ~ N(0, 1/fan_in), biases and LayerNorm beta ~ N(0, 0.1^2), gamma = 1 + N(0, 0.1^2), embeddings
    ~ N(0, 0.5^2).  No rescaling: with these the causal mask moves the tiny config's output by
    0.55 rel-L2 (tests/test_clip_host.py asserts >= 0.2) and the bf16 emulation by 0.005."""
    sd = {}
    for key, shape in sorted(param_shapes(cfg).items()):
        g = torch.Generator().manual_seed((int(seed) * 1000003 + zlib.crc32(key.encode())) % (1 << 31))
        z = torch.randn(shape, generator=g, dtype=torch.float32)
        if "embedding" in key:
            v = 0.5 * z
        elif "layer_norm" in key:
            v = 1.0 + 0.1 * z if key.endswith(".weight") else 0.1 * z
        elif key.endswith(".bias"):
            v = 0.1 * z
        else:
            v = z / math.sqrt(shape[1])
        sd[key] = v.to(torch.bfloat16).float()
    return sd


def unprefixed(sd: dict) -> dict:
    """The spelling of transformers 5.x's own state_dict(): no `text_model.` prefix."""
    return {k[len("text_model."):]: v for k, v in sd.items()}


def weights_checksum(sd: dict) -> int:
    c = 0
    for k in sorted(sd):
        c = zlib.crc32(sd[k].to(torch.bfloat16).contiguous().view(torch.int16).numpy().tobytes(), zlib.crc32(k.encode(), c))
    return c


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


ACTS = {"quick_gelu": quick_gelu, "gelu": gelu_erf}


def _ln(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def clip_ref(sd, cfg, ids, *, causal=True, act=None, emulate_bf16=False):
    """{"hidden_states": [L + 1 tensors (B, S, H)], "last_hidden_state", "pooler_output"} in fp64.
    sd in either key spelling; ids a (B, S) integer tensor."""
    sd = {(k if k.startswith("text_model.") else "text_model." + k): v.double() for k, v in sd.items()
          if not k.endswith("position_ids")}
    r = (lambda t: t.to(torch.bfloat16).double()) if emulate_bf16 else (lambda t: t)
    act = ACTS[act or cfg["hidden_act"]]
    eps, heads = cfg["layer_norm_eps"], cfg["num_attention_heads"]
    ids = torch.as_tensor(ids).long()
    B, S = ids.shape
    H = cfg["hidden_size"]
    d = H // heads
    E = "text_model.embeddings."
    x = r(sd[E + "token_embedding.weight"][ids] + sd[E + "position_embedding.weight"][:S])
    hidden = [x]
    mask = torch.full((S, S), float("-inf"), dtype=torch.float64).triu(1) if causal else torch.zeros(S, S, dtype=torch.float64)
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        lin = lambda t, n: t @ sd[p + n + ".weight"].T + sd[p + n + ".bias"]  # noqa: E731
        n1 = r(_ln(x, sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], eps))
        q, k, v = (r(lin(n1, f"self_attn.{n}_proj")).view(B, S, heads, d).transpose(1, 2) for n in "qkv")
        s = q @ k.transpose(-1, -2) * d ** -0.5 + mask
        a = r((torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, H))
        x = r(lin(a, "self_attn.out_proj") + x)
        n2 = r(_ln(x, sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], eps))
        m = r(act(lin(n2, "mlp.fc1")))
        x = r(lin(m, "mlp.fc2") + x)
        hidden.append(x)
    last = r(_ln(x, sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"], eps))
    eos = cfg.get("eos_token_id", 2)
    at = ids.argmax(-1) if eos == 2 else (ids == eos).int().argmax(-1)
    return {"hidden_states": hidden, "last_hidden_state": last, "pooler_output": last[torch.arange(B), at]}


def rel_l2(got, want) -> float:
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).norm() / want.norm()).item()


def fixture_ids(vocab_size: int = 512, seq: int = 77, seed: int = 0):
    """The four sequences of the fixture: a long prompt, one truncated at 77 (eos in the last
    slot), the empty prompt (bos, eos, pads) and one with an eos in the middle of the text.
    Word ids stay below BOS; the pad id is EOS, as in SD-1.5's tokenizer."""
    g = torch.Generator().manual_seed(seed)
    words = lambda n: torch.randint(3, min(vocab_size, BOS), (n,), generator=g).tolist()  # noqa: E731

    def row(body):
        ids = [BOS] + body[:seq - 2] + [EOS]
        return ids + [EOS] * (seq - len(ids))
    mid = words(20)
    mid[9] = EOS
    return torch.tensor([row(words(40)), row(words(seq + 10)), row([]), row(mid)], dtype=torch.long)
