"""CLIP text encoder and tokenizer, the parts that need no GPU.

The reference of the GPU parity tests (tests/clip_ref.py, fp64 plain torch) is pinned here to
transformers' OWN CLIPTextModel: to the outputs stored in tests/golden/clip_tiny.npz (written by
tests/golden/make_clip_golden.py with the transformers version recorded in the file) and, where
transformers is importable, to a live model — both hidden_act values, both state-dict key
spellings.  The fixture's conditioning (the causal mask must matter) is asserted, so the GPU
bar cannot hide a kernel that ignores the mask.  vdiff.CLIPTokenizer is held to the ids
transformers.CLIPTokenizer produced from the same vocab.json / merges.txt.  The loader, and the
argument checks of the two new argument values (VD_ATTN_CAUSAL, VD_ACT_QUICK_GELU), follow.
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import clip_ref
import vdiff
from vdiff import AnimateDiffPipeline, CLIPTextModel, CLIPTokenizer, MotionAdapter, UNetMotionModel, init_synthetic_
from vdiff.pipeline import SyntheticTextEncoder

GOLD = np.load(clip_ref.__file__.replace("clip_ref.py", "golden/clip_tiny.npz"))
CFG = json.loads(str(GOLD["config_json"]))
IDS = torch.from_numpy(GOLD["input_ids"])
STRINGS = json.loads(str(GOLD["strings_json"]))


@pytest.fixture(scope="module")
def tiny_sd():
    sd = clip_ref.synthetic_state_dict(CFG, 0)
    assert clip_ref.weights_checksum(sd) == int(GOLD["weights_checksum"]), "synthetic_state_dict changed: rewrite the fixture"
    return sd


@pytest.fixture(scope="module")
def tiny_ref(tiny_sd):
    return clip_ref.clip_ref(tiny_sd, CFG, IDS)


# ---------------------------------------------------------------- 1. the reference vs transformers
def test_fixture_inputs_are_the_documented_sequences():
    assert CFG == clip_ref.TINY and torch.equal(IDS, clip_ref.fixture_ids())
    B, E = clip_ref.BOS, clip_ref.EOS
    assert IDS.shape == (4, 77) and (IDS[:, 0] == B).all()
    assert (IDS[0] == E).nonzero()[0].item() == 41            # a long prompt
    assert (IDS[1] == E).nonzero()[0].item() == 76            # truncated: eos in the last slot
    assert IDS[2].tolist() == [B] + [E] * 76                  # the empty prompt
    assert (IDS[3] == E).nonzero()[0].item() == 10 and IDS[3, 21] == E and IDS[3, 20] != E  # eos mid-sequence


def test_clip_ref_reproduces_transformers_fixture(tiny_ref):
    """fp64 restatement vs transformers' fp32 outputs: 1e-5 rel-L2 per hidden state (measured
    0 / 3.1e-7 / 3.7e-7 / 3.8e-7 and 3.9e-7 on the last hidden state)."""
    assert GOLD["hidden_states"].shape == (CFG["num_hidden_layers"] + 1, 4, 77, CFG["hidden_size"])
    for i, h in enumerate(tiny_ref["hidden_states"]):
        e = clip_ref.rel_l2(h, torch.from_numpy(GOLD["hidden_states"][i]))
        print(f"hidden_states[{i}] rel-L2 vs transformers {e:.2e}")
        assert e <= 1e-5
    for k in ("last_hidden_state", "pooler_output"):
        e = clip_ref.rel_l2(tiny_ref[k], torch.from_numpy(GOLD[k]))
        print(f"{k} rel-L2 vs transformers {e:.2e}")
        assert e <= 1e-5
    # the pooled rows are the rows at the highest id (legacy eos_token_id == 2): the first eos here
    at = IDS.argmax(-1)
    assert at.tolist() == [41, 76, 1, 10]
    assert torch.equal(tiny_ref["pooler_output"], tiny_ref["last_hidden_state"][torch.arange(4), at])


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
@pytest.mark.parametrize("spelling", ["prefixed", "unprefixed"])
@pytest.mark.parametrize("eos", [2, clip_ref.EOS])
def test_clip_ref_reproduces_live_transformers(act, spelling, eos):
    transformers = pytest.importorskip("transformers")
    cfg = dict(CFG, hidden_act=act, eos_token_id=eos)
    sd = clip_ref.synthetic_state_dict(cfg, 3)
    model = transformers.CLIPTextModel(transformers.CLIPTextConfig(**cfg, bos_token_id=0, pad_token_id=1,
                                                                   attn_implementation="eager")).float().eval()
    own = model.state_dict()
    src = sd if next(iter(own)).startswith("text_model.") else clip_ref.unprefixed(sd)
    assert not [k for k in own if k not in src and not k.endswith("position_ids")]
    model.load_state_dict(src, strict=False)
    with torch.no_grad():
        out = model(input_ids=IDS, output_hidden_states=True)
    ref = clip_ref.clip_ref(sd if spelling == "prefixed" else clip_ref.unprefixed(sd), cfg, IDS)
    for h, w in zip(ref["hidden_states"], out.hidden_states):
        assert clip_ref.rel_l2(h, w) <= 1e-5
    assert clip_ref.rel_l2(ref["last_hidden_state"], out.last_hidden_state) <= 1e-5
    assert clip_ref.rel_l2(ref["pooler_output"], out.pooler_output) <= 1e-5
    # vdiff.CLIPTextModel takes the same dict in either spelling, into transformers' module names
    m = CLIPTextModel(cfg)
    m.load_state_dict(dict(sd if spelling == "prefixed" else clip_ref.unprefixed(sd),
                           **{("text_model." if spelling == "prefixed" else "") + "embeddings.position_ids":
                              torch.arange(77)[None]}))
    got = m.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


# ---------------------------------------------------------------- 2. conditioning
def test_fixture_is_sensitive_to_the_causal_mask(tiny_sd, tiny_ref):
    """Without the mask the output must move by >= 0.2 rel-L2 (measured 0.55), far above any bar the
    GPU parity test can take (it refuses a bar above 0.1).  The activation form is NOT visible end
    to end (erf-GELU for QuickGELU moves the output by ~2 %), so that epilogue is pinned at kernel
    level in tests/test_gpu_clip.py."""
    nc = clip_ref.clip_ref(tiny_sd, CFG, IDS, causal=False)
    e = clip_ref.rel_l2(nc["last_hidden_state"], tiny_ref["last_hidden_state"])
    print(f"no-mask vs causal rel-L2 {e:.3f}")
    assert e >= 0.2


def test_emulation_switch_only_rounds(tiny_sd, tiny_ref):
    """The bf16 emulation the GPU bar is built from: close to the reference, not equal to it."""
    em = clip_ref.clip_ref(tiny_sd, CFG, IDS, emulate_bf16=True)
    e = clip_ref.rel_l2(em["last_hidden_state"], tiny_ref["last_hidden_state"])
    print(f"bf16 emulation rel-L2 {e:.4f}")
    assert 1e-4 < e < 0.1 / 3


# ---------------------------------------------------------------- 3. tokenizer
@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("tok")
    (d / "vocab.json").write_text(str(GOLD["vocab_json"]), encoding="utf-8")
    (d / "merges.txt").write_text(str(GOLD["merges_txt"]), encoding="utf-8")
    return d


def test_tokenizer_matches_fixture(tok_dir):
    tok = CLIPTokenizer.from_pretrained(tok_dir)
    assert len(tok) == 256 + 256 + 60 + 2 and len(STRINGS) == 12
    want = torch.from_numpy(GOLD["token_ids"])
    got = tok(STRINGS, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert got.dtype == torch.long and got.shape == (len(STRINGS), 77)
    for s, a, b in zip(STRINGS, got, want):
        assert torch.equal(a, b), f"{s!r}: {a.tolist()} != {b.tolist()}"
    bos, eos = tok.bos_token_id, tok.eos_token_id
    assert (bos, eos, tok.pad_token_id) == (572, 573, 573)
    # the empty prompt: bos, eos, then pads
    assert tok("").input_ids[0].tolist() == [bos, eos] + [tok.pad_token_id] * 75
    # truncation keeps the final eos at position 76
    long = tok(STRINGS[-1]).input_ids[0]
    assert long[0] == bos and long[76] == eos and (long[1:76] != eos).all()
    assert len(tok.encode(STRINGS[-1], truncation=False)) > 77
    # case, whitespace runs and tabs / newlines collapse
    assert torch.equal(got[0], got[1])
    # one string, lists, and the unpadded forms
    assert tok("a cat", padding=False, return_tensors=None).input_ids == tok.encode("a cat")
    assert tok(["a cat", "a"], padding="longest").input_ids.shape == (2, len(tok.encode("a cat")))


def test_tokenizer_matches_live_transformers(tok_dir):
    transformers = pytest.importorskip("transformers")
    theirs = transformers.CLIPTokenizer.from_pretrained(str(tok_dir))
    ours = CLIPTokenizer.from_pretrained(tok_dir)
    extra = ["A man's hat; the men's hats... 'quoted' text", "1 22 333 a1b2", "tab\tand\nnewline  and   spaces",
             "x" * 200, "the the the the", "UPPER lower MiXeD"]
    for s in STRINGS + extra:
        want = theirs(s, padding="max_length", max_length=77, truncation=True)["input_ids"]
        assert ours(s).input_ids[0].tolist() == want, s


def test_tokenizer_pad_token_from_config(tok_dir, tmp_path):
    for f in ("vocab.json", "merges.txt"):
        (tmp_path / f).write_text((tok_dir / f).read_text(encoding="utf-8"), encoding="utf-8")
    (tmp_path / "special_tokens_map.json").write_text(json.dumps({"pad_token": {"content": "!", "lstrip": False}}))
    (tmp_path / "tokenizer_config.json").write_text(json.dumps({"model_max_length": 16, "pad_token": "!"}))
    tok = CLIPTokenizer.from_pretrained(tmp_path)
    ids = tok("a cat").input_ids[0].tolist()
    assert tok.pad_token_id == tok.encoder["!"] and len(ids) == 16 and ids[-1] == tok.pad_token_id
    with pytest.raises(FileNotFoundError, match="local directory"):
        CLIPTokenizer.from_pretrained("openai/clip-vit-large-patch14")


# ---------------------------------------------------------------- 4. loader
def _sd_dir(root, tiny_sd, tok_dir, with_text=True):
    from safetensors.torch import save_file
    from test_pretrained import ADAPTER_CFG, PNDM_CFG, UNET_CFG, _write
    unet = init_synthetic_(UNetMotionModel("tiny"), seed=0)
    sd = {k: v.float() for k, v in unet.state_dict().items()}
    motion = {k: v for k, v in sd.items() if ".motion_modules." in k}
    _write(root / "adapter", ADAPTER_CFG, motion)
    _write(root / "sd" / "unet", UNET_CFG, {k: v for k, v in sd.items() if k not in motion})
    _write(root / "sd" / "scheduler", PNDM_CFG, None, "scheduler_config.json")
    if with_text:
        enc = root / "sd" / "text_encoder"
        enc.mkdir(parents=True)
        (enc / "config.json").write_text(json.dumps(dict(CFG, architectures=["CLIPTextModel"], model_type="clip_text_model",
                                                         projection_dim=512, torch_dtype="float32")))
        save_file(dict(tiny_sd, **{"text_model.embeddings.position_ids": torch.arange(77)[None]}),
                  str(enc / "model.safetensors"))
        tk = root / "sd" / "tokenizer"
        tk.mkdir()
        for f in ("vocab.json", "merges.txt"):
            (tk / f).write_text((tok_dir / f).read_text(encoding="utf-8"), encoding="utf-8")
        (tk / "tokenizer_config.json").write_text(json.dumps({"model_max_length": 77, "pad_token": "<|endoftext|>"}))
    return root


def test_from_pretrained_loads_text_encoder_and_tokenizer(tmp_path, tiny_sd, tok_dir):
    root = _sd_dir(tmp_path, tiny_sd, tok_dir)
    adapter = MotionAdapter.from_pretrained(root / "adapter")
    pipe = AnimateDiffPipeline.from_pretrained(root / "sd", motion_adapter=adapter, device="cpu")
    assert isinstance(pipe.text_encoder, CLIPTextModel) and isinstance(pipe.tokenizer, CLIPTokenizer)
    got = pipe.text_encoder.state_dict()
    assert set(got) == set(tiny_sd)
    for k, v in tiny_sd.items():
        assert got[k].dtype == torch.bfloat16 and torch.equal(got[k].float(), v), k  # the weights are bf16-exact
    assert pipe.text_encoder.config["hidden_size"] == 128 and pipe.tokenizer.model_max_length == 77
    assert pipe.tokenizer("a cat").input_ids.shape == (1, 77)
    # the device path has no CPU fallback
    with pytest.raises(ValueError, match="GPU only"):
        pipe.text_encoder(pipe.tokenizer("a cat").input_ids)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        pipe.text_encoder(IDS, attention_mask=torch.ones_like(IDS))
    # hub names are refused as elsewhere; a missing weight is an error, not a half-loaded model
    with pytest.raises(FileNotFoundError, match="local directory"):
        vdiff.pretrained.load_text_encoder("openai/clip-vit-large-patch14", device="cpu")
    with pytest.raises(FileNotFoundError, match="local directory"):
        vdiff.pretrained.load_tokenizer("openai/clip-vit-large-patch14")
    (root / "sd" / "text_encoder" / "model.safetensors").unlink()
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        AnimateDiffPipeline.from_pretrained(root / "sd", motion_adapter=adapter, device="cpu")


def test_from_pretrained_without_the_two_folders_keeps_the_stub(tmp_path, tiny_sd, tok_dir):
    root = _sd_dir(tmp_path, tiny_sd, tok_dir, with_text=False)
    adapter = MotionAdapter.from_pretrained(root / "adapter")
    pipe = AnimateDiffPipeline.from_pretrained(root / "sd", motion_adapter=adapter, device="cpu")
    assert isinstance(pipe.text_encoder, SyntheticTextEncoder) and pipe.tokenizer is None
    # only one of the two: still the stub
    (root / "sd" / "tokenizer").mkdir()
    pipe = AnimateDiffPipeline.from_pretrained(root / "sd", motion_adapter=adapter, device="cpu")
    assert isinstance(pipe.text_encoder, SyntheticTextEncoder) and pipe.tokenizer is None
    assert pipe.encode_prompt("a cat", 2).shape == (2, 77, 64)
    with pytest.raises(ValueError, match="tokenizer"):
        AnimateDiffPipeline(pipe.unet, tokenizer=CLIPTokenizer.from_pretrained(tok_dir))


def test_named_configs():
    from vdiff.models.clip import CLIP_SD15 as sd15, CLIP_TINY as tiny
    assert (sd15["vocab_size"], sd15["hidden_size"], sd15["intermediate_size"], sd15["num_hidden_layers"],
            sd15["num_attention_heads"], sd15["max_position_embeddings"]) == (49408, 768, 3072, 12, 12, 77)
    assert tiny == clip_ref.TINY
    names = [n for n, _ in CLIPTextModel("tiny").named_modules()]
    for n in ("text_model.embeddings.token_embedding", "text_model.embeddings.position_embedding",
              "text_model.encoder.layers.2.self_attn.q_proj", "text_model.encoder.layers.0.self_attn.out_proj",
              "text_model.encoder.layers.1.layer_norm1", "text_model.encoder.layers.1.layer_norm2",
              "text_model.encoder.layers.0.mlp.fc1", "text_model.encoder.layers.0.mlp.fc2", "text_model.final_layer_norm"):
        assert n in names, n
    with pytest.raises(NotImplementedError):
        CLIPTextModel(dict(clip_ref.TINY, num_attention_heads=1))   # d = 128: no causal kernel
    with pytest.raises(NotImplementedError):
        CLIPTextModel(dict(clip_ref.TINY, hidden_act="relu"))


# ---------------------------------------------------------------- 5. ABI: the two new argument values
def _attention_ex(sq, skv, d, kv_div, kernel, batch=2):
    L = vdiff._lib.lib()
    p = 256  # aligned dummy operands: the argument checks read sizes and alignments only and launch nothing
    return L.vd_attention_ex(p, 128, p, 128, p, 128, p, 128, batch, 2, sq, skv, d, kv_div, C.c_float(0.125), 0, kernel,
                             None)


def test_causal_flag_argument_checks():
    from vdiff import ops
    assert ops.ATTN_CAUSAL == 0x100 and ops.ACT_QUICK_GELU == 4
    assert _attention_ex(77, 64, 64, 1, 0x100) == 1000        # sq != skv
    assert _attention_ex(77, 77, 64, 2, 0x100) == 1000        # kv_div != 1
    assert _attention_ex(77, 77, 64, 1, 0x200) == 1000        # an unknown flag bit
    assert _attention_ex(77, 77, 64, 1, 0x104) == 1000        # kernel code above 3 under the flag
    assert _attention_ex(77, 77, 64, 1, 4) == 1000            # ... and without it, as before
    assert _attention_ex(77, 77, 40, 1, 0x100) == 1001        # d = 40: no causal instance
    assert _attention_ex(77, 77, 160, 1, 0x101) == 1001


def test_quick_gelu_plans_like_gelu():
    from vdiff._lib import GemmDesc
    from vdiff.ops import _plan_query
    for M, N, K in [(154, 3072, 768), (154, 768, 3072), (154, 2304, 768), (65600, 160, 320), (2, 1280, 320),
                    (2048, 1280, 5120), (131072, 320, 320), (308, 512, 128)]:
        for path in (0, 1, 2, 3, 5, 6, 8, 9):
            plans = []
            for act in (3, 4):
                d = GemmDesc(a0=256, lda0=K, k0=K, a_mode=0, w=256, ldw=K, M=M, N=N, K=K, bias=256, act=act, out=256,
                             ldc=N, path=path)
                plans.append(_plan_query(d))
            assert plans[0] == plans[1] and plans[0][0] != 0, (M, N, K, path, plans)
    d = GemmDesc(a0=256, lda0=64, k0=64, a_mode=0, w=256, ldw=64, M=64, N=64, K=64, act=5, out=256, ldc=64)
    assert vdiff._lib.lib().vd_gemm(C.byref(d), None) == 1000  # the next act value is still refused
