"""The CLIP text encoder on the MI355X: the causal instances of the flash kernel, the QuickGELU
GEMM epilogue on every kernel family that carries a pointwise activation, vdiff.CLIPTextModel
against the fp64 reference (tests/clip_ref.py, itself pinned to transformers' CLIPTextModel by
tests/test_clip_host.py) and the pipeline's prompt -> embeddings path.

Operands of the kernel tests sit in poisoned frames (tests/memframe.py): guard rows and columns
must stay 0xFF and every output element must be written, as tests/test_gpu_memframe.py does for
the entry points its COVERAGE table names.
"""

import numpy as np
import pytest
import torch

import clip_ref
import memframe as mf
from memframe import close_bf16, close_f32
from vdiff import AnimateDiffPipeline, CLIPTextModel, CLIPTokenizer, DDIMScheduler, UNetMotionModel, init_synthetic_, ops
from vdiff._lib import GemmDesc, check, lib
from vdiff.config import get_config

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
LOG2E = 1.4426950408889634
GOLD = np.load(clip_ref.__file__.replace("clip_ref.py", "golden/clip_tiny.npz"))
IDS = torch.from_numpy(GOLD["input_ids"])


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def rnd(*shape, std=1.0, g=None):
    return (torch.randn(*shape, device="cuda", generator=g) * std).to(BF)


def causal_sdpa_ref(q, k, v, batch, heads, s, d, scale=None):
    """fp64 causal SDPA of the bf16 operands, rows [(b, s)][heads * d]."""
    q, k, v = (t.double().reshape(batch, s, heads, d).transpose(1, 2) for t in (q, k, v))
    sc = q @ k.transpose(-1, -2) * (d ** -0.5 if scale is None else scale)
    sc = sc + torch.full((s, s), float("-inf"), dtype=torch.float64, device=sc.device).triu(1)
    return (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(batch * s, heads * d)


def framed_attention(qkv, batch, heads, s, d, *, out_f32=False, kernel="auto", scale=None, causal=True):
    """ops.attention on column slices of ONE framed fused-QKV buffer into a framed output; the
    frames are checked (guards intact, output written) before the output is returned."""
    C = heads * d
    buf, fin = mf.load2d(qkv, col_slack=8, name="qkv")
    out, fout = mf.framed((batch * s, C), F32 if out_f32 else BF, qkv.device, col_slack=8, name="out")
    ops.attention(buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:], batch, heads, s, s, d, scale=scale, out=out,
                  out_f32=out_f32, kernel=kernel, causal=causal)
    torch.cuda.synchronize()
    mf.assert_all_intact(fin, fout)
    fout.assert_written()
    assert torch.equal(buf, qkv), "the kernel wrote into its inputs"
    return out.clone()


# ---------------------------------------------------------------- 1. causal attention vs fp64
# d = 64 (QBLK 2: 128 queries per workgroup, 32 per wave, 64-key tiles): a single key, a partial
# query fragment, a tile edge (63 / 64 / 65), SD-1.5's 77, a ragged second tile, a second
# workgroup whose first tiles are full and whose last is the diagonal (129, 200), >= 3 query
# blocks with tiles skipped for the first ones (257).  d = 32: the same kernel at the other
# contraction width, and 1030 rows, which take the QBLK = 4 launch (sq >= 1024).
SHAPES = [(64, s) for s in (1, 15, 16, 17, 63, 64, 65, 77, 128, 129, 200, 257)] + [(32, s) for s in (77, 130, 1030)]


@pytest.mark.parametrize("d,s", SHAPES)
def test_causal_attention_matches_fp64(cuda, d, s):
    """bf16 output on N(0, 1.5^2) operands within close_bf16 of fp64 causal SDPA; fp32 output within
    close_f32 (rtol 1e-3 / atol 1e-4, the bar include/vdiff.h states for vd_attention_f32) on the
    operands that bar is stated for — integer q / k at the unit scale, so every P is an exact
    power of two and only the fp32 accumulation is measured, as tests/test_gpu_memframe.py's
    test_attention does.  Both kernel codes ("auto", "v1") run."""
    batch, heads = 2, 2
    C = heads * d
    g = gen(1000 * d + s)
    qkv = rnd(batch * s, 3 * C, std=1.5, g=g)
    want = causal_sdpa_ref(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], batch, heads, s, d)
    qi = torch.cat([torch.randint(-1, 2, (batch * s, 2 * C), device=cuda, generator=g).to(BF), rnd(batch * s, C, g=g)], 1)
    want_i = causal_sdpa_ref(qi[:, :C], qi[:, C:2 * C], qi[:, 2 * C:], batch, heads, s, d, scale=1 / LOG2E)
    for kernel in ("auto", "v1"):
        close_bf16(framed_attention(qkv, batch, heads, s, d, kernel=kernel), want)
        # softmax in base 2 of integer scores: scale = 1 / log2(e) makes the kernel's c exactly 1
        got = framed_attention(qi, batch, heads, s, d, out_f32=True, kernel=kernel, scale=1 / LOG2E)
        close_f32(got, want_i)


# ---------------------------------------------------------------- 2. future keys cannot matter
@pytest.mark.parametrize("d,s", [(64, 77), (64, 200), (32, 200)])
def test_future_keys_do_not_reach_the_output(cuda, d, s):
    batch, heads = 2, 2
    C = heads * d
    g = gen(7 * s + d)
    qkv = rnd(batch * s, 3 * C, std=1.5, g=g)
    base = framed_attention(qkv, batch, heads, s, d)
    assert torch.equal(framed_attention(qkv, batch, heads, s, d), base), "two identical runs differ"
    pos = torch.arange(batch * s, device=cuda) % s
    for i in (0, 40, 63, 64, s - 2):
        mod = qkv.clone()
        mod[pos > i, C:] = rnd(int((pos > i).sum()), 2 * C, std=3.0, g=g)   # K and V rows j > i, both batches
        got = framed_attention(mod, batch, heads, s, d)
        assert torch.equal(got[pos <= i], base[pos <= i]), f"keys after {i} changed output rows <= {i}"
        assert not torch.equal(got[pos > i], base[pos > i])                # ... and the later rows do see them


# ---------------------------------------------------------------- 3. non-causal is untouched
@pytest.mark.parametrize("d,s", [(32, 300), (64, 1024), (160, 64)])
def test_non_causal_bits_equal_vd_attention(cuda, d, s):
    """ops.attention(causal=False) goes through vd_attention_ex with the flag clear: the same bits
    as vd_attention, the entry point that has no flag at all."""
    batch, heads = 2, 3
    C = heads * d
    torch.manual_seed(3)
    qkv = rnd(batch * s, 3 * C, std=1.5)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    got = ops.attention(q, k, v, batch, heads, s, s, d, causal=False)
    ref = torch.empty_like(got)
    check(lib().vd_attention(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                             ref.data_ptr(), ref.stride(0), batch, heads, s, s, d, 1, d ** -0.5,
                             torch.cuda.current_stream().cuda_stream), "vd_attention")
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    # and it is not the causal answer
    if d in (32, 64):
        assert not torch.equal(ops.attention(q, k, v, batch, heads, s, s, d, causal=True), ref)


# ---------------------------------------------------------------- 4. QuickGELU epilogue
# (path, M, N, K, out_f32, expected (kernel, split > 1)): every family with a pointwise act at the
# small shapes their own tests use, v8 at its GELU shape, one split-K launch through
# gemm_splitk.hip's reduce epilogue, and the encoder's three GEMM shapes under the automatic plan.
QG_CASES = [
    ("v1", 1, 300, 320, 640, True, 1), ("v2", 2, 1000, 160, 128, True, 2), ("v3", 3, 300, 512, 128, True, 3),
    ("v5", 5, 300, 128, 96, True, 5), ("v6", 6, 100, 320, 2560, True, 6), ("v9", 9, 2, 1280, 320, True, 9),
    ("v9-16", 9, 16, 4096, 2560, False, 9), ("v8", 8, 65600, 160, 320, False, 8), ("splitk", 0, 1024, 1280, 2560, True, 2),
    ("clip-qkv", 0, 154, 2304, 768, True, None), ("clip-fc1", 0, 154, 3072, 768, False, None),
    ("clip-fc2", 0, 154, 768, 3072, True, None),
]


@pytest.mark.parametrize("name,path,M,N,K,out_f32,kern", QG_CASES, ids=[c[0] for c in QG_CASES])
def test_quick_gelu_epilogue(cuda, name, path, M, N, K, out_f32, kern):
    """act 4 = x * sigmoid(1.702 x) on accumulator + bias, against fp64 of the bf16 operands:
    close_f32 where the path writes fp32, close_bf16 otherwise.  First the case must be able to
    tell the activations apart: on >= 10 % of the elements |quick_gelu - gelu_erf| of the reference
    pre-activations exceeds the tolerance the output is held to (pre-activations ~ N(-1, 1.5^2):
    the two forms differ most, by 0.02, around x = -2).  Families documented bit-equal (v8 / v2,
    v9 / v1) are bit-equal for act 4 too."""
    g = gen(M + N + K)
    a = rnd(M, K, g=g)
    w = rnd(N, K, std=1.4 * K ** -0.5, g=g)
    b = (torch.randn(N, device=cuda, generator=g) * 0.5 - 1.0).contiguous()
    pre = a.double() @ w.double().T + b.double()
    want, other = clip_ref.quick_gelu(pre), clip_ref.gelu_erf(pre)
    if out_f32:
        tol = 1e-4 + 1e-3 * want.abs()
    else:
        tol = want.abs() / 128 + 2e-3 * want.abs().max()
    frac = ((want - other).abs() > tol).double().mean().item()
    print(f"{name}: pre-activation std {pre.std().item():.2f}, {100 * frac:.1f} % of elements tell the activations apart")
    assert frac >= 0.10, "ill-conditioned case: a GELU epilogue would pass"

    def launch(p):
        av, fa = mf.load2d(a, col_slack=8, name="a")
        wv, fw = mf.load2d(w, col_slack=8, name="w")
        out, fo = mf.framed((M, N), F32 if out_f32 else BF, cuda, col_slack=8, name="out")
        with ops.gemm_plan(path=p):
            d = GemmDesc(a0=av.data_ptr(), lda0=av.stride(0), k0=K, a_mode=0, w=wv.data_ptr(), ldw=wv.stride(0), M=M,
                         N=N, K=K, bias=b.data_ptr(), act=ops.ACT_QUICK_GELU, out=out.data_ptr(), ldc=out.stride(0),
                         out_f32=int(out_f32))
            plan = ops.gemm_plan_of(d)
            with mf.poisoned_empty():  # the split-K workspace starts as NaN bytes
                ops.gemm(av, wv, bias=b, act=ops.ACT_QUICK_GELU, out=out, out_f32=out_f32)
        torch.cuda.synchronize()
        mf.assert_all_intact(fa, fw, fo)
        fo.assert_written(want)
        return out.clone(), plan

    got, plan = launch(path)
    print(f"{name}: plan {plan}")
    if kern is not None:
        assert plan[0] == kern, f"{name}: the plan ran kernel {plan[0]}, not {kern}"
    if name == "splitk":
        assert plan[1] > 1, "not a split-K launch"
    (close_f32 if out_f32 else close_bf16)(got, want)
    twin = {8: 2, 9: 1}.get(path)
    if twin is not None:
        ref, tplan = launch(twin)
        assert tplan[0] == twin and torch.equal(got, ref), f"v{path} != v{twin} bits for act 4"


# ---------------------------------------------------------------- 5. model parity
SD15_1K = dict(clip_ref.TINY, vocab_size=1000, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
               num_attention_heads=12)
MODEL_CASES = {"tiny": dict(clip_ref.TINY), "tiny-4heads": dict(clip_ref.TINY, num_attention_heads=4),
               "tiny-gelu-eos": dict(clip_ref.TINY, hidden_act="gelu", eos_token_id=clip_ref.EOS), "sd15-1k": SD15_1K}
BAR_FACTOR = 3.0   # device deviation <= 3 x the emulated one: summation order, bf16 P, hardware exp2 / rcp
BAR_CEILING = 0.1  # half of the 0.2 the causal mask must move the output by (tests/test_clip_host.py)


def device_model(cfg, sd, cuda):
    m = CLIPTextModel(cfg)
    m.load_state_dict(sd)
    return m.to(cuda, BF).prepare()


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_model_parity(cuda, case):
    """rel-L2 of the last hidden state against the fp64 reference, held to 3 x the deviation of the
    CPU bf16 emulation of the same case (computed here, never taken from the device).  Measured
    (emulated / device): see DESIGN.md §8's table."""
    cfg = MODEL_CASES[case]
    sd = clip_ref.synthetic_state_dict(cfg, 0)
    ref = clip_ref.clip_ref(sd, cfg, IDS)
    emu = clip_ref.clip_ref(sd, cfg, IDS, emulate_bf16=True)
    e_emu = clip_ref.rel_l2(emu["last_hidden_state"], ref["last_hidden_state"])
    bar = BAR_FACTOR * e_emu
    assert 0 < bar <= BAR_CEILING, f"ill-conditioned: the bar {bar:.3f} is above {BAR_CEILING}"
    m = device_model(cfg, sd, cuda)
    ids = IDS.to(cuda)
    out = m(ids, output_hidden_states=True)
    torch.cuda.synchronize()
    assert out.last_hidden_state.shape == (4, 77, cfg["hidden_size"]) and out.last_hidden_state.dtype == BF
    e_dev = clip_ref.rel_l2(out.last_hidden_state, ref["last_hidden_state"])
    print(f"PARITY {case}: emulated {e_emu:.5f} device {e_dev:.5f} ratio {e_dev / e_emu:.2f} bar {bar:.5f}")
    assert torch.isfinite(out.last_hidden_state.float()).all()
    assert e_dev <= bar
    assert out[0] is out.last_hidden_state and len(out.hidden_states) == cfg["num_hidden_layers"] + 1
    # per layer, each against its own emulated deviation
    for i, (h, r, e) in enumerate(zip(out.hidden_states, ref["hidden_states"], emu["hidden_states"])):
        e_h, b_h = clip_ref.rel_l2(h, r), BAR_FACTOR * clip_ref.rel_l2(e, r)
        assert e_h <= b_h, f"hidden_states[{i}]: {e_h:.5f} > {b_h:.5f}"
    if case == "tiny":  # ... and against transformers' own hidden states (the fixture), at the same bar
        for i, h in enumerate(out.hidden_states):
            e_h = clip_ref.rel_l2(h, torch.from_numpy(GOLD["hidden_states"][i]))
            print(f"PARITY tiny hidden_states[{i}] vs transformers {e_h:.5f}")
            assert e_h <= bar
        assert clip_ref.rel_l2(out.last_hidden_state, torch.from_numpy(GOLD["last_hidden_state"])) <= bar
    # the pooled rows are rows of the last hidden state, exactly
    eos = cfg["eos_token_id"]
    at = IDS.argmax(-1) if eos == 2 else (IDS == eos).int().argmax(-1)
    assert at.tolist() == [41, 76, 1, 10]
    assert torch.equal(out.pooler_output.cpu(), out.last_hidden_state.cpu()[torch.arange(4), at])
    # tuple form
    tup = m(ids, return_dict=False)
    assert torch.equal(tup[0], out.last_hidden_state) and torch.equal(tup[1], out.pooler_output)
    # a later token cannot change an earlier row: prefixes are bit-identical
    for cut in (1, 40, 64):
        ids2 = ids.clone()
        ids2[:, cut:] = torch.randint(3, 500, ids2[:, cut:].shape, device=cuda, generator=gen(cut))
        o2 = m(ids2).last_hidden_state
        assert torch.equal(o2[:, :cut], out.last_hidden_state[:, :cut]), f"rows < {cut} depend on later tokens"
        assert not torch.equal(o2[:, cut:], out.last_hidden_state[:, cut:])


def test_model_refuses_what_it_does_not_do(cuda):
    m = device_model(clip_ref.TINY, clip_ref.synthetic_state_dict(clip_ref.TINY, 0), cuda)
    with pytest.raises(ValueError, match="GPU only"):
        m(IDS)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        m(IDS.to(cuda), attention_mask=torch.ones_like(IDS).to(cuda))
    short = m(IDS[:, :20].to(cuda)).last_hidden_state   # any S <= 77
    assert torch.equal(short, m(IDS.to(cuda)).last_hidden_state[:, :20])


# ---------------------------------------------------------------- 6. pipeline
@pytest.fixture(scope="module")
def clip_pipe(cuda, tmp_path_factory):
    d = tmp_path_factory.mktemp("tok")
    (d / "vocab.json").write_text(str(GOLD["vocab_json"]), encoding="utf-8")
    (d / "merges.txt").write_text(str(GOLD["merges_txt"]), encoding="utf-8")
    tok = CLIPTokenizer.from_pretrained(d)
    cfg = dict(clip_ref.TINY, vocab_size=len(tok))
    enc = device_model(cfg, clip_ref.synthetic_state_dict(cfg, 0), cuda)
    ucfg = get_config("tiny")
    ucfg["cross_attention_dim"] = cfg["hidden_size"]
    unet = init_synthetic_(UNetMotionModel(ucfg), seed=0).to(cuda, BF).prepare()
    sched = DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)
    return AnimateDiffPipeline(unet, sched, text_encoder=enc, tokenizer=tok), cfg


def test_pipeline_prompt_equals_prompt_embeds(clip_pipe, cuda):
    pipe, cfg = clip_pipe
    kw = dict(num_frames=2, height=64, width=64, num_inference_steps=3, guidance_scale=7.5, output_type="latent")
    lat = torch.randn(1, 4, 2, 8, 8, generator=torch.Generator().manual_seed(5))
    both = pipe.encode_prompt(["", "a cat"], 2)          # the negative prompt defaults to ""
    assert both.shape == (2, 77, cfg["hidden_size"]) and both.dtype == BF
    a = pipe(prompt="a cat", latents=lat.clone(), **kw).frames
    b = pipe(prompt_embeds=both[1:], negative_prompt_embeds=both[:1], latents=lat.clone(), **kw).frames
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    c = pipe(prompt="a dog on the moon", latents=lat.clone(), **kw).frames
    assert not torch.equal(a, c), "the latents do not depend on the prompt"
    # clip_skip: the final LayerNorm of an earlier hidden state
    ids = pipe.tokenizer(["a cat"]).input_ids.to(cuda)
    hs = pipe.text_encoder(ids, output_hidden_states=True).hidden_states
    skip = pipe.encode_prompt("a cat", 1, clip_skip=1)
    assert torch.equal(skip, pipe.text_encoder.text_model.final_layer_norm(hs[-2]))
    assert torch.equal(pipe.encode_prompt("a cat", 1, clip_skip=0), pipe.encode_prompt("a cat", 1))
    assert not torch.equal(skip, pipe.encode_prompt("a cat", 1))


def test_pipeline_encodes_all_prompts_in_one_forward(clip_pipe, cuda):
    """A list of prompts, positive and negative together, is ONE batched encoder forward: the
    causal attention (sq == skv == 77) is launched once per layer, with the whole batch."""
    pipe, cfg = clip_pipe
    calls = []
    ops.ATTN_TAP = lambda q, k, v, batch, heads, sq, skv, d, scale: calls.append((batch, sq, skv))
    try:
        emb = pipe.encode_prompt(["a cat", "a dog", "the sea at night"], 3)
        enc_calls = [c for c in calls if c[1] == c[2] == 77]
        assert enc_calls == [(3, 77, 77)] * cfg["num_hidden_layers"] and emb.shape[0] == 3
        calls.clear()
        pipe(prompt=["a cat", "a dog"], negative_prompt="blurry", num_frames=2, height=64, width=64,
             num_inference_steps=1, output_type="latent", use_graph=False)
        enc_calls = [c for c in calls if c[1] == c[2] == 77]
        assert enc_calls == [(4, 77, 77)] * cfg["num_hidden_layers"]
    finally:
        ops.ATTN_TAP = None
