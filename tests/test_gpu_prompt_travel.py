"""FreeNoise prompt travel on the device: vd_rows_eltwise op 9 (VD_ROWS_PROMPT_LERP) against the
fp64 reference and in poisoned frames, per-frame text through the tiny UNet's fast and module
paths, the DenoiseLoop, the ControlNet and the pipelines (tests/prompt_travel_ref.py is the
authority; the case is tests/prompt_travel_case.py's)."""
import numpy as np
import pytest
import torch

import clip_ref
import controlnet_ref
import memframe as mf
import prompt_travel_case as T
import prompt_travel_ref as P
from oracle import ddim_ref
from vdiff import (AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline, CLIPTextModel, CLIPTokenizer,
                   ControlNetConditioning, DDIMScheduler, DenoiseLoop, UNetMotionModel, init_synthetic_, ops)
from vdiff._lib import VdiffError
from vdiff.config import TINY, get_config

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
BAR, FN, rel_l2 = T.BAR, T.FN, T.rel_l2


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ---------------------------------------------------------------- op 9
#        B, F,   idx,            L,    C
CASES = [(1, 2, [0, 1], 1, 8),              # the minimal shape
         (2, 7, [0, 2, 6], 3, 24),          # several videos and unequal gaps
         (3, 9, [0, 1, 2, 8], 5, 72),       # adjacent keys, a non-power-of-two width
         (1, 33, [0, 32], 2, 8),            # one long gap
         (2, 1, [0], 4, 8),                 # K = 1
         (1, 256, [0, 100, 255], 1, 8),     # the cap
         (1, 6, [0, 5], 1030, 8),           # several workgroups per frame, ragged
         (1, 16, [0, 8, 15], 77, 64),       # the tiny model's shape
         (1, 8, [0, 3, 7], 77, 768)]        # the product width
ids = [f"B{c[0]}-F{c[1]}-K{len(c[2])}-L{c[3]}-C{c[4]}" for c in CASES]


def key_rows(B, K, L, C, seed, cancel=False):
    """Normal bf16 key rows [B * K * L, C]; cancel: key k + 1 is about minus key k (times 1 + 2^-6
    noise), so the interpolated value is far smaller than its operands and only the absolute slack
    of the bound covers the roundings."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, L, C, generator=g)
    if cancel:
        for k in range(1, K):
            x[:, k] = -x[:, k - 1] * (1 + torch.randn(B, L, C, generator=g) / 64)
    return x.to(BF).reshape(B * K * L, C)


def assert_lerp_bound(got, keys, idx, B, F, L, what=""):
    """|got - ref| <= 2^-8 |ref| + 2^-21 max(|a|, |b|) against lerp_ref in fp64: half a bf16 ulp of
    the result, plus at most five fp32 roundings (1 - w, (1 - w) a, the fused multiply-add, and the
    quotient w entering two products) of terms no larger than max(|a|, |b|).  Key frames bit for bit."""
    K, C = len(idx), keys.shape[1]
    k4 = keys.cpu().view(B, K, L, C)
    ref = P.lerp_ref(k4, idx, F)
    big = P.lerp_operands(k4, idx, F)
    g4 = got.cpu().view(B, F, L, C)
    err = (g4.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -21 * big
    bad = int((~(err <= bound)).sum())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"op 9 {what}: worst error / bound {worst:.3f}")
    assert bad == 0, f"{what}: {bad} of {ref.numel()} elements past the bound (worst {worst:.3f} x)"
    for k, f in enumerate(idx):
        assert torch.equal(bits(g4[:, f]), bits(k4[:, k])), f"{what}: key frame {f} is not key {k} bit for bit"
    return ref


@pytest.mark.parametrize("cancel", [False, True], ids=["normal", "cancelling"])
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_op9_matches_fp64(cuda, case, cancel):
    B, F, idx, L, C = case
    keys = key_rows(B, len(idx), L, C, seed=F * 100 + L, cancel=cancel).cuda()
    with mf.poisoned_empty():
        got = ops.prompt_lerp(keys, idx, B, F, L)
    assert got.shape == (B * F * L, C) and got.dtype == BF
    mf.assert_no_poison(got)
    assert_lerp_bound(got, keys, idx, B, F, L, f"{case}")
    # a video's result is the B = 1 call on its slice, bit for bit
    K = len(idx)
    for b in range(B):
        own = ops.prompt_lerp(keys[b * K * L:(b + 1) * K * L], idx, 1, F, L)
        assert torch.equal(bits(own), bits(got[b * F * L:(b + 1) * F * L])), b


@pytest.mark.parametrize("slack", [0, 8])
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_op9_framed(cuda, case, slack):
    """The key rows and out in poisoned frames (slack 8: both are column slices of wider buffers):
    no store outside out, every element of out written, nothing from beyond x in it, x only read."""
    B, F, idx, L, C = case
    keys = key_rows(B, len(idx), L, C, seed=7).cuda()
    xv, fx = mf.load2d(keys, col_slack=slack, name="keys")
    ov, fo = mf.framed((B * F * L, C), BF, cuda, col_slack=slack, name="out")
    got = ops.prompt_lerp(xv, idx, B, F, L, out=ov)
    torch.cuda.synchronize()
    assert got.data_ptr() == ov.data_ptr()
    mf.assert_all_intact(fx, fo)
    ref = assert_lerp_bound(ov.contiguous(), keys, idx, B, F, L, f"framed {case} slack {slack}")
    fo.assert_written(ref.reshape(B * F * L, C))
    assert torch.equal(bits(xv.contiguous()), bits(keys))


def test_op9_wrapper_refuses_with_device_operands(cuda):
    keys = key_rows(1, 3, 4, 8, seed=1).cuda()
    with pytest.raises(ValueError, match="strictly increasing"):
        ops.prompt_lerp(keys, [0, 6, 2], 1, 7, 4)
    with pytest.raises(ValueError, match="first frame index must be 0"):
        ops.prompt_lerp(keys, [1, 2, 6], 1, 7, 4)
    with pytest.raises(ValueError, match="last frame index must be 6"):
        ops.prompt_lerp(keys, [0, 2, 5], 1, 7, 4)
    with pytest.raises(ValueError, match="are not 1 videos x 3 key prompts x 5 tokens"):
        ops.prompt_lerp(keys, [0, 2, 6], 1, 7, 5)
    with pytest.raises(ValueError, match="out of shape"):
        ops.prompt_lerp(keys, [0, 2, 6], 1, 7, 4, out=torch.empty(7 * 4 + 1, 8, device=cuda, dtype=BF))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.prompt_lerp(keys.cpu(), [0, 2, 6], 1, 7, 4)
    with pytest.raises(ValueError, match="expected torch.bfloat16"):
        ops.prompt_lerp(keys.float(), [0, 2, 6], 1, 7, 4)
    with pytest.raises(VdiffError):  # out == x reaches the entry point, which refuses it before any launch
        ops.prompt_lerp(keys[:8], [0], 2, 1, 4, out=keys[:8])
    torch.cuda.synchronize()
    assert torch.equal(bits(ops.prompt_lerp(keys, [0, 2, 6], 1, 7, 4)[:4]), bits(keys[:4]))


def test_op9_einval_list_with_a_valid_device_table(cuda):
    """Every item of the VD_EINVAL list on DEVICE operands with a valid device index table, so each
    refusal is the named argument's own (on host operands the table's address alone refuses every
    call).  The valid call returns 0 before and after; no refused call writes out or leaves an
    error behind."""
    from vdiff._lib import lib
    h = lib()
    x = key_rows(1, 2, 2, 16, seed=3).cuda()            # K = 2 keys of L = 2 tokens, 16 columns
    out = torch.zeros(4, 16, device=cuda, dtype=BF)      # F = 2 frames
    idx = torch.tensor([0, 1, 0, 0], dtype=torch.int32, device=cuda)
    host = torch.tensor([0, 1], dtype=torch.int32)
    px, po, py = x.data_ptr(), out.data_ptr(), idx.data_ptr()

    def call(op=9, x=px, ldx=16, y=py, K=2, y_f32=1, L=2, F=2, rows=4, C=8, out=po, ldo=16):
        return h.vd_rows_eltwise(op, x, ldx, y, K, y_f32, L, F, rows, C, out, ldo, None)

    assert call() == 0
    torch.cuda.synchronize()
    want = out.clone()
    assert torch.equal(bits(want[:2, :8]), bits(x[:2, :8])) and torch.equal(bits(want[2:, :8]), bits(x[2:, :8]))
    assert not want[:, 8:].any()                         # a column slice: the rest of out is untouched
    out.zero_()
    bad = dict(bit8=dict(op=9 | (1 << 8)), bit16=dict(op=9 | (1 << 16)), K0=dict(K=0), K257=dict(K=257),
               F0=dict(F=0), F257=dict(F=257, rows=257 * 2), L0=dict(L=0), rows_ragged=dict(rows=5), rows0=dict(rows=0),
               C12=dict(C=12), C0=dict(C=0), x_null=dict(x=None), out_null=dict(out=None), x_misaligned=dict(x=px + 2),
               out_misaligned=dict(out=po + 2), out_is_x=dict(out=px), ldx_short=dict(C=16, ldx=8),
               ldo_short=dict(C=16, ldo=8), ldx_odd=dict(ldx=12), ldo_odd=dict(ldo=12), y_null=dict(y=None),
               y_misaligned=dict(y=py + 2), y_f32_0=dict(y_f32=0), y_host=dict(y=host.data_ptr()))
    for name, kw in bad.items():
        assert call(**kw) == 1000, name
    torch.cuda.synchronize()
    assert not out.any()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want))


# ---------------------------------------------------------------- the tiny UNet
@pytest.fixture(scope="module")
def tiny(cuda):
    m, sd = T.model()
    unet = UNetMotionModel("tiny")
    unet.load_state_dict(m.state_dict())
    unet = unet.to("cuda", BF).prepare()
    assert not unet.free_noise_enabled
    return dict(unet=unet, sd=sd)


@pytest.fixture(params=[True, False], ids=["free-noise", "plain"])
def fn(request, tiny):
    if request.param:
        tiny["unet"].enable_free_noise(*FN)
    yield request.param
    tiny["unet"].disable_free_noise()


def hooked(unet, call):
    """`call()` with a forward hook registered, so forward() takes the module path."""
    hook = unet.mid_block.register_forward_hook(lambda m, a, o: None)
    try:
        return call()
    finally:
        hook.remove()


# BAR (tests/prompt_travel_case.py, where both measurements are written down) = 1.3 x 0.01608, the
# device on the parent's path against its fp32 reference; the bf16 emulation sits at 0.01605.
# Measured against it with per-frame text (FreeNoise on / off): the fast path 0.01540 / 0.01558
# (F = 6), 0.01588 / 0.01570 (F = 7); the module path, which rounds every module's output to bf16,
# 0.02015 / 0.02010 and 0.02039 / 0.02020, where the same path with per-video text sits at 0.02019 /
# 0.02027 and 0.02038 / 0.02068 from its own reference.  Per-frame rows that repeat each video's text
# gave the per-video call's bits in every case.  The one BAR holds for both paths; the module path
# passes it with about 2.5 % to spare, so a change to that path's rounding shows here first, prompt
# travel or not.  A wrong frame or half costs >= 13 BAR
# (tests/test_prompt_travel_host.py).
@pytest.mark.parametrize("F", [6, 7])
@pytest.mark.parametrize("path", ["fast", "module"])
def test_tiny_unet_per_frame_text(tiny, fn, F, path):
    unet, c = tiny["unet"], T.case(F)
    x, pf, pv = c["x2"].cuda(), c["pf"].cuda(), c["pv"].cuda()
    run = (lambda e: unet(x, 961, encoder_hidden_states=e).sample.clone()) if path == "fast" else \
        (lambda e: hooked(unet, lambda: unet(x, 961, encoder_hidden_states=e).sample.clone()))
    ref = T.reference(F, fn)
    emu = rel_l2(T.reference(F, fn, "bf16"), ref)
    parent = rel_l2(run(pv), T.reference(F, fn, "fp32", "pv"))
    got = run(pf)
    err = rel_l2(got, ref)
    print(f"tiny UNet, per-frame text, {path} path, F={F}, FreeNoise {fn}: rel-L2 vs the fp32 reference {err:.5f}; "
          f"bf16 emulation {emu:.5f}; the parent's path (per-video text) vs its reference {parent:.5f}; BAR {BAR:.5f}")
    assert torch.isfinite(got).all()
    assert err < BAR, err
    # per-frame rows that repeat each video's text, against the per-video call
    rep = run(pv.repeat_interleave(F, 0))
    per_video = run(pv)
    d = rel_l2(rep, per_video)
    print(f"  repeated per-frame text vs per-video text: rel-L2 {d:.6f}, bit-equal {torch.equal(rep, per_video)}")
    assert d < BAR, d
    with pytest.raises(ValueError, match="one per frame"):
        unet(x, 961, encoder_hidden_states=pf[:F + 1])


# ---------------------------------------------------------------- the DenoiseLoop
def ddim():
    return DDIMScheduler(beta_schedule="linear", steps_offset=1, clip_sample=False)


@pytest.fixture(scope="module")
def loop3_ref(tiny):
    """Three DDIM steps of oracle.ddim_ref on unet_forward_per_frame, CFG 7.5, FreeNoise on: the
    fp32 reference with per-frame text, its bf16 emulation, and the fp32 one with per-video text."""
    acp = ddim_ref.alphas_cumprod()
    c = T.case(7)

    def loop(ehs, act):
        with torch.no_grad():
            return ddim_ref.denoise_loop(lambda xi, t, e: P.unet_forward_per_frame(tiny["sd"], TINY, xi, t, e, FN, act),
                                         c["lat"], ehs, 50, 7.5, acp, steps=3)

    return dict(pf=loop(c["pf"], "fp32"), pf_bf16=loop(c["pf"], "bf16"), pv=loop(c["pv"], "fp32"))


# LOOP_BAR = 1.3 x the larger of the emulated reference loop's distance from the fp32 reference loop
# with per-frame text (0.00639; 0.00618 on another host's CPU, another BLAS blocking) and the
# per-video device loop's distance from its own reference loop (0.00635): 1.3 x 0.0064.  Measured
# against it with per-frame text: 0.00611.  The two reference loops are 0.243 apart.
LOOP_BAR = 1.3 * 0.0064


def test_three_step_loop_per_frame_text(tiny, loop3_ref):
    unet, c = tiny["unet"], T.case(7)
    lat, pf, pv = c["lat"].cuda(), c["pf"].cuda(), c["pv"].cuda()
    unet.enable_free_noise(*FN)
    try:
        s = ddim()
        s.set_timesteps(50)
        out = {}
        for use_graph in (True, False):
            loop = DenoiseLoop(unet, s, lat, pf, 7.5, use_graph=use_graph).prime()
            if use_graph:
                assert loop.graph is not None, loop.graph_error
            assert loop.text_frames == 7 and loop.ehs_rows.shape == (2 * 7 * 77, 64)
            out[use_graph] = loop.run(3).clone()
            kv = next(iter(loop.kv_cache.values()))
            assert kv.shape[0] == 2 * 7 * 77 and len(loop.kv_cache) == len(unet.spatial_cross_attentions())
        assert torch.equal(bits(out[True]), bits(out[False]))  # the graph run and the eager run
        per_video = DenoiseLoop(unet, s, lat, pv, 7.5).prime()
        assert per_video.text_frames == 1 and per_video.ehs_rows.shape == (2 * 77, 64)
        first = per_video.run(3).clone()
        per_video.reset(lat)
        assert torch.equal(bits(per_video.run(3)), bits(first))  # unchanged from one run to the next
    finally:
        unet.disable_free_noise()
    emu = rel_l2(loop3_ref["pf_bf16"], loop3_ref["pf"])
    dev_pv = rel_l2(first, loop3_ref["pv"])
    err = rel_l2(out[True], loop3_ref["pf"])
    print(f"3-step loop, per-frame text + CFG: rel-L2 vs the reference loop {err:.6f}; emulated loop {emu:.6f}; "
          f"per-video device loop vs its reference loop {dev_pv:.6f}; LOOP_BAR {LOOP_BAR:.6f}; "
          f"per-frame vs per-video reference loops {rel_l2(loop3_ref['pv'], loop3_ref['pf']):.6f}")
    assert LOOP_BAR >= 1.3 * dev_pv, dev_pv  # LOOP_BAR is what its comment says (the device's side of it)
    assert err < LOOP_BAR, err


def test_loop_refusals_on_the_device(tiny):
    unet, c = tiny["unet"], T.case(7)
    s = ddim()
    s.set_timesteps(50)
    with pytest.raises(NotImplementedError, match="per-frame text.*ip_embeds"):
        DenoiseLoop(unet, s, c["lat"].cuda(), c["pf"].cuda(), 7.5, ip_embeds=torch.zeros(2, 4, 64, device="cuda"))
    with pytest.raises(NotImplementedError, match="per-frame text.*cfg_shard"):
        DenoiseLoop(unet, s, c["lat"].cuda(), c["pf"].cuda(), 7.5, cfg_shard=object())
    with pytest.raises(ValueError, match="per-frame form"):
        DenoiseLoop(unet, s, c["lat"].cuda(), c["pf"][:5].cuda(), 7.5)


# ---------------------------------------------------------------- the ControlNet
def test_controlnet_takes_per_frame_text(tiny):
    """guess mode under CFG: the ControlNet reads the conditional half's B * F * L rows.  Its
    residuals (the loop's own operands through forward_rows) with per-frame rows that repeat the
    text sit within BAR of the per-video ones; distinct per-frame text moves them by > 5 BAR.
    Measured (rel-L2 over all five residuals): repeated text 0, the per-video call's bits; distinct
    text 0.2448 = 11.7 BAR (the mid residual alone 0.2848)."""
    unet, c = tiny["unet"], T.case(7)
    cn = T.sharpened_(controlnet_ref.random_controlnet("tiny", seed=1)).to("cuda", BF).prepare()
    cond = torch.rand(1, 3, 7, 128, 128, generator=torch.Generator().manual_seed(5))
    s = ddim()
    s.set_timesteps(50)
    lat, pf, pv = c["lat"].cuda(), c["pf"].cuda(), c["pv"].cuda()

    def residuals(ehs):
        ctl = ControlNetConditioning(cn, cond, 1.0, True)
        loop = DenoiseLoop(unet, s, lat, ehs, 7.5, use_graph=False, control=ctl)
        assert loop.cn_cond_only and loop.cn_batch == 1
        te = ops.timestep_embed(loop.ts, unet.time_proj.num_channels, step_idx=loop.step_idx, batch=loop.Bu)
        ctx = cn.make_ctx(te[:1], loop.cn_ehs_rows, 1, 7, 77, kv_cache={})
        res = cn.forward_rows(loop.cn_x_in, loop.cn_cond_rows, 16, 16, ctx)
        loop.step()  # and the loop's own step runs with it
        torch.cuda.synchronize()
        assert torch.isfinite(loop.lat).all()
        return loop, torch.cat([a.t.float().flatten() for a in res]), res[-1].t.float()

    loop, all_pf, mid_pf = residuals(pf)
    assert loop.cn_ehs_rows.shape == (7 * 77, 64)
    assert torch.equal(bits(loop.cn_ehs_rows), bits(pf[7:].to(BF).reshape(7 * 77, 64)))  # the conditional half
    loop_v, all_pv, mid_pv = residuals(pv)
    assert torch.equal(bits(loop_v.cn_ehs_rows), bits(pv[1:].to(BF).reshape(77, 64)))
    _, all_rep, mid_rep = residuals(pv.repeat_interleave(7, 0))
    d_rep, d_pf = rel_l2(all_rep, all_pv), rel_l2(all_pf, all_pv)
    m_rep, m_pf = rel_l2(mid_rep, mid_pv), rel_l2(mid_pf, mid_pv)
    print(f"ControlNet residuals: repeated per-frame text vs per-video {d_rep:.6f} (mid {m_rep:.6f}), bit-equal "
          f"{torch.equal(all_rep, all_pv)}; distinct per-frame text vs per-video {d_pf:.4f} = {d_pf / BAR:.1f} BAR "
          f"(mid {m_pf:.4f})")
    assert d_rep < BAR and m_rep < BAR
    assert d_pf > 5 * BAR, d_pf


# ---------------------------------------------------------------- the pipelines
GOLD = np.load(clip_ref.__file__.replace("clip_ref.py", "golden/clip_tiny.npz"))
A, B_ = "a cat", "a dog on the moon"


@pytest.fixture(scope="module")
def clip_pipe(cuda, tmp_path_factory):
    """tests/test_gpu_clip.py's pipeline (the tiny CLIP text model and its tokenizer) on the
    sharpened tiny UNet, FreeNoise (4, 2)."""
    d = tmp_path_factory.mktemp("tok")
    (d / "vocab.json").write_text(str(GOLD["vocab_json"]), encoding="utf-8")
    (d / "merges.txt").write_text(str(GOLD["merges_txt"]), encoding="utf-8")
    tok = CLIPTokenizer.from_pretrained(d)
    cfg = dict(clip_ref.TINY, vocab_size=len(tok))
    enc = CLIPTextModel(cfg)
    enc.load_state_dict(clip_ref.synthetic_state_dict(cfg, 0))
    enc = enc.to(cuda, BF).prepare()
    ucfg = get_config("tiny")
    ucfg["cross_attention_dim"] = cfg["hidden_size"]
    unet = T.sharpened_(init_synthetic_(UNetMotionModel(ucfg), seed=0)).to(cuda, BF).prepare()
    pipe = AnimateDiffPipeline(unet, DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1,
                                                               clip_sample=False), text_encoder=enc, tokenizer=tok)
    pipe.enable_free_noise(context_length=4, context_stride=2)
    yield pipe, cfg
    pipe.disable_free_noise()


def test_pipeline_prompt_travel(clip_pipe, cuda):
    pipe, cfg = clip_pipe
    D = cfg["hidden_size"]
    lat = T.latents(7, 107)
    kw = dict(num_frames=7, height=128, width=128, num_inference_steps=3, guidance_scale=7.5, output_type="latent")
    travel = {0: A, 4: B_}
    # the embeddings: one batched encoder forward, then op 9 per side; the last key appended at frame 6
    calls, seen, encode = [], [], pipe.encode_prompt
    ops.ATTN_TAP = lambda q, k, v, batch, heads, sq, skv, d, scale: calls.append((batch, sq, skv))
    pipe.encode_prompt = lambda texts, *a, **k: seen.append((list(texts), encode(texts, *a, **k))) or seen[-1][1]
    try:
        pos, neg = pipe.encode_prompt_free_noise(travel, None, 7)
    finally:
        ops.ATTN_TAP = None
        del pipe.encode_prompt
    assert [c for c in calls if c[1] == c[2] == 77] == [(5, 77, 77)] * cfg["num_hidden_layers"]  # 2 negative + 3 positive
    assert len(seen) == 1 and seen[0][0] == ["", "", A, B_, B_]
    assert pos.shape == neg.shape == (1, 7, 77, D) and pos.dtype == BF
    k_neg, k_pos = seen[0][1][:2].contiguous(), seen[0][1][2:].contiguous()  # the encoder's key outputs
    assert_lerp_bound(pos.reshape(7 * 77, D), k_pos.reshape(3 * 77, D), [0, 4, 6], 1, 7, 77, "pipeline positive")
    assert_lerp_bound(neg.reshape(7 * 77, D), k_neg.reshape(2 * 77, D), [0, 6], 1, 7, 77, "pipeline negative")
    assert torch.equal(bits(pos[0, 6]), bits(k_pos[2])) and torch.equal(bits(pos[0, 4]), bits(k_pos[1]))
    two, _ = pipe.encode_prompt_free_noise(travel, None, 7, num_videos_per_prompt=2, do_classifier_free_guidance=False)
    assert _ is None and two.shape == (2, 7, 77, D) and torch.equal(bits(two), bits(pos.repeat(2, 1, 1, 1)))
    # the latents: a hand-built DenoiseLoop fed those embeddings, bit for bit
    got = pipe(prompt=travel, latents=lat.clone(), **kw).frames.clone()
    pipe.scheduler.set_timesteps(3)
    loop = DenoiseLoop(pipe.unet, pipe.scheduler, lat.cuda(), torch.cat([neg[0], pos[0]]), 7.5).prime()
    assert loop.graph is not None, loop.graph_error
    assert torch.equal(bits(got), bits(loop.run()))
    assert torch.isfinite(got).all()
    # precomputed per-frame embeddings are 4-D, [videos, F, 77, D]; 3-D ones stay per video, whatever their
    # row count; a per-video negative beside a per-frame positive is read by every frame
    pre = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat.clone(), **kw).frames
    assert torch.equal(bits(pre), bits(got))
    seven = pipe(prompt_embeds=pos[0], negative_prompt_embeds=neg[0], latents=lat.repeat(7, 1, 1, 1, 1), **kw).frames
    assert seven.shape[0] == 7  # seven videos, as before this form existed
    mixed = pipe(prompt=travel, negative_prompt_embeds=k_neg[:1], latents=lat.clone(), **kw).frames
    assert rel_l2(mixed, got) < BAR  # the positive keys come from an encoder batch of another size
    # against the one prompt
    one = pipe(prompt=A, latents=lat.clone(), **kw).frames
    d = rel_l2(got, one)
    print(f"pipeline latents, prompt travel vs prompt=a: rel-L2 {d:.4f} = {d / BAR:.1f} BAR")
    assert d > 5 * BAR, d
    same = pipe(prompt={0: A}, latents=lat.clone(), **kw).frames  # {0: a}: every frame reads a
    assert rel_l2(same, one) < BAR
    # a negative dict with keys of its own
    negd = pipe(prompt=travel, negative_prompt={0: "blurry", 3: "dark"}, latents=lat.clone(), **kw).frames
    assert torch.isfinite(negd).all() and not torch.equal(negd, got)


def test_video_to_video_accepts_the_dict(cuda):
    pipe = AnimateDiffVideoToVideoPipeline.from_config("tiny")
    lat = T.latents(7, 107)[:, :, :, :8, :8].contiguous()
    kw = dict(latents=lat, num_inference_steps=3, strength=0.7, guidance_scale=7.5, output_type="latent")
    with pytest.raises(NotImplementedError, match="prompt dict.*enable_free_noise"):
        pipe(prompt={0: A, 4: B_}, **kw)
    pipe.enable_free_noise(context_length=4, context_stride=2)
    try:
        got = pipe(prompt={0: A, 4: B_}, **kw).frames.clone()
        pos, neg = pipe.encode_prompt_free_noise({0: A, 4: B_}, None, 7)
        pre = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, **kw).frames
        one = pipe(prompt=A, **kw).frames
    finally:
        pipe.disable_free_noise()
    assert got.shape == lat.shape and torch.isfinite(got).all()
    assert torch.equal(bits(got), bits(pre)) and not torch.equal(got, one)


def test_controlnet_pipeline_accepts_the_dict(cuda):
    """AnimateDiffControlNetPipeline inherits the call: the dict reaches its loop, ControlNet included."""
    from vdiff import AnimateDiffControlNetPipeline
    pipe = AnimateDiffControlNetPipeline.from_config("tiny", vae=None)
    frames = torch.rand(7, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    kw = dict(num_frames=7, height=64, width=64, num_inference_steps=2, guidance_scale=7.5, output_type="latent",
              latents=T.latents(7, 107)[:, :, :, :8, :8].contiguous(), conditioning_frames=frames, guess_mode=True)
    pipe.enable_free_noise(context_length=4, context_stride=2)
    try:
        got = pipe(prompt={0: A, 4: B_}, **kw).frames.clone()
        pos, neg = pipe.encode_prompt_free_noise({0: A, 4: B_}, None, 7)
        pre = pipe(prompt_embeds=pos, negative_prompt_embeds=neg, **kw).frames
        one = pipe(prompt=A, **kw).frames
    finally:
        pipe.disable_free_noise()
    assert torch.isfinite(got).all() and torch.equal(bits(got), bits(pre)) and not torch.equal(got, one)
    assert pipe._control is None


def test_pipeline_refusals_on_the_device(cuda):
    from test_ip_adapter_host import synthetic_adapter
    pipe = AnimateDiffPipeline.from_config("tiny", vae=None)
    pipe.load_ip_adapter(synthetic_adapter(pipe.unet, n=4, clip_dim=48, scale=3.0))
    kw = dict(num_frames=7, height=64, width=64, num_inference_steps=2, output_type="latent")
    travel = {0: A, 4: B_}
    with pytest.raises(NotImplementedError, match="prompt dict.*enable_free_noise"):  # FreeNoise disabled
        pipe(prompt=travel, **kw)
    with pytest.raises(NotImplementedError, match="prompt_interpolation_callback"):
        pipe.enable_free_noise(prompt_interpolation_callback=lambda *a: None)
    assert not pipe.free_noise_enabled
    pipe.enable_free_noise(context_length=4, context_stride=2)
    try:
        with pytest.raises(NotImplementedError, match="IP-Adapter"):
            pipe(prompt=travel, ip_adapter_image_embeds=torch.zeros(2, 1, 48), **kw)
        with pytest.raises(NotImplementedError, match="cfg_shard"):
            pipe(prompt=travel, cfg_shard=object(), **kw)
        out = pipe(prompt=travel, **kw).frames  # the adapter loaded, no image prompt: text alone
        assert torch.isfinite(out).all()
    finally:
        pipe.disable_free_noise()
