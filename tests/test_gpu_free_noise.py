"""FreeNoise on the MI355X: vd_rows_eltwise ops 4 (window gather) and 5 (weighted window merge)
against an fp64 restatement, framed by tests/memframe.py, and enable_free_noise end to end on the
tiny UNet (fast path, module path, hipGraph loop, pipeline, past the 32-frame cap) and on the
full config's level-1 motion module (the windowed batch on the fused QKV attention kernel).

Kernel bar (set by the arithmetic, not by what the kernel gives): gather is bit-exact; merge is
|got - ref| <= 2^-8 |ref| + 4e-6 max|x| — one bf16 rounding plus at most 34 fp32 operations of
2^-24 each (32 fmaf, the division, one spare) on sums bounded by max|x|.

Model bar: see BAR below.
"""
import pytest
import torch

import free_noise_ref as R
import memframe as mf
from oracle import ddim_ref, unet_ref
from vdiff import AnimateDiffPipeline, DDIMScheduler, DenoiseLoop, UNetMotionModel, init_synthetic_, ops
from vdiff._lib import VdiffError
from vdiff.config import TINY
from vdiff.models.blocks import AnimateDiffTransformer3D, Ctx
from vdiff.models.layers import Act, prepare_tree

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
FREEU = (0.9, 0.2, 1.2, 1.4)

# (B, F, L, s, hw, C)
SMALL = [(1, 5, 4, 1, 1, 8),       # maximal overlap
         (2, 7, 4, 2, 3, 8),       # tail of 1
         (2, 9, 4, 3, 2, 24),      # tail of 2, s does not divide L
         (1, 8, 4, 4, 5, 40),      # no overlap
         (1, 28, 16, 4, 2, 8),     # the default: a frame under 4 windows
         (2, 20, 16, 4, 4, 64),
         (1, 33, 32, 1, 1, 8),     # 32-fold overlap
         (1, 6, 4, 2, 1030, 8)]    # several workgroups per frame, ragged
PRODUCT = [(2, 32, 16, 4, 1024, 320), (2, 32, 16, 4, 256, 640), (2, 32, 16, 4, 64, 1280)]
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


def rel_l2(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).norm() / want.norm()).item()


def rand_rows(rows, c, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(rows, c, device="cuda", generator=g).to(BF)


def weights_dev(L, scheme):
    return torch.tensor(R.frame_weights(L, scheme), dtype=F32, device="cuda")


def gather_ref(x, B, F, hw, L, s):
    """The window rows of x, by indexing (exact)."""
    idx, _ = R.frame_indices(F, L, s)
    v = x.reshape(B, F, hw, -1)
    return torch.stack([v[:, a:e] for a, e in idx], 1).reshape(B * len(idx) * L * hw, -1)


def merge_ref(xw, wt, B, F, hw, L, s):
    """fp64 restatement of diffusers' accumulation over the window rows xw (the reference's
    merge_windows on the rows' layout), with the fp32 weights the device reads."""
    idx, tail = R.frame_indices(F, L, s)
    v = xw.double().reshape(B, len(idx), L, hw, -1)
    w = wt.double().to(xw.device)[None, :, None, None]
    acc = torch.zeros(B, F, hw, v.shape[-1], dtype=torch.float64, device=xw.device)
    cnt = torch.zeros(1, F, 1, 1, dtype=torch.float64, device=xw.device)
    for i, (a, e) in enumerate(idx):
        if tail and i == len(idx) - 1:
            acc[:, -tail:] += v[:, i, -tail:] * w[:, -tail:]
            cnt[:, -tail:] += w[:, -tail:]
        else:
            acc[:, a:e] += v[:, i] * w
            cnt[:, a:e] += w
    return (acc / cnt).reshape(B * F * hw, -1)


def assert_within_bar(got, ref, xmax, what=""):
    err = (got.double() - ref.to(got.device)).abs()
    bound = 2.0 ** -8 * ref.to(got.device).abs() + 4e-6 * xmax
    bad = int((~(err <= bound)).sum())  # a NaN is out of tolerance
    worst = (err - bound).max().item()
    print(f"window_merge {what}: max|err| {err.max().item():.3e}, max(err - bound) {worst:.3e}")
    assert bad == 0, f"{what}: {bad} of {ref.numel()} elements past the bar (worst by {worst:.3e})"


def sliced_in(x):
    """x as a view with ldx > C inside a NaN-filled wider buffer."""
    c = x.shape[1]
    wide = torch.full((x.shape[0], c + 16), float("nan"), dtype=BF, device="cuda")
    wide[:, 8:8 + c] = x
    return wide[:, 8:8 + c]


def sliced_out(rows, c):
    buf = torch.zeros(rows, c + 24, dtype=BF, device="cuda")
    return buf, buf[:, 16:16 + c]


def assert_rest_untouched(buf, c):
    assert not buf[:, :16].any() and not buf[:, 16 + c:].any()


# ---------------------------------------------------------------- ops 4 and 5
@pytest.mark.parametrize("shape", SMALL + PRODUCT, ids=ids)
def test_gather_is_exact(cuda, shape):
    B, F, L, s, hw, C = shape
    x = rand_rows(B * F * hw, C, seed=F * 100 + hw)
    want = gather_ref(x, B, F, hw, L, s)
    buf, out = sliced_out(want.shape[0], C)
    got = ops.window_gather(sliced_in(x), B, F, hw, L, s, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert_rest_untouched(buf, C)
    with mf.poisoned_empty():
        own = ops.window_gather(x, B, F, hw, L, s)
    assert torch.equal(own.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("scheme", R.SCHEMES)
@pytest.mark.parametrize("shape", SMALL + PRODUCT, ids=ids)
def test_merge_matches_fp64(cuda, shape, scheme):
    B, F, L, s, hw, C = shape
    nW = len(R.frame_indices(F, L, s)[0])
    xw = rand_rows(B * nW * L * hw, C, seed=F * 100 + hw + 1)
    wt = weights_dev(L, scheme)
    ref = merge_ref(xw, wt, B, F, hw, L, s)
    buf, out = sliced_out(B * F * hw, C)
    got = ops.window_merge(sliced_in(xw), wt, B, F, hw, L, s, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert_within_bar(got, ref, xw.double().abs().max().item(), f"{shape} {scheme}")
    assert_rest_untouched(buf, C)


@pytest.mark.parametrize("scheme", ["flat", "pyramid"])
@pytest.mark.parametrize("shape", SMALL + PRODUCT[:1], ids=ids)
def test_merge_of_gather_is_the_identity_bitwise(cuda, shape, scheme):
    """Integer weights: every partial sum (sum of w) * x is exact in fp32 for a bf16 x (8 + 9
    significant bits at most), and the correctly rounded quotient of two exact values is x."""
    B, F, L, s, hw, C = shape
    x = rand_rows(B * F * hw, C, seed=F + hw)
    with mf.poisoned_empty():
        back = ops.window_merge(ops.window_gather(x, B, F, hw, L, s), weights_dev(L, scheme), B, F, hw, L, s)
    assert torch.equal(back.view(torch.int16), x.view(torch.int16))


def test_merge_order_does_not_depend_on_batch_positions_or_columns(cuda):
    """Video 1, positions 2..3, columns 8..16 of a larger call equal the same rows run alone."""
    B, F, L, s, hw, C = 3, 28, 16, 4, 5, 24
    nW = len(R.frame_indices(F, L, s)[0])
    xw = rand_rows(B * nW * L * hw, C, seed=9)
    wt = weights_dev(L, "delayed_reverse_sawtooth")
    whole = ops.window_merge(xw, wt, B, F, hw, L, s).reshape(B, F, hw, C)
    part = xw.reshape(B, nW, L, hw, C)[1:2, :, :, 2:4, 8:16].contiguous().reshape(-1, 8)
    alone = ops.window_merge(part, wt, 1, F, 2, L, s).reshape(1, F, 2, 8)
    assert torch.equal(whole[1:2, :, 2:4, 8:16].contiguous().view(torch.int16), alone.view(torch.int16))


def test_wrappers_refuse_bad_shapes(cuda):
    x = rand_rows(2 * 6 * 3, 8, seed=1)
    wt = weights_dev(4, "flat")
    with pytest.raises(ValueError, match="rows are not"):
        ops.window_gather(x, 2, 7, 3, 4, 2)
    with pytest.raises(ValueError, match="windows need"):
        ops.window_gather(x, 2, 6, 3, 4, 5)
    with pytest.raises(VdiffError, match="invalid argument"):
        ops.window_gather(x, 1, 4, 9, 4, 2, out=x)  # one window, in place
    with pytest.raises(ValueError, match="weights"):
        ops.window_merge(ops.window_gather(x, 2, 6, 3, 4, 2), wt[:3], 2, 6, 3, 4, 2)
    with pytest.raises(ValueError, match="rows are not"):
        ops.window_merge(x, wt, 2, 6, 3, 4, 2)


# ---------------------------------------------------------------- framing
FRAMED = [(2, 7, 4, 2, 3, 8), (2, 9, 4, 3, 2, 24), (1, 28, 16, 4, 2, 8), (1, 33, 32, 1, 1, 8), (1, 6, 4, 2, 1030, 8)]


@pytest.mark.parametrize("slack", [0, 8])
@pytest.mark.parametrize("shape", FRAMED, ids=ids)
def test_gather_framed(cuda, shape, slack):
    """x and out in poisoned frames: no store outside out, every element of out written, no NaN
    from beyond x's rows or columns in the output, x only read."""
    B, F, L, s, hw, C = shape
    x = rand_rows(B * F * hw, C, seed=5)
    want = gather_ref(x, B, F, hw, L, s)
    xv, fx = mf.load2d(x, col_slack=slack, name="x")
    ov, fo = mf.framed(want.shape, BF, cuda, col_slack=slack, name="out")
    ops.window_gather(xv, B, F, hw, L, s, out=ov)
    torch.cuda.synchronize()
    mf.assert_all_intact(fx, fo)
    fo.assert_written(want)
    assert torch.equal(ov.contiguous().view(torch.int16), want.view(torch.int16))
    assert torch.equal(xv.contiguous().view(torch.int16), x.view(torch.int16))


@pytest.mark.parametrize("slack", [0, 8])
@pytest.mark.parametrize("shape", FRAMED, ids=ids)
def test_merge_framed(cuda, shape, slack):
    """The window rows, the L weights and out in poisoned frames; the tail window's frames that
    the merge must not use are NaN, so a read of them would poison the output."""
    B, F, L, s, hw, C = shape
    idx, tail = R.frame_indices(F, L, s)
    nW = len(idx)
    xw = rand_rows(B * nW * L * hw, C, seed=6)
    if tail:
        xw.reshape(B, nW, L, hw, C)[:, -1, :L - tail] = float("nan")
    wt = weights_dev(L, "pyramid")
    clean = torch.nan_to_num(xw.float(), nan=0.0).to(BF)
    ref = merge_ref(clean, wt, B, F, hw, L, s)
    xv, fx = mf.load2d(xw, col_slack=slack, name="xw")
    wv, fw = mf.framed_1d(L, F32, cuda, name="wt")
    fw.load(wt)
    ov, fo = mf.framed((B * F * hw, C), BF, cuda, col_slack=slack, name="out")
    got = ops.window_merge(xv, wv, B, F, hw, L, s, out=ov)
    torch.cuda.synchronize()
    mf.assert_all_intact(fx, fw, fo)
    fo.assert_written(ref)
    assert_within_bar(got, ref, clean.double().abs().max().item(), f"framed {shape} slack {slack}")


# ---------------------------------------------------------------- the tiny UNet
FN = (4, 2, "pyramid")  # context_length, context_stride, weighting_scheme


def sharpened_(model):
    """With the stock synthetic weights the motion branch is too weak to show windowing (FreeNoise
    on against off moves the UNet output by about 0.02 rel-L2, the bf16 path's own distance from
    the fp32 reference): every motion module's to_q / to_k x 8 and its proj_out x 4 (powers of
    two: the values stay bf16)."""
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "motion_modules." in n or n.startswith(("transformer_blocks.", "proj_out.")):
                if n.endswith(("to_q.weight", "to_k.weight")):
                    p.mul_(8)
                elif n.endswith("proj_out.weight") and "transformer_blocks" not in n:
                    p.mul_(4)
    return model


def latents(F, seed):
    return torch.randn(1, 4, F, 16, 16, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def tiny(cuda):
    """The sharpened tiny UNet, 16 x 16 latents with CFG batch 2 at 6 and 7 frames, and the CPU
    references (fp32, FreeNoise on and off; the bf16-emulating one), computed once."""
    m = sharpened_(init_synthetic_(UNetMotionModel("tiny"), seed=0))
    sd = {k: v.float() for k, v in m.state_dict().items()}
    unet = m.to("cuda", BF).prepare()
    assert not unet.free_noise_enabled
    ehs = torch.randn(2, 77, 64, generator=torch.Generator().manual_seed(1234)).to(BF).float()
    d = dict(unet=unet, sd=sd, ehs=ehs)
    with torch.no_grad():
        for F in (6, 7):
            lat = latents(F, 100 + F)
            x2 = torch.cat([lat, lat])
            d[F] = dict(lat=lat, x2=x2, on=R.unet_forward_free_noise(sd, TINY, x2, 961, ehs, FN, "fp32"),
                        off=unet_ref.unet_forward(sd, TINY, x2, 961, ehs),
                        on_bf16=R.unet_forward_free_noise(sd, TINY, x2, 961, ehs, FN, "bf16"))
            d[F]["never"] = unet(x2.cuda(), 961, encoder_hidden_states=ehs.cuda()).sample.clone()
    return d


@pytest.fixture
def fn_on(tiny):
    tiny["unet"].enable_free_noise(*FN)
    yield tiny["unet"]
    tiny["unet"].disable_free_noise()


# BAR = 1.3 x the larger of two measurements on this model and these inputs (1.3 x is the headroom
# test_tiny_unet_matches_oracle keeps):
#   the bf16-emulating CPU reference against the fp32 one, FreeNoise on: 0.01513 (F = 6), 0.01585
#     (F = 7); 0.01496 / 0.01561 on another host's CPU (another BLAS blocking)
#   the device with FreeNoise DISABLED against the fp32 reference without it — the code as it
#     was before FreeNoise: 0.01546 (F = 6), 0.01595 (F = 7)
# so BAR = 1.3 x 0.01596.  Measured against it with FreeNoise on: the fast path 0.01506 (F = 6),
# 0.01579 (F = 7), 0.01500 (F = 40); the module path 0.01985 / 0.02035, where the module path
# without FreeNoise sits at 0.02021 / 0.01993 from its own reference (it rounds every module's
# output to bf16).  The reference itself moves by 0.1595 (F = 6) and 0.1853 (F = 7) when FreeNoise
# is switched on, more than 5 bars (test_reference_moves_far_more_than_the_bar), so a no-op
# enable_free_noise, a wrong window list, a dropped tail or the PE by absolute frame cannot pass.
BAR = 1.3 * 0.01596


def test_reference_moves_far_more_than_the_bar(tiny):
    for F in (6, 7):
        d = rel_l2(tiny[F]["off"], tiny[F]["on"])
        emu = rel_l2(tiny[F]["on_bf16"], tiny[F]["on"])
        dev_off = rel_l2(tiny[F]["never"], tiny[F]["off"])
        print(f"F={F}: reference FreeNoise on vs off rel-L2 {d:.4f}; bf16 emulation vs fp32 {emu:.5f}; "
              f"device with FreeNoise disabled vs the fp32 reference without {dev_off:.5f}; BAR {BAR:.5f}")
        assert d >= 5 * BAR, (F, d)
        assert BAR >= 1.3 * emu and BAR >= 1.3 * dev_off, (F, emu, dev_off)  # BAR is what its comment says


@pytest.mark.parametrize("F", [6, 7])
def test_tiny_unet_fast_path(tiny, fn_on, F):
    t = tiny[F]
    out = fn_on(t["x2"].cuda(), 961, encoder_hidden_states=tiny["ehs"].cuda()).sample
    err = rel_l2(out, t["on"])
    print(f"tiny UNet + FreeNoise{FN}, fast path, F={F}: rel-L2 vs fp32 reference {err:.5f}; "
          f"FreeNoise off vs that reference {rel_l2(t['never'], t['on']):.5f}")
    assert err < BAR, err


@pytest.mark.parametrize("F", [6, 7])
def test_tiny_unet_module_path(tiny, fn_on, F):
    """A forward hook sends the call down forward(): the same semantics on the HIP ops.  The
    module path rounds every module's output to bf16, so without FreeNoise it already sits a
    little above the fast path (printed)."""
    t = tiny[F]
    seen = []
    blk = fn_on.down_blocks[0].motion_modules[0].transformer_blocks[0]
    hook = blk.register_forward_hook(lambda m, a, o: seen.append(tuple(a[0].shape)))
    try:
        out = fn_on(t["x2"].cuda(), 961, encoder_hidden_states=tiny["ehs"].cuda()).sample
    finally:
        hook.remove()
    n_w = len(R.frame_indices(F, FN[0], FN[1])[0])
    assert seen == [(2 * n_w * 256, FN[0], 64)]  # every window one more video: (B * nW * H * W, L, C)
    err = rel_l2(out, t["on"])
    fn_on.disable_free_noise()
    hook = blk.register_forward_hook(lambda m, a, o: None)
    try:
        off = fn_on(t["x2"].cuda(), 961, encoder_hidden_states=tiny["ehs"].cuda()).sample
    finally:
        hook.remove()
    print(f"tiny UNet + FreeNoise{FN}, module path, F={F}: rel-L2 vs fp32 reference {err:.5f}; the module "
          f"path without FreeNoise vs the fp32 reference without {rel_l2(off, t['off']):.5f}")
    assert err < BAR, err


def test_one_window_equals_off_bitwise(tiny):
    unet, ehs = tiny["unet"], tiny["ehs"].cuda()
    lat = latents(4, 55)
    x = torch.cat([lat, lat]).cuda()
    off = unet(x, 961, encoder_hidden_states=ehs).sample.clone()
    unet.enable_free_noise(*FN)
    try:
        on = unet(x, 961, encoder_hidden_states=ehs).sample.clone()
        hook = unet.mid_block.register_forward_hook(lambda m, a, o: None)
        try:
            on_mod = unet(x, 961, encoder_hidden_states=ehs).sample.clone()
        finally:
            hook.remove()
        with pytest.raises(ValueError, match="fewer than context_length"):
            unet(x[:, :, :3], 961, encoder_hidden_states=ehs)
    finally:
        unet.disable_free_noise()
    hook = unet.mid_block.register_forward_hook(lambda m, a, o: None)
    try:
        off_mod = unet(x, 961, encoder_hidden_states=ehs).sample
    finally:
        hook.remove()
    assert torch.equal(on, off) and torch.equal(on_mod, off_mod)


def test_disable_free_noise_restores_every_bit(tiny):
    unet, x, ehs = tiny["unet"], tiny[7]["x2"].cuda(), tiny["ehs"].cuda()
    unet.enable_free_noise(*FN)
    on = unet(x, 961, encoder_hidden_states=ehs).sample
    unet.disable_free_noise()
    off = unet(x, 961, encoder_hidden_states=ehs).sample
    assert not torch.equal(on, tiny[7]["never"])
    assert torch.equal(off, tiny[7]["never"])
    assert all(m._fn_wt is None for m in unet.motion_modules_in_order())


@pytest.fixture(scope="module")
def loop3_ref(tiny):
    acp = ddim_ref.alphas_cumprod()
    with torch.no_grad():
        return ddim_ref.denoise_loop(lambda xi, t, e: R.unet_forward_free_noise(tiny["sd"], TINY, xi, t, e, FN, "fp32"),
                                     tiny[7]["lat"], tiny["ehs"], 50, 7.5, acp, steps=3)


@pytest.mark.parametrize("use_graph", [True, False])
def test_three_step_loop(tiny, fn_on, loop3_ref, use_graph):
    s = DDIMScheduler(beta_schedule="linear", steps_offset=1, clip_sample=False)
    s.set_timesteps(50)
    loop = DenoiseLoop(fn_on, s, tiny[7]["lat"].cuda(), tiny["ehs"].cuda(), 7.5, use_graph=use_graph).prime()
    if use_graph:
        assert loop.graph is not None, loop.graph_error
    assert all(w is not None and w.tolist() == [1, 2, 2, 1] for w in loop.free_noise_operands)
    x = loop.run(3)
    err = rel_l2(x, loop3_ref)
    print(f"3-step loop + FreeNoise (graph {use_graph}): rel-L2 {err:.5f}")
    assert err < 0.01, err  # test_denoise_loop_graph_matches_oracle's bar


def test_loop_built_before_enable_keeps_running_without(tiny):
    unet, lat, ehs = tiny["unet"], tiny[7]["lat"].cuda(), tiny["ehs"].cuda()
    s = DDIMScheduler(beta_schedule="linear", steps_offset=1, clip_sample=False)
    s.set_timesteps(50)
    before = DenoiseLoop(unet, s, lat, ehs, 7.5).prime()
    assert before.graph is not None, before.graph_error
    want = before.run(2).clone()
    before.reset(lat)
    unet.enable_free_noise(*FN)
    try:
        assert torch.equal(before.run(2), want)
    finally:
        unet.disable_free_noise()


def test_pipeline_enable_free_noise(tiny):
    unet, lat, ehs = tiny["unet"], tiny[7]["lat"].cuda(), tiny["ehs"].cuda()
    sched = DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = AnimateDiffPipeline(unet, sched)
    kw = dict(prompt_embeds=ehs[1:2], negative_prompt_embeds=ehs[0:1], latents=lat, num_frames=7, height=128,
              width=128, num_inference_steps=3, guidance_scale=7.5, output_type="latent")
    off = pipe(**kw).frames.clone()
    pipe.enable_free_noise(context_length=FN[0], context_stride=FN[1], weighting_scheme=FN[2])
    try:
        on = pipe(**kw).frames.clone()
        sched.set_timesteps(3)
        loop = DenoiseLoop(unet, sched, lat, ehs, 7.5).prime()
        assert torch.equal(on, loop.run())
        # the rescheduled noise: 4 user frames are extended to the 7 asked for
        ext = pipe(**{**kw, "latents": lat[:, :, :4], "generator": torch.Generator().manual_seed(3)}).frames
        assert ext.shape == on.shape and torch.isfinite(ext).all()
    finally:
        pipe.disable_free_noise()
    assert torch.isfinite(on).all() and rel_l2(on, off) > 0.02
    assert torch.equal(pipe(**kw).frames, off)


def test_freeu_and_free_noise_together(tiny):
    unet, x, ehs = tiny["unet"], tiny[6]["x2"].cuda(), tiny["ehs"].cuda()
    outs = {}
    try:
        for name, (fu, fnz) in {"freeu": (True, False), "free_noise": (False, True), "both": (True, True)}.items():
            unet.disable_freeu()
            unet.disable_free_noise()
            if fu:
                unet.enable_freeu(*FREEU)
            if fnz:
                unet.enable_free_noise(*FN)
            outs[name] = unet(x, 961, encoder_hidden_states=ehs).sample.clone()
    finally:
        unet.disable_freeu()
        unet.disable_free_noise()
    assert torch.isfinite(outs["both"]).all()
    assert rel_l2(outs["both"], outs["freeu"]) > 0.02 and rel_l2(outs["both"], outs["free_noise"]) > 0.02


def test_forty_frames_past_the_old_cap(tiny, fn_on):
    """40 frames (19 windows of 4) against the reference at BAR; without FreeNoise the same call
    is refused, as every call past motion_max_seq_length = 32 always was."""
    lat = latents(40, 140)
    x2, ehs = torch.cat([lat, lat]), tiny["ehs"]
    with torch.no_grad():
        want = R.unet_forward_free_noise(tiny["sd"], TINY, x2, 961, ehs, FN, "fp32")
    out = fn_on(x2.cuda(), 961, encoder_hidden_states=ehs.cuda()).sample
    err = rel_l2(out, want)
    print(f"tiny UNet + FreeNoise{FN}, F=40: rel-L2 vs fp32 reference {err:.5f}")
    assert err < BAR, err
    fn_on.disable_free_noise()
    with pytest.raises(ValueError, match="motion_max_seq_length"):
        fn_on(x2.cuda(), 961, encoder_hidden_states=ehs.cuda())


# ---------------------------------------------------------------- the product kernel
def test_level1_motion_module_windows_reach_the_fused_qkv_kernel(cuda):
    """The full config's level-1 motion module alone (C 320, 8 heads of d 40), sharpened as the
    tiny model: B 2, F 20, windows of 16 by 4 (2 per video), 32 x 32 positions.  The windowed
    batch (4 videos of 16 frames) is a shape vd_motion_qkv_attention takes.  Bar: 1.3 x the
    device's own error at F = 16 with FreeNoise off, on the same module and the same inputs'
    first 16 frames — measured in this test, before FreeNoise is enabled."""
    heads, C, B, F, L, s, H = 8, 320, 2, 20, 16, 4, 32
    m = sharpened_(init_synthetic_(AnimateDiffTransformer3D(heads, C // heads, C, 32, 32), seed=0))
    sd = {f"m.{k}": v.detach().float() for k, v in m.state_dict().items()}
    m = m.to("cuda", BF)
    prepare_tree(m)
    nW = len(R.frame_indices(F, L, s)[0])
    assert ops.motion_qkv_takes(B * nW, L, H * H, heads, C // heads)
    x20 = torch.randn(B * F, C, H, H, generator=torch.Generator().manual_seed(7)).to(BF).float()
    x16 = x20.reshape(B, F, C, H, H)[:, :L].reshape(B * L, C, H, H)

    def rows(x):
        return x.permute(0, 2, 3, 1).reshape(-1, C).to("cuda", BF).contiguous()

    def fmap(t, n):
        return t.float().cpu().reshape(n, H, H, C).permute(0, 3, 1, 2)

    with torch.no_grad():
        want16 = unet_ref.motion_module(sd, "m", x16, L, heads, 32, 32)
        want20 = R.motion_module(sd, "m", x20, F, heads, 32, 32, (L, s, "pyramid"))
        off20 = unet_ref.motion_module(sd, "m", x20, F, heads, 32, 32)
    err16 = rel_l2(fmap(m.run(Act(rows(x16), B * L, H, H), Ctx(B, L, None, None, 77)).t, B * L), want16)
    m.context_length, m.context_stride, m.weighting_scheme = L, s, "pyramid"
    m.prepare()
    got = fmap(m.run(Act(rows(x20), B * F, H, H), Ctx(B, F, None, None, 77)).t, B * F)
    err20, moved = rel_l2(got, want20), rel_l2(off20, want20)
    print(f"level-1 motion module: F=16 FreeNoise off {err16:.5f} (bar {1.3 * err16:.5f}); F=20 windows of 16 by 4 "
          f"{err20:.5f}; the reference on vs off {moved:.4f}")
    assert moved >= 5 * 1.3 * err16, (moved, err16)
    assert err20 <= 1.3 * err16, (err20, err16)
