"""FreeU on the MI355X: vd_rows_eltwise ops 2 (the spectral skip filter) and 3 (the backbone
scale) against tests/freeu_ref.py, framed by tests/memframe.py, and enable_freeu end to end on
the tiny UNet (fast path, module path, hipGraph loop, pipeline).

Kernel bar (set by the arithmetic, not by what the kernel gives): |got - ref| <= 2^-8 |ref| +
1e-5 max|x| against the closed form in fp64 — one bf16 rounding (unit roundoff 2^-8) plus the
fp32 sums (7 sums of <= 1024 terms scaled by |s - 1| / HW: well under 1e-6 max|x|).

Shapes: the issue's six, the three product shapes (32 images x {8x8x1280, 16x16x1280,
16x16x640}: slabs of 8 and 4 chunks, the register path), 16 x 2x3 x 640 (the slab of 2 chunks),
and 1 x 32x32 x 16 (a plane too large for the registers: the re-reading path).
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import freeu_ref as R
import memframe as mf
from oracle import ddim_ref, unet_ref
from vdiff import AnimateDiffPipeline, DDIMScheduler, DenoiseLoop, UNetMotionModel, init_synthetic_, ops
from vdiff.config import TINY

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GOLD = Path(__file__).resolve().parent / "golden"
FREEU = (0.9, 0.2, 1.2, 1.4)  # s1, s2, b1, b2

SMALL = [(1, 2, 2, 8), (2, 2, 7, 8), (2, 3, 5, 24), (3, 8, 8, 64), (2, 16, 16, 40), (1, 32, 32, 16), (16, 2, 3, 640)]
PRODUCT = [(32, 8, 8, 1280), (32, 16, 16, 1280), (32, 16, 16, 640)]


def rel_l2(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).norm() / want.norm()).item()


def rows_of(n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n * h * w, c, generator=g).to(BF)


def nchw(rows, n, h, w):
    return rows.double().cpu().reshape(n, h, w, -1).permute(0, 3, 1, 2)


def closed_form_rows(x, n, h, w, s):
    """fp64 closed form of the rows x (bf16, CPU) with the fp32 value of s the device reads."""
    s32 = torch.tensor(s, dtype=F32).double().item()
    return R.closed_form(nchw(x, n, h, w), s32).permute(0, 2, 3, 1).reshape(n * h * w, -1)


def assert_within_bar(got, ref, xmax, what=""):
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * xmax
    bad = int((~(err <= bound)).sum())  # a NaN is out of tolerance
    worst = (err - bound).max().item()
    print(f"freeu_filter {what}: max|err| {err.max().item():.3e}, max(err - bound) {worst:.3e}")
    assert bad == 0, f"{what}: {bad} of {ref.numel()} elements past the bar (worst by {worst:.3e})"


def filter_sliced(x, n, h, w, s):
    """op 2 with ldx > C and out a column slice of a wider buffer."""
    c = x.shape[1]
    xin = torch.full((x.shape[0], c + 16), float("nan"), dtype=BF, device="cuda")
    xin[:, 8:8 + c] = x.cuda()
    buf = torch.zeros(x.shape[0], c + 24, dtype=BF, device="cuda")
    out = ops.freeu_filter(xin[:, 8:8 + c], n, h, w, torch.tensor([s], dtype=F32, device="cuda"), out=buf[:, 16:16 + c])
    assert out.data_ptr() == buf[:, 16:].data_ptr()
    assert not buf[:, :16].any() and not buf[:, 16 + c:].any()  # the rest of the wider buffer is untouched
    return out


# ---------------------------------------------------------------- op 2
@pytest.mark.parametrize("s", [0.2, 0.9])
@pytest.mark.parametrize("shape", SMALL, ids=lambda v: "x".join(map(str, v)))
def test_filter_matches_closed_form(cuda, shape, s):
    n, h, w, c = shape
    x = rows_of(n, h, w, c, seed=h * 100 + w)
    got = filter_sliced(x, n, h, w, s)
    assert_within_bar(got, closed_form_rows(x, n, h, w, s), x.double().abs().max().item(), f"{shape} s={s}")


@pytest.mark.parametrize("shape", PRODUCT, ids=lambda v: "x".join(map(str, v)))
def test_filter_product_shapes(cuda, shape):
    n, h, w, c = shape
    x = rows_of(n, h, w, c, seed=c + h)
    got = filter_sliced(x, n, h, w, 0.2)
    assert_within_bar(got, closed_form_rows(x, n, h, w, 0.2), x.double().abs().max().item(), f"{shape} s=0.2")


@pytest.mark.parametrize("shape", [(2, 3, 5, 24), (3, 8, 8, 64), (1, 32, 32, 16)], ids=lambda v: "x".join(map(str, v)))
def test_filter_s_equal_1_returns_x_bits(cuda, shape):
    n, h, w, c = shape
    x = rows_of(n, h, w, c, seed=7).cuda()
    got = ops.freeu_filter(x, n, h, w, torch.ones(1, device="cuda"))
    assert torch.equal(got.view(torch.int16), x.view(torch.int16))


@pytest.mark.parametrize("n_all,shape", [(5, (8, 8, 64)), (5, (32, 32, 16)), (40, (2, 3, 1024))],
                         ids=["5x8x8x64", "5x32x32x16", "40x2x3x1024-slab8-vs-slab1"])
def test_filter_image_independence(cuda, n_all, shape):
    """Image 3 of an n-image call equals the same image run alone, bit for bit: the summation
    order depends on (H, W) alone — also where the n-image grid runs slabs of 8 chunks and the
    single image slabs of 1 (40 images of 1024 channels)."""
    h, w, c = shape
    x = rows_of(n_all, h, w, c, seed=11).cuda()
    s = torch.tensor([0.2], device="cuda")
    whole = ops.freeu_filter(x, n_all, h, w, s)
    one = ops.freeu_filter(x[3 * h * w:4 * h * w], 1, h, w, s)
    assert torch.equal(whole[3 * h * w:4 * h * w].view(torch.int16), one.view(torch.int16))


def test_filter_refuses_in_place_and_flat_planes(cuda):
    from vdiff._lib import VdiffError
    x = rows_of(2, 2, 4, 8, seed=1).cuda()
    s = torch.ones(1, device="cuda")
    with pytest.raises(VdiffError, match="invalid argument"):
        ops.freeu_filter(x, 2, 2, 4, s, out=x)
    with pytest.raises(VdiffError, match="invalid argument"):
        ops.freeu_filter(x, 2, 1, 8, s)
    with pytest.raises(ValueError, match="rows are not"):
        ops.freeu_filter(x, 3, 2, 4, s)


# ---------------------------------------------------------------- op 3
@pytest.mark.parametrize("g", [1.2, 1.4, 0.3])
def test_scale_is_one_fp32_multiply_rounded_once(cuda, g):
    x = rows_of(77, 1, 1, 72, seed=3).cuda()
    want = (x.float() * torch.tensor(g, dtype=F32)).to(BF)
    got = ops.scale_rows_(x.clone(), torch.tensor([g], dtype=F32, device="cuda"))
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_scale_in_place_on_a_column_slice(cuda):
    x = rows_of(33, 1, 1, 48, seed=4).cuda()
    y = x.clone()
    r = ops.scale_rows_(y[:, :24], torch.tensor([1.4], dtype=F32, device="cuda"))
    assert r.data_ptr() == y.data_ptr()
    assert torch.equal(y[:, :24], (x[:, :24].float() * torch.tensor(1.4, dtype=F32)).to(BF))
    assert torch.equal(y[:, 24:].view(torch.int16), x[:, 24:].view(torch.int16))
    z = x.clone()
    ops.scale_rows_(z[:, 8:32], torch.ones(1, device="cuda"))  # g = 1: the identity
    assert torch.equal(z.view(torch.int16), x.view(torch.int16))


# ---------------------------------------------------------------- framing
@pytest.mark.parametrize("slack", [0, 8])
@pytest.mark.parametrize("shape", [(2, 3, 5, 24), (3, 8, 8, 64), (1, 32, 32, 16), (16, 2, 3, 640)],
                         ids=lambda v: "x".join(map(str, v)))
def test_filter_framed(cuda, shape, slack):
    """x, the scalar and out in poisoned frames: no store outside out, every element of out
    written, and no NaN from beyond x's rows or columns in any output."""
    n, h, w, c = shape
    x = rows_of(n, h, w, c, seed=5)
    xv, fx = mf.load2d(x.cuda(), col_slack=slack, name="x")
    sv, fs = mf.framed_1d(1, F32, cuda, name="s")
    fs.load(torch.tensor([0.2]))
    ov, fo = mf.framed((n * h * w, c), BF, cuda, col_slack=slack, name="out")
    with mf.poisoned_empty():
        got = ops.freeu_filter(xv, n, h, w, sv, out=ov)
    torch.cuda.synchronize()
    mf.assert_all_intact(fx, fs, fo)
    ref = closed_form_rows(x, n, h, w, 0.2)
    fo.assert_written(ref)
    assert_within_bar(got, ref, x.double().abs().max().item(), f"framed {shape} slack {slack}")
    assert torch.equal(xv.cpu().view(torch.int16), x.view(torch.int16))  # the input is only read


@pytest.mark.parametrize("slack", [0, 8])
def test_scale_framed(cuda, slack):
    """op 3 out of place through the entry point (framed out: written everywhere, nothing beside
    it) and in place through the wrapper (the frame around x intact)."""
    from vdiff._lib import check, lib
    x = rows_of(77, 1, 1, 72, seed=6)
    want = (x.float() * torch.tensor(1.2, dtype=F32)).to(BF)
    xv, fx = mf.load2d(x.cuda(), col_slack=slack, name="x")
    gv, fg = mf.framed_1d(1, F32, cuda, name="g")
    fg.load(torch.tensor([1.2]))
    ov, fo = mf.framed((77, 72), BF, cuda, col_slack=slack, name="out")
    check(lib().vd_rows_eltwise(3, xv.data_ptr(), xv.stride(0), gv.data_ptr(), 0, 1, 1, 1, 77, 72, ov.data_ptr(),
                                ov.stride(0), torch.cuda.current_stream().cuda_stream), "vd_rows_eltwise(scale)")
    torch.cuda.synchronize()
    mf.assert_all_intact(fx, fg, fo)
    fo.assert_written(want)
    assert torch.equal(ov.cpu().view(torch.int16), want.view(torch.int16))
    with mf.poisoned_empty():
        ops.scale_rows_(xv, gv)
    torch.cuda.synchronize()
    mf.assert_all_intact(fx, fg)
    assert torch.equal(xv.cpu().view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------- the tiny UNet
@pytest.fixture(scope="module")
def tiny(cuda):
    """The tiny UNet, the golden inputs cut to 2 frames x 32^2, the model's output before FreeU
    was ever enabled, and the CPU references (fp32 oracle with and without FreeU), computed once."""
    m = init_synthetic_(UNetMotionModel("tiny"), seed=0)
    sd = {k: v.float() for k, v in m.state_dict().items()}
    unet = m.to("cuda", BF).prepare()
    g = np.load(GOLD / "tiny_unet.npz")
    lat = torch.from_numpy(g["latents"])[:, :, :2, :32, :32].contiguous()
    ehs = torch.from_numpy(g["ehs"])
    x2 = torch.cat([lat, lat])
    with torch.no_grad():
        want_on = R.unet_forward_freeu(sd, TINY, x2, 961, ehs, FREEU, "fp32")
        want_off = unet_ref.unet_forward(sd, TINY, x2, 961, ehs)
    never = unet(x2.cuda(), 961, encoder_hidden_states=ehs.cuda()).sample.clone()
    return dict(unet=unet, sd=sd, lat=lat, ehs=ehs, x2=x2, want_on=want_on, want_off=want_off, never=never)


@pytest.fixture
def freeu_on(tiny):
    tiny["unet"].enable_freeu(*FREEU)
    yield tiny["unet"]
    tiny["unet"].disable_freeu()


# test_tiny_unet_matches_oracle's bar is 0.018 at 1.3x headroom over its measured 0.0137-0.0138.
# The fast path with FreeU measures 0.01415 at this shape (the bf16-emulating reference against
# the fp32 one: 0.0141 on the CPU), which leaves 0.018 only 1.27x, so the bar is 1.3 x 0.01415.
BAR = 0.0184


def test_reference_moves_far_more_than_the_bar(tiny):
    """A no-op enable_freeu must fail the parity tests: FreeU moves the reference >= 5 bars."""
    d = rel_l2(tiny["want_off"], tiny["want_on"])
    print(f"reference FreeU on vs off rel-L2 {d:.4f}")
    assert d >= 5 * BAR, d


def test_tiny_unet_fast_path(tiny, freeu_on):
    out = freeu_on(tiny["x2"].cuda(), 961, encoder_hidden_states=tiny["ehs"].cuda()).sample
    err = rel_l2(out, tiny["want_on"])
    print(f"tiny UNet + FreeU, fast path: rel-L2 vs fp32 reference {err:.5f}; FreeU off vs that reference "
          f"{rel_l2(tiny['never'], tiny['want_on']):.5f}")
    assert err < BAR, err


def test_tiny_unet_module_path(tiny, freeu_on):
    """Same reference, same bar.  Measured 0.01821: the module path rounds every module's output
    to bf16 and sits at 0.01805 at this shape without FreeU as well (printed below; 0.0182 at
    the golden shape, where tests/test_gpu_modules.py holds it to 0.024), so FreeU adds 0.0002 to
    it, and the fast path's bar leaves it 1 % of headroom."""
    seen = []
    hook = freeu_on.up_blocks[0].resnets[0].register_forward_hook(lambda m, a, o: seen.append(tuple(a[0].shape)))
    try:
        out = freeu_on(tiny["x2"].cuda(), 961, encoder_hidden_states=tiny["ehs"].cuda()).sample
    finally:
        hook.remove()
    assert seen == [(4, 256, 16, 16)]  # the concatenated (N, C, H, W) map diffusers' hook sees
    err = rel_l2(out, tiny["want_on"])
    print(f"tiny UNet + FreeU, module path: rel-L2 vs fp32 reference {err:.5f}")
    freeu_on.disable_freeu()
    hook = freeu_on.up_blocks[0].register_forward_hook(lambda m, a, o: None)
    try:
        off = freeu_on(tiny["x2"].cuda(), 961, encoder_hidden_states=tiny["ehs"].cuda()).sample
    finally:
        hook.remove()
    print(f"  the module path without FreeU vs the fp32 oracle: {rel_l2(off, tiny['want_off']):.5f}")
    assert err < BAR, err


def test_disable_freeu_restores_every_bit(tiny):
    unet, x, ehs = tiny["unet"], tiny["x2"].cuda(), tiny["ehs"].cuda()
    unet.enable_freeu(*FREEU)
    on = unet(x, 961, encoder_hidden_states=ehs).sample
    unet.disable_freeu()
    off = unet(x, 961, encoder_hidden_states=ehs).sample
    assert not torch.equal(on, tiny["never"])
    assert torch.equal(off, tiny["never"])
    assert all(b._freeu is None for b in unet.up_blocks)


@pytest.fixture(scope="module")
def loop3_ref(tiny):
    acp = ddim_ref.alphas_cumprod()
    with torch.no_grad():
        return ddim_ref.denoise_loop(lambda xi, t, e: R.unet_forward_freeu(tiny["sd"], TINY, xi, t, e, FREEU, "fp32"),
                                     tiny["lat"], tiny["ehs"], 50, 7.5, acp, steps=3)


@pytest.mark.parametrize("use_graph", [True, False])
def test_three_step_loop(tiny, freeu_on, loop3_ref, use_graph):
    s = DDIMScheduler(beta_schedule="linear", steps_offset=1, clip_sample=False)
    s.set_timesteps(50)
    loop = DenoiseLoop(freeu_on, s, tiny["lat"].cuda(), tiny["ehs"].cuda(), 7.5, use_graph=use_graph).prime()
    if use_graph:
        assert loop.graph is not None, loop.graph_error
    x = loop.run(3)
    err = rel_l2(x, loop3_ref)
    print(f"3-step loop + FreeU (graph {use_graph}): rel-L2 {err:.5f}")
    assert err < 0.01, err  # test_denoise_loop_graph_matches_oracle's bar


def test_pipeline_enable_freeu(tiny):
    unet, lat, ehs = tiny["unet"], tiny["lat"].cuda(), tiny["ehs"].cuda()
    sched = DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)
    pipe = AnimateDiffPipeline(unet, sched)
    kw = dict(prompt_embeds=ehs[1:2], negative_prompt_embeds=ehs[0:1], latents=lat, num_frames=2, height=256,
              width=256, num_inference_steps=3, guidance_scale=7.5, output_type="latent")
    off = pipe(**kw).frames.clone()
    pipe.enable_freeu(*FREEU)
    try:
        on = pipe(**kw).frames.clone()
        sched.set_timesteps(3)
        loop = DenoiseLoop(unet, sched, lat, ehs, 7.5).prime()
        assert torch.equal(on, loop.run())
    finally:
        pipe.disable_freeu()
    assert torch.isfinite(on).all() and rel_l2(on, off) > 0.02
    assert torch.equal(pipe(**kw).frames, off)
