"""The VAE encoder on the MI355X: the conv loaders' pad-end stride-2 mode (VD_CONV_PAD_END) in every
conv-capable GEMM family against fp64 torch with framed operands, the pad-1 stride-2 conv those
loaders also serve, AutoencoderKL.encode against the fp64 reference (tests/vae_encoder_ref.py), and
the video-to-video pipeline.

Bounds.  Conv outputs are fp32 at the project's per-kernel tolerance (memframe.close_f32, rtol 1e-3 /
atol 1e-4).  The encoder's moments are held to rel-L2(device, fp64) <= 3 x d_emu, d_emu = rel-L2 of
the reference's own bf16-storage emulation against fp64 (mean and logvar separately): the factor
allows for the fp32 accumulation order, the flash kernel's bf16 probabilities and the hardware
exp2 the emulation leaves out.  Parity to diffusers is unpinned (reference header).
"""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import memframe as mf
import vae_encoder_ref as R
import vdiff._lib as L
import vdiff.pipeline as P
from vdiff import (AnimateDiffVideoToVideoPipeline, AutoencoderKL, DenoiseLoop, EulerDiscreteScheduler,
                   init_synthetic_, ops)
from vdiff.models.layers import pack_conv3x3
from vdiff.models.vae import VAE_FULL

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
BF, F32 = torch.bfloat16, torch.float32


# ---------------------------------------------------------------- the conv mode
def planned(path, n, h, w, ho, wo, cin, cout, stride):
    """(kernel, split) vd_gemm_plan gives the conv under a forced path (decided on the CPU side:
    sizes only)."""
    K = 9 * cin
    d = L.GemmDesc(a0=256, lda0=cin, k0=cin, a_mode=ops.A_CONV3X3, n_img=n, h_in=h, w_in=w, h_out=ho, w_out=wo,
                   stride=stride, w=256, ldw=K, M=n * ho * wo, N=cout, K=K, out=256, ldc=cout, out_f32=1, path=path)
    k, sp = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert L.lib().vd_gemm_plan(ctypes.byref(d), ctypes.byref(k), ctypes.byref(sp)) == 0
    return k.value, sp.value


def conv_operands(n, h, w, ho, wo, cin, cout, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n * h * w, cin, device="cuda", generator=g).to(BF)
    wt = (torch.randn(cout, cin, 3, 3, device="cuda", generator=g) * (9 * cin) ** -0.5).to(BF)
    b = torch.randn(cout, device="cuda", generator=g)
    r = torch.randn(n * ho * wo, cout, device="cuda", generator=g).to(BF)
    return x, wt, b, r


def run_framed(path, n, h, w, ho, wo, x, wt, b, r, **kw):
    """One conv with every operand in a poisoned frame; returns (fp32 output rows, frames)."""
    cout = wt.shape[0]
    xv, fx = mf.load2d(x, col_slack=8, name="x")
    wv, fw = mf.load2d(pack_conv3x3(wt), col_slack=8, name="w")
    bv, fb = mf.loadnd(b, name="bias")
    rv, fr = mf.load2d(r, col_slack=4, name="res")
    ov, fo = mf.framed((n * ho * wo, cout), F32, "cuda", col_slack=4, name="out")
    with ops.gemm_plan(path=path), mf.poisoned_empty():
        _, gh, gw = ops.conv3x3(xv, n, h, w, wv, bias=bv, res=rv, out=ov, out_f32=True, **kw)
    torch.cuda.synchronize()
    assert (gh, gw) == (ho, wo)
    return ov, fo, (fx, fw, fb, fr, fo)


def pad_end_case(path, n, h, w, cin, cout):
    ho, wo = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    ver, split = planned(path, n, h, w, ho, wo, cin, cout, 2 | ops.CONV_PAD_END)
    assert ver == path, f"the plan gives family {ver} (split {split}), not {path}: choose another shape"
    x, wt, b, r = conv_operands(n, h, w, ho, wo, cin, cout, seed=1000 * path + 16 * h + w + cin + cout)
    got, fo, frames = run_framed(path, n, h, w, ho, wo, x, wt, b, r, stride=2, pad_end=True)
    img = x.double().cpu().reshape(n, h, w, cin).permute(0, 3, 1, 2)
    want = F.conv2d(F.pad(img, (0, 1, 0, 1)), wt.double().cpu(), b.double().cpu(), stride=2)
    assert tuple(want.shape) == (n, cout, ho, wo)
    want = want.permute(0, 2, 3, 1).reshape(-1, cout) + r.double().cpu()
    fo.assert_written(want)
    mf.assert_all_intact(*frames)
    mf.close_f32(got, want)
    if h % 2 == 0 and w % 2 == 0:  # the mode is not pad 1: a kernel that ignored the flag fails here
        pad1 = F.conv2d(img, wt.double().cpu(), b.double().cpu(), stride=2, padding=1)
        assert not torch.allclose(pad1.permute(0, 2, 3, 1).reshape(-1, cout) + r.double().cpu(), want, atol=1e-2)


@pytest.mark.parametrize("cout", [20, 128])
@pytest.mark.parametrize("cin", [8, 64])
@pytest.mark.parametrize("h,w", [(8, 8), (7, 5), (6, 10), (2, 2)])
def test_pad_end_conv_v1(cuda, h, w, cin, cout):
    """3 images, so the seams fall inside one 128-row tile and a wrong edge reads the neighbour's real
    data: 8 x 8 -> 4 x 4 (the far taps land in the padding), 7 x 5 -> 3 x 2 (no tap reaches padding;
    smaller than pad 1's output), 6 x 10 -> 3 x 5, 2 x 2 -> 1 x 1.  Fewer than 64 rows: the plan's
    own choice is v1 too."""
    n, ho, wo = 3, (h - 2) // 2 + 1, (w - 2) // 2 + 1
    assert planned(0, n, h, w, ho, wo, cin, cout, 2 | ops.CONV_PAD_END)[0] == 1
    pad_end_case(1, n, h, w, cin, cout)


# one shape per LDS-DMA family, the smallest row count the family takes (v6: 64 rows, v2 / v5: 256),
# an image count that is no multiple of the tile so seams and the ragged last tile are inside it
FAMILY_CASES = [
    pytest.param(6, 11, 7, 5, 64, 128, id="v6-7x5-66rows"),
    pytest.param(6, 17, 8, 8, 64, 128, id="v6-8x8-272rows-splitk"),
    pytest.param(2, 17, 8, 8, 64, 128, id="v2-8x8-272rows-bn128"),
    pytest.param(2, 19, 6, 10, 64, 160, id="v2-6x10-285rows-bn160"),
    pytest.param(2, 43, 7, 5, 64, 20, id="v2-7x5-258rows-bn32"),
    pytest.param(5, 18, 6, 10, 64, 128, id="v5-6x10-270rows"),
]


@pytest.mark.parametrize("path,n,h,w,cin,cout", FAMILY_CASES)
def test_pad_end_conv_lds_dma_families(cuda, path, n, h, w, cin, cout):
    pad_end_case(path, n, h, w, cin, cout)


def test_every_conv_family_is_covered():
    fams = {1} | {p.values[0] for p in FAMILY_CASES}
    assert fams == {1, 2, 5, 6}


def test_pad_end_wrapper_refuses_other_strides(cuda):
    x = torch.zeros(64, 8, device=cuda, dtype=BF)
    wp = torch.zeros(8, 72, device=cuda, dtype=BF)
    with pytest.raises(ValueError, match="pad_end"):
        ops.conv3x3(x, 1, 8, 8, wp, stride=1, pad_end=True)
    with pytest.raises(ValueError, match="pad_end"):
        ops.conv3x3(x, 1, 8, 8, wp, stride=2, upsample=True, pad_end=True)


@pytest.mark.parametrize("path,n,h,w,cin,cout", [(1, 3, 7, 5, 64, 128), (6, 5, 8, 8, 64, 128), (2, 17, 8, 8, 64, 128),
                                                 (5, 18, 6, 10, 64, 128)])
def test_pad1_stride2_conv_is_unchanged(cuda, path, n, h, w, cin, cout):
    """The existing Downsample2D (pad 1, stride 2) through the loaders the mode was added to: fp64 at
    the same tolerance, and the same bits from two calls."""
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert planned(path, n, h, w, ho, wo, cin, cout, 2)[0] == path
    x, wt, b, r = conv_operands(n, h, w, ho, wo, cin, cout, seed=7 * path + h)
    got, fo, frames = run_framed(path, n, h, w, ho, wo, x, wt, b, r, stride=2)
    img = x.double().cpu().reshape(n, h, w, cin).permute(0, 3, 1, 2)
    want = F.conv2d(img, wt.double().cpu(), b.double().cpu(), stride=2, padding=1)
    want = want.permute(0, 2, 3, 1).reshape(-1, cout) + r.double().cpu()
    fo.assert_written(want)
    mf.assert_all_intact(*frames)
    mf.close_f32(got, want)
    again, _, _ = run_framed(path, n, h, w, ho, wo, x, wt, b, r, stride=2)
    assert torch.equal(got, again)


# ---------------------------------------------------------------- the encoder
@pytest.fixture(scope="module")
def tiny_vae(cuda):
    return init_synthetic_(AutoencoderKL("tiny", encoder=True), seed=0).to("cuda", BF).prepare()


def test_tiny_encoder_matches_the_fixture(tiny_vae):
    gold = np.load(GOLD / "vae_encoder_tiny.npz")
    x = torch.from_numpy(gold["x"]).cuda()
    dist = tiny_vae.encode(x).latent_dist
    want = torch.from_numpy(gold["moments"])
    assert dist.mean.shape == (2, 4, 16, 16) and dist.mean.dtype == torch.float32 and dist.mean.is_cuda
    assert tiny_vae.encode(x, return_dict=False)[0].parameters.shape == (2, 8, 16, 16)
    for name, got, ref, d_emu in (("mean", dist.mean, want[:, :4], float(gold["d_emu_mean"])),
                                  ("logvar", dist.logvar, want[:, 4:], float(gold["d_emu_logvar"]))):
        err = R.rel_l2(got, ref)
        print(f"tiny encoder {name}: rel-L2 vs fp64 {err:.5f} = {err / d_emu:.2f} x d_emu ({d_emu:.5f})")
        assert err <= 3 * d_emu, (name, err, d_emu)


def test_chunked_encode_is_bit_identical(tiny_vae):
    x = torch.rand((5, 3, 32, 32), generator=torch.Generator().manual_seed(3)) * 2 - 1
    whole = tiny_vae.encode(x.cuda()).latent_dist.parameters.clone()
    tiny_vae.frames_per_chunk = 2
    try:
        parts = tiny_vae.encode(x.cuda()).latent_dist.parameters
    finally:
        tiny_vae.frames_per_chunk = 8
    assert whole.shape == (5, 8, 16, 16) and torch.equal(whole, parts)


def test_full_encoder_one_frame_matches_reference(cuda):
    """The full SD-1.5 encoder (34.2M parameters) on one 256 x 256 frame: every channel width, the
    three pad-end downsamples (256 -> 128 -> 64 -> 32) and the d = 512 attention over 1024 tokens;
    d_emu from the reference's own emulation on the same weights and input."""
    vae = init_synthetic_(AutoencoderKL("full", encoder=True), seed=0).to("cuda", BF).prepare()
    x = (torch.rand((1, 3, 256, 256), generator=torch.Generator().manual_seed(8)) * 2 - 1).to(BF).float()
    dist = vae.encode(x.cuda()).latent_dist
    assert dist.mean.shape == (1, 4, 32, 32)
    sd = {k: v.detach().float().cpu() for k, v in vae.state_dict().items()}
    want = R.moments(sd, VAE_FULL, x)
    emu = R.moments(sd, VAE_FULL, x, rnd=R.bf16_round)
    for name, got, sl in (("mean", dist.mean, slice(0, 4)), ("logvar", dist.logvar, slice(4, 8))):
        d_emu, err = R.rel_l2(emu[:, sl], want[:, sl]), R.rel_l2(got, want[:, sl])
        print(f"full encoder {name}: rel-L2 vs fp64 {err:.5f} = {err / d_emu:.2f} x d_emu ({d_emu:.5f})")
        assert err <= 3 * d_emu, (name, err, d_emu)


# ---------------------------------------------------------------- video to video
@pytest.fixture(scope="module")
def pipe(cuda):
    return AnimateDiffVideoToVideoPipeline.from_config("tiny")


def inputs(frames=2, size=16):
    g = torch.Generator().manual_seed(12)
    video = torch.rand((frames, 3, size, size), generator=g)
    pe = torch.randn((1, 77, 64), generator=g)
    ne = torch.randn((1, 77, 64), generator=g)
    return video, dict(prompt_embeds=pe, negative_prompt_embeds=ne, guidance_scale=7.5)


class SpyLoop(DenoiseLoop):
    made = []

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        SpyLoop.made.append(self)


def call(pipe, video, kw, monkeypatch=None, seed=5, **more):
    args = dict(kw, video=video, generator=torch.Generator().manual_seed(seed), output_type="latent")
    args.update(more)
    if monkeypatch is not None:
        SpyLoop.made.clear()
        monkeypatch.setattr(P, "DenoiseLoop", SpyLoop)
    return pipe(**args).frames


def test_vid2vid_half_strength_runs_two_steps_like_a_hand_driven_loop(pipe, monkeypatch):
    video, kw = inputs()
    out = call(pipe, video, kw, monkeypatch, strength=0.5, num_inference_steps=4).clone()
    (loop,) = SpyLoop.made
    assert loop.n_steps == 2 == loop.issued and int(loop.step_idx.item()) == 2 and loop.graph is not None
    assert out.shape == (1, 4, 2, 8, 8) and out.dtype == torch.float32 and torch.isfinite(out).all()
    monkeypatch.undo()
    # by hand: the same draws, the last two timesteps of the 4-step schedule
    pipe.scheduler.set_timesteps(4)
    ts, n = pipe.get_timesteps(4, 0.5)
    assert n == 2 and torch.equal(ts, pipe.scheduler.timesteps[2:])
    lat = pipe.prepare_latents(P.preprocess_video(video), ts[:1], generator=torch.Generator().manual_seed(5))
    assert lat.shape == (1, 4, 2, 8, 8)
    ehs = torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]])
    want = DenoiseLoop(pipe.unet, pipe.scheduler, lat, ehs, 7.5, timesteps=ts, use_graph=True).prime().run()
    assert torch.equal(out, want)
    # the same generator seed twice: the same video; another seed: another
    assert torch.equal(out, call(pipe, video, kw, strength=0.5, num_inference_steps=4))
    assert not torch.equal(out, call(pipe, video, kw, seed=6, strength=0.5, num_inference_steps=4))
    # without the graph: the existing loop tests' bound (rel-L2 0.01)
    eager = call(pipe, video, kw, strength=0.5, num_inference_steps=4, use_graph=False)
    assert R.rel_l2(eager, out) < 0.01
    # latents= bypasses encoding and noising
    assert torch.equal(pipe(latents=lat, strength=0.5, num_inference_steps=4, output_type="latent", **kw).frames, out)


def test_vid2vid_full_strength_starts_from_add_noise_at_the_first_timestep(pipe, monkeypatch):
    video, kw = inputs()
    out = call(pipe, video, kw, monkeypatch, strength=1.0, num_inference_steps=3).clone()
    (loop,) = SpyLoop.made
    assert loop.n_steps == 3 == loop.issued
    monkeypatch.undo()
    pipe.scheduler.set_timesteps(3)
    g = torch.Generator().manual_seed(5)
    x = P.preprocess_video(video)[0].permute(1, 0, 2, 3)               # (F, 3, H, W) in [-1, 1]
    z = pipe.vae.encode(x).latent_dist.sample(generator=g) * pipe.vae.config["scaling_factor"]
    noise = P.randn_tensor((1, 2, 4, 8, 8), generator=g, device="cuda", dtype=pipe.torch_dtype)
    lat = pipe.scheduler.add_noise(z[None], noise.float(), pipe.scheduler.timesteps[:1]).permute(0, 2, 1, 3, 4)
    ts, _ = pipe.get_timesteps(3, 1.0)
    assert torch.equal(ts, pipe.scheduler.timesteps)
    assert torch.equal(lat, pipe.prepare_latents(P.preprocess_video(video), ts[:1],
                                                 generator=torch.Generator().manual_seed(5)))
    ehs = torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]])
    want = DenoiseLoop(pipe.unet, pipe.scheduler, lat.contiguous(), ehs, 7.5, timesteps=ts).prime().run()
    assert torch.equal(out, want)


def test_vid2vid_euler(cuda, monkeypatch):
    sched = EulerDiscreteScheduler.from_config(None, timestep_spacing="linspace", beta_schedule="linear")
    pipe = AnimateDiffVideoToVideoPipeline.from_config("tiny", scheduler=sched)
    video, kw = inputs()
    out = call(pipe, video, kw, monkeypatch, strength=0.5, num_inference_steps=4).clone()
    (loop,) = SpyLoop.made
    monkeypatch.undo()
    ts, _ = pipe.get_timesteps(4, 0.5)
    i0 = sched.index_for_timestep(ts[0])
    assert loop.n_steps == 2 and loop.kind == "euler" and i0 == 2 and loop.in_div0 == sched.input_divisor(i0)
    lat = pipe.prepare_latents(P.preprocess_video(video), ts[:1], generator=torch.Generator().manual_seed(5))
    ehs = torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]])
    want = DenoiseLoop(pipe.unet, sched, lat, ehs, 7.5, timesteps=ts).prime().run()
    assert torch.equal(out, want) and torch.isfinite(out).all()


def test_vid2vid_output_types(pipe):
    from PIL import Image
    video, kw = inputs()
    lat = call(pipe, video, kw, strength=0.5, num_inference_steps=2)
    assert lat.shape == (1, 4, 2, 8, 8)
    pt = call(pipe, video, kw, strength=0.5, num_inference_steps=2, output_type="pt")
    assert pt.shape == (1, 2, 3, 16, 16) and float(pt.min()) >= 0 and float(pt.max()) <= 1
    frames = [Image.fromarray((f.permute(1, 2, 0).numpy() * 255).round().astype("uint8")) for f in video]
    pil = call(pipe, frames, kw, strength=0.5, num_inference_steps=2, output_type="pil")
    assert len(pil) == 1 and len(pil[0]) == 2 and pil[0][0].size == (16, 16)
    with pytest.raises(ValueError, match="strength"):
        call(pipe, video, kw, strength=0.0, num_inference_steps=2)
