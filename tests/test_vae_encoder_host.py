"""The VAE encoder and the video-to-video pipeline, everything that needs no GPU: the module tree
and its parameter counts, the synthetic weight stream, checkpoint loading, the pad-end conv
descriptor's argument checks and plan, the fp64 reference and its committed fixture, the posterior,
the schedulers' add_noise, get_timesteps and the video input forms."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

import vae_encoder_ref as R
import vdiff._lib as L
from vdiff import (AnimateDiffVideoToVideoPipeline, AutoencoderKL, DDIMScheduler, DiagonalGaussianDistribution,
                   EulerDiscreteScheduler, init_synthetic_, ops)
from vdiff.models.vae import VAE_FULL, VAE_TINY
from vdiff.pipeline import preprocess_video
from vdiff.pretrained import load_vae
from vdiff.sched.ddim import sqrt32

GOLD = Path(__file__).resolve().parent / "golden"
EINVAL = 1000
VAE_CFG = {"_class_name": "AutoencoderKL", "act_fn": "silu", "block_out_channels": [64, 64], "in_channels": 3,
           "latent_channels": 4, "layers_per_block": 1, "norm_num_groups": 32, "out_channels": 3,
           "sample_size": 32, "scaling_factor": 0.18215}


def count(m):
    return sum(p.numel() for p in m.parameters())


# ---------------------------------------------------------------- structure
def _conv(ci, co, k):
    return co * ci * k * k + co


def _resnet(ci, co):
    return 2 * ci + _conv(ci, co, 3) + 2 * co + _conv(co, co, 3) + (_conv(ci, co, 1) if ci != co else 0)


def _encoder_params(cfg):
    """Closed form over diffusers' Encoder: conv_in, the down blocks, the mid block (2 resnets + one
    attention: GroupNorm + 4 biased Linears), conv_norm_out, conv_out."""
    ch, lpb, lc = cfg["block_out_channels"], cfg["layers_per_block"], cfg["latent_channels"]
    n, prev = _conv(cfg["in_channels"], ch[0], 3), ch[0]
    for i, c in enumerate(ch):
        n += sum(_resnet(prev if j == 0 else c, c) for j in range(lpb))
        n += _conv(c, c, 3) if i < len(ch) - 1 else 0
        prev = c
    c = ch[-1]
    n += 2 * _resnet(c, c) + 2 * c + 4 * (c * c + c)
    return n + 2 * c + _conv(c, 2 * lc, 3)


def test_encoder_tree_and_parameter_counts():
    assert _encoder_params(VAE_FULL) == 34_163_592 and _encoder_params(VAE_TINY) == 356_680
    with torch.device("meta"):
        full, dec = AutoencoderKL("full", encoder=True), AutoencoderKL("full")
    assert count(dec) == 49_490_199 and dec.encoder is None and dec.quant_conv is None
    assert count(full.encoder) == 34_163_592 and count(full.quant_conv) == 72
    assert count(full) == 83_653_863 == 49_490_199 + 34_163_592 + 72
    tiny = AutoencoderKL("tiny", encoder=True)
    assert count(tiny.encoder) == 356_680
    keys = set(full.state_dict())
    for k in ("encoder.conv_in.weight", "encoder.down_blocks.0.resnets.1.conv2.bias",
              "encoder.down_blocks.1.resnets.0.conv_shortcut.weight", "encoder.down_blocks.2.downsamplers.0.conv.weight",
              "encoder.mid_block.resnets.1.norm2.weight", "encoder.mid_block.attentions.0.to_out.0.bias",
              "encoder.mid_block.attentions.0.group_norm.weight", "encoder.conv_norm_out.bias",
              "encoder.conv_out.weight", "quant_conv.weight", "quant_conv.bias", "post_quant_conv.weight"):
        assert k in keys, k
    assert not any(k.startswith("encoder.down_blocks.3.downsamplers") for k in keys)
    assert full.encoder.down_blocks[3].downsamplers is None and len(full.encoder.down_blocks) == 4
    assert all(len(b.resnets) == 2 for b in full.encoder.down_blocks)
    assert tuple(full.state_dict()["encoder.conv_out.weight"].shape) == (8, 512, 3, 3)
    assert tuple(full.state_dict()["quant_conv.weight"].shape) == (8, 8, 1, 1)
    d = full.encoder.down_blocks[0].downsamplers[0].conv
    assert d.stride == (2, 2) and d.padding == (0, 0)
    assert not any(k.startswith(("encoder.", "quant_conv.")) for k in dec.state_dict())


def test_synthetic_weight_stream_of_the_decoder_does_not_move():
    a = init_synthetic_(AutoencoderKL("tiny"), seed=0).state_dict()
    b = init_synthetic_(AutoencoderKL("tiny", encoder=True), seed=0).state_dict()
    assert list(b)[:len(a)] == list(a)  # encoder and quant_conv come after everything the decoder-only model has
    for k, v in a.items():
        assert torch.equal(v, b[k]), k
    assert all(k.startswith(("encoder.", "quant_conv.")) for k in list(b)[len(a):])


def test_chunk_of_eight_frames_fits_the_gemm_offsets():
    """8 frames of the first level's 512 x 512 x 128 activation: 0.5 GiB of bf16, M * ldc = 2^28 <
    2^31 (vd_gemm's check) and below the LDS-DMA kernels' 2^31-byte buffer bound."""
    with torch.device("meta"):
        m = AutoencoderKL("full", encoder=True)
    M = m.frames_per_chunk * 512 * 512
    c = VAE_FULL["block_out_channels"][0]
    assert m.frames_per_chunk == 8 and M * c == 1 << 28 and M * c < 0x7fffffff
    assert M * c * 2 == 1 << 29 and M * c * 2 < 0x80000000


# ---------------------------------------------------------------- loading
def _write(folder, sd):
    folder.mkdir(parents=True, exist_ok=True)
    (folder / "config.json").write_text(json.dumps(VAE_CFG))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(folder / "diffusion_pytorch_model.safetensors"))


def test_load_vae_builds_the_encoder_only_from_a_complete_checkpoint(tmp_path):
    src = init_synthetic_(AutoencoderKL("tiny", encoder=True), seed=3)
    sd = {k: v.float() for k, v in src.state_dict().items()}
    _write(tmp_path / "whole", sd)
    vae = load_vae(tmp_path / "whole", device="cpu")
    got = vae.state_dict()
    assert vae.encoder is not None and set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v.to(torch.bfloat16)), k
    # one encoder tensor missing: the decoder-only model, as for a checkpoint with no encoder at all
    part = {k: v for k, v in sd.items() if k != "encoder.mid_block.attentions.0.to_k.bias"}
    _write(tmp_path / "part", part)
    dec = load_vae(tmp_path / "part", device="cpu")
    want = {k for k in sd if not k.startswith(("encoder.", "quant_conv."))}
    assert dec.encoder is None and dec.quant_conv is None and set(dec.state_dict()) == want
    for k in want:
        assert torch.equal(dec.state_dict()[k], sd[k].to(torch.bfloat16)), k
    with pytest.raises(ValueError, match="encoder=True"):
        dec.encode(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match="encoder=True"):
        AutoencoderKL("tiny").encode(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match="multiples of 8"):
        vae.encode(torch.zeros(1, 3, 36, 32))


def test_vid2vid_pipeline_refuses_a_decoder_only_vae():
    p = AnimateDiffVideoToVideoPipeline.__new__(AnimateDiffVideoToVideoPipeline)

    class U:
        config = {"cross_attention_dim": 64}
    with pytest.raises(ValueError, match="encoder"):
        AnimateDiffVideoToVideoPipeline.__init__(p, U(), vae=AutoencoderKL("tiny"))
    with pytest.raises(ValueError, match="encoder"):
        AnimateDiffVideoToVideoPipeline.__init__(p, U(), vae=None)


# ---------------------------------------------------------------- descriptor checks, no launch
PAD_END = ops.CONV_PAD_END


def _desc(p, *, h_in=8, w_in=8, h_out=4, w_out=4, stride=2 | PAD_END, n_img=3, cin=64, cout=64, M=None, **kw):
    K = cin * 9
    d = L.GemmDesc(a0=p, lda0=cin, k0=cin, a_mode=ops.A_CONV3X3, n_img=n_img, h_in=h_in, w_in=w_in, h_out=h_out,
                   w_out=w_out, stride=stride, upsample=0, w=p, ldw=K, M=n_img * h_out * w_out if M is None else M,
                   N=cout, K=K, out=p, ldc=cout)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_pad_end_descriptor_is_validated_before_launch():
    assert PAD_END == 0x100
    h = L.lib()
    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 255) & ~255

    def rc(d):
        return h.vd_gemm(ctypes.byref(d), None)
    # M = 0 returns after the flag's own checks and before everything else: the flag alone decides
    assert rc(_desc(p, M=0)) == 0
    assert rc(_desc(p, M=0, stride=2)) == 0
    assert rc(_desc(p, M=0, stride=1 | PAD_END)) == EINVAL
    assert rc(_desc(p, M=0, upsample=1)) == EINVAL
    assert rc(_desc(p, M=0, kt=3, frames_in=3, frames_out=3, K=64 * 27, ldw=64 * 27)) == EINVAL
    assert rc(_desc(p, M=0, ks=1, K=64, ldw=64)) == EINVAL
    for stray in (2 | 0x200, 2 | PAD_END | 0x400, 1 | 0x1000, 2 | PAD_END | (1 << 30), -2):
        assert rc(_desc(p, M=0, stride=stray)) == EINVAL, hex(stray)
    # the same with rows to compute
    assert rc(_desc(p, stride=1 | PAD_END, h_out=8, w_out=8)) == EINVAL
    assert rc(_desc(p, upsample=1, h_out=16, w_out=16)) == EINVAL
    assert rc(_desc(p, kt=3, frames_in=3, frames_out=3, K=64 * 27, ldw=64 * 27)) == EINVAL
    assert rc(_desc(p, ks=1, K=64, ldw=64)) == EINVAL
    assert rc(_desc(p, stride=2 | 0x200)) == EINVAL
    # odd input: the mode's size is (7 - 2) // 2 + 1 = 3 by 2; pad-1's 4 by 3 is refused
    assert rc(_desc(p, h_in=7, w_in=5, h_out=4, w_out=3)) == EINVAL
    assert rc(_desc(p, h_in=7, w_in=5, h_out=3, w_out=3)) == EINVAL
    assert rc(_desc(p, h_in=1, w_in=8, h_out=1, w_out=4)) == EINVAL


@pytest.mark.parametrize("hw,cin", [(512, 128), (256, 256), (128, 512)])
@pytest.mark.parametrize("path", [0, 1, 2, 5, 6])
def test_plan_does_not_see_the_flag(hw, cin, path):
    """The encoder's three downsamples at 8 frames (and one frame): kernel, split and workspace are
    those of plain stride 2, under the automatic plan and under every forced path."""
    h = L.lib()
    for n_img in (8, 1):
        got = []
        for stride in (2, 2 | PAD_END):
            d = _desc(256, h_in=hw, w_in=hw, h_out=hw // 2, w_out=hw // 2, stride=stride, n_img=n_img, cin=cin,
                      cout=cin, path=path)
            k, sp = ctypes.c_int32(-1), ctypes.c_int32(-1)
            assert h.vd_gemm_plan(ctypes.byref(d), ctypes.byref(k), ctypes.byref(sp)) == 0
            got.append((k.value, sp.value, h.vd_gemm_ws_bytes(ctypes.byref(d))))
        assert got[0] == got[1] and got[0][0] in (1, 2, 5, 6)


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("hw,out", [((8, 8), (4, 4)), ((7, 5), (3, 2)), ((6, 10), (3, 5)), ((2, 2), (1, 1)),
                                    ((3, 3), (1, 1))])
def test_reference_downsample_is_the_tap_sum(hw, out):
    g = torch.Generator().manual_seed(hw[0] * 16 + hw[1])
    x = torch.randn((2, 3, *hw), generator=g, dtype=torch.float64)
    w = torch.randn((5, 3, 3, 3), generator=g, dtype=torch.float64)
    b = torch.randn((5,), generator=g, dtype=torch.float64)
    got, want = R.downsample(x, w, b), R.downsample_taps(x, w, b)
    assert tuple(got.shape[-2:]) == out == tuple(want.shape[-2:])
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    if hw[0] % 2 == 0 and hw[1] % 2 == 0:  # not the pad-1 conv: the zero band is on the other side
        assert not torch.allclose(got, torch.nn.functional.conv2d(x, w, b, stride=2, padding=1))


def test_fixture_is_the_reference():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_vae_encoder_golden", GOLD / "make_vae_encoder_golden.py")
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    gold = np.load(GOLD / "vae_encoder_tiny.npz")
    sd, x = mk.tiny_inputs()
    assert np.array_equal(gold["x"], x.numpy()) and gold["moments"].dtype == np.float64
    want = R.moments(sd, VAE_TINY, x)
    np.testing.assert_allclose(gold["moments"], want.numpy(), rtol=1e-9, atol=1e-12)
    emu = torch.from_numpy(gold["moments_bf16emu"])
    assert abs(R.rel_l2(emu[:, :4], want[:, :4]) - float(gold["d_emu_mean"])) < 1e-9
    assert abs(R.rel_l2(emu[:, 4:], want[:, 4:]) - float(gold["d_emu_logvar"])) < 1e-9
    # bf16 storage moves the result by about 2^-8 per stage, not by nothing and not by percents
    assert 1e-3 < float(gold["d_emu_mean"]) < 2e-2 and 1e-3 < float(gold["d_emu_logvar"]) < 2e-2


# ---------------------------------------------------------------- posterior
def test_diagonal_gaussian_distribution():
    g = torch.Generator().manual_seed(0)
    p = torch.randn((2, 8, 4, 4), generator=g)
    p[0, 4, 0, 0], p[0, 5, 1, 1] = 55.0, -70.0   # logvar outside [-30, 20]
    d = DiagonalGaussianDistribution(p)
    lv = p[:, 4:].clamp(-30.0, 20.0)
    assert torch.equal(d.mean, p[:, :4]) and torch.equal(d.logvar, lv) and torch.equal(d.mode(), p[:, :4])
    assert d.logvar[0, 0, 0, 0] == 20.0 and d.logvar[0, 1, 1, 1] == -30.0
    assert torch.equal(d.std, torch.exp(0.5 * lv)) and torch.equal(d.var, torch.exp(lv))
    s1 = d.sample(generator=torch.Generator().manual_seed(9))
    s2 = d.sample(generator=torch.Generator().manual_seed(9))
    noise = torch.randn(d.mean.shape, generator=torch.Generator().manual_seed(9))
    assert torch.equal(s1, s2) and torch.equal(s1, d.mean + d.std * noise)
    assert not torch.equal(s1, d.sample(generator=torch.Generator().manual_seed(10)))
    kl = 0.5 * (d.mean.double() ** 2 + torch.exp(lv.double()) - 1 - lv.double()).sum((1, 2, 3))
    torch.testing.assert_close(d.kl().double(), kl, rtol=1e-5, atol=1e-5)
    assert d.kl().shape == (2,)
    torch.testing.assert_close(d.kl(d), torch.zeros(2), rtol=0, atol=1e-3 * float(kl.max()))


# ---------------------------------------------------------------- add_noise
def test_ddim_add_noise_is_the_formula():
    s = DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)
    s.set_timesteps(50)
    g = torch.Generator().manual_seed(1)
    x, n = torch.randn((2, 3, 4, 5, 5), generator=g), torch.randn((2, 3, 4, 5, 5), generator=g)
    for t in (int(s.timesteps[0]), int(s.timesteps[10]), 1):
        a = s.alphas_cumprod[t]
        want = sqrt32(a) * x + sqrt32(1 - a) * n
        assert torch.equal(s.add_noise(x, n, torch.tensor([t])), want)
        assert torch.equal(s.add_noise(x, n, t), want)
        # torch's own fp32 ** 0.5 (diffusers' expression) is within an ulp of the correctly rounded root
        torch.testing.assert_close(want, a ** 0.5 * x + (1 - a) ** 0.5 * n, rtol=3e-7, atol=1e-6)
    ts = torch.tensor([981, 1])
    want = torch.stack([sqrt32(s.alphas_cumprod[t]) * x[i] + sqrt32(1 - s.alphas_cumprod[t]) * n[i]
                        for i, t in enumerate(ts.tolist())])
    got = s.add_noise(x, n, ts)
    assert torch.equal(got, want) and got.dtype == torch.float32
    assert s.add_noise(x.half(), n.half(), 981).dtype == torch.float32


def test_euler_add_noise_is_the_formula():
    s = EulerDiscreteScheduler.from_config(None, timestep_spacing="linspace", beta_schedule="linear")
    s.set_timesteps(25)
    g = torch.Generator().manual_seed(2)
    x, n = torch.randn((1, 4, 3, 6, 6), generator=g), torch.randn((1, 4, 3, 6, 6), generator=g)
    for i in (0, 7, 24):
        t = s.timesteps[i]
        assert s.index_for_timestep(t) == i
        assert torch.equal(s.add_noise(x, n, t.reshape(1)), x + n * s.sigmas[i])
    assert torch.equal(s.add_noise(x, n, s.timesteps[0]), x + n * s.sigmas.max())
    with pytest.raises(ValueError, match="not in the schedule"):
        s.add_noise(x, n, torch.tensor([3.25]))


# ---------------------------------------------------------------- get_timesteps, video input
def _bare_pipe(sched):
    p = AnimateDiffVideoToVideoPipeline.__new__(AnimateDiffVideoToVideoPipeline)
    p.scheduler = sched
    return p


@pytest.mark.parametrize("n,strength,run", [(50, 0.8, 40), (25, 1.0, 25), (4, 0.5, 2)])
def test_get_timesteps(n, strength, run):
    for s in (DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False),
              EulerDiscreteScheduler.from_config(None, timestep_spacing="linspace", beta_schedule="linear")):
        s.set_timesteps(n)
        ts, k = _bare_pipe(s).get_timesteps(n, strength)
        assert k == run == len(ts) and torch.equal(ts, s.timesteps[n - run:])


def test_get_timesteps_refuses_what_leaves_no_step():
    s = DDIMScheduler()
    s.set_timesteps(10)
    p = _bare_pipe(s)
    with pytest.raises(ValueError, match="no step"):
        p.get_timesteps(10, 0.05)
    for bad in (0.0, -0.1, 1.01):
        with pytest.raises(ValueError, match="strength"):
            p.get_timesteps(10, bad)


def test_video_input_forms():
    from PIL import Image
    g = torch.Generator().manual_seed(4)
    t = torch.rand((3, 3, 16, 24), generator=g)                       # (F, 3, H, W) in [0, 1]
    want = (2 * t - 1).permute(1, 0, 2, 3)[None]
    got = preprocess_video(t)
    assert got.shape == (1, 3, 3, 16, 24) and got.dtype == torch.float32 and torch.equal(got, want)
    two = preprocess_video(torch.stack([t, t.flip(0)]))               # (B, F, 3, H, W)
    assert two.shape == (2, 3, 3, 16, 24) and torch.equal(two[0], want[0]) and torch.equal(two[1], want[0].flip(1))
    a = t.permute(0, 2, 3, 1).numpy()                                  # (F, H, W, 3)
    assert torch.equal(preprocess_video(a), want)
    assert torch.equal(preprocess_video(np.stack([a, a])), torch.cat([want, want]))
    assert torch.equal(preprocess_video(a, height=16, width=24), want)
    frames = [Image.fromarray((f * 255).round().astype("uint8")) for f in a]
    q = torch.from_numpy(np.stack([np.asarray(f, dtype=np.float32) / 255.0 for f in frames])).permute(3, 0, 1, 2)[None]
    pil = preprocess_video(frames)
    assert torch.equal(pil, 2 * q - 1) and float((pil - want).abs().max()) <= 1.0 / 255 + 1e-6
    assert torch.equal(preprocess_video([frames, frames]), torch.cat([pil, pil]))
    # PIL frames of another size are resized with LANCZOS; arrays and tensors are refused
    small = preprocess_video(frames, height=8, width=16)
    ref = np.stack([np.asarray(f.resize((16, 8), Image.LANCZOS), dtype=np.float32) / 255.0 for f in frames])
    assert small.shape == (1, 3, 3, 8, 16)
    assert torch.equal(small, 2 * torch.from_numpy(ref).permute(3, 0, 1, 2)[None] - 1)
    for v in (a, t):
        with pytest.raises(ValueError, match="only PIL frames are resized"):
            preprocess_video(v, height=8, width=16)
    with pytest.raises(ValueError, match="multiples of 8"):
        preprocess_video(torch.rand(2, 3, 12, 16))
    with pytest.raises(ValueError):
        preprocess_video(torch.rand(2, 4, 16, 16))
    with pytest.raises(ValueError, match="same number of frames"):
        preprocess_video([frames, frames[:2]])
    assert float(got.min()) >= -1 and float(got.max()) <= 1
