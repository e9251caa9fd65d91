"""LPIPS (AlexNet) on the MI355X: the exact-fp32 MFMA convolution, the per-tap distance kernel and
the whole metric, against the fp64 restatement tests/lpips_ref.py with seeded synthetic weights.

Bounds are derived, not measured:
  conv        |dev - ref| <= 1e-6 (|x| * |w| + |b|) elementwise — a k-ordered fp32 fmaf chain is
              within 3.5e-7 sum|a b| of fp64 at K = 4096; 3x margin.
  distance    relative 3e-5 — a C-term fp32 sum of non-negative terms (C 2^-24 <= 2.3e-5 at
              C = 384) plus a few roundings from sqrt / divide.
  end to end  4x the case's own conditioning floor: the worst relative LPIPS change of the fp64
              restatement when every conv output moves by +-1e-6 (|x| * |w| + |b|) with random signs
              (seeds 0, 1, 2; the margin covers three draws under-sampling the worst sign
              pattern).  A floor above 2.5e-5 means an ill-conditioned case and fails as such.
"""
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import lpips_ref
from oracle import metrics_ref
from vdiff import metrics, ops

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden" / "metrics" / "portrait_cfg9.0_steps25"
MAX_FLOOR = 2.5e-5


@pytest.fixture(scope="module")
def weights():
    return lpips_ref.synthetic_state_dicts(1)


@pytest.fixture(scope="module")
def model(cuda):
    return metrics.LPIPS.synthetic(1, device=cuda)


# ---------------------------------------------------------------- convolution alone
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("cin,cout,k,stride,pad,N,H,W", [
    (3, 64, 11, 4, 2, 2, 64, 48),      # Cin = 3 (scalar loader), K = 363 padded to 384
    (3, 64, 11, 4, 2, 1, 31, 31),
    (64, 192, 5, 1, 2, 3, 7, 5),       # ragged M = 105
    (192, 384, 3, 1, 1, 2, 3, 2),      # M = 12, smaller than a tile
    (384, 256, 3, 1, 1, 1, 31, 31),    # K = 3456
])
def test_conv2d_f32_against_fp64(cuda, cin, cout, k, stride, pad, N, H, W, relu):
    g = torch.Generator().manual_seed(cin * 1000 + H * W + k)
    if cin == 3:  # ScalingLayer'd uint8 frames, with a saturated block reaching the image border
        u = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
        u[0, :9, -13:] = 255
        x = lpips_ref.scale_input(u, torch.float32)
    else:         # ReLU-like features, with a block at the maximum in a corner
        x = torch.randn(N, cin, H, W, generator=g).clamp_min(0)
        x[0, :, :2, -2:] = x.max()
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride, pad)
    bound = 1e-6 * lpips_ref.conv_bound(x.double(), w.double(), b.double(), stride, pad)
    if relu:
        ref = ref.clamp_min(0)
    y = ops.conv2d_f32(x.permute(0, 2, 3, 1).contiguous().to(cuda), w.permute(0, 2, 3, 1).contiguous().to(cuda),
                       b.to(cuda), stride=stride, pad=pad, relu=relu)
    assert tuple(y.shape) == (N, ref.shape[2], ref.shape[3], cout)
    err = (y.cpu().double().permute(0, 3, 1, 2) - ref).abs()
    print(f"conv ({cin},{cout},{k},{stride},{pad}) {N}x{H}x{W} relu={relu}: worst |err| / bound "
          f"{(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------- distance kernel alone
@pytest.mark.parametrize("pairs", [1, 4])
@pytest.mark.parametrize("pixels", [6, 165, 961])
@pytest.mark.parametrize("C", [64, 192, 384, 256])
def test_lpips_layer_against_fp64(cuda, C, pixels, pairs):
    g = torch.Generator().manual_seed(C + pixels + pairs)
    fa = torch.randn(pairs, pixels, C, generator=g).clamp_min(0)
    fb = torch.randn(pairs, pixels, C, generator=g).clamp_min(0)
    fa[:, 1] = 0                 # a zero vector in one map: normalises to 0 through the +1e-10
    fa[:, 3] = 0
    fb[:, 3] = 0                 # ... and in both
    fb[:, pixels - 1] = 0
    if pairs > 1:
        fb[2] = fa[2]            # an identical pair
    lin = torch.randn(C, generator=g).abs() / C ** 0.5

    def nchw(f):
        return f.double().permute(0, 2, 1)[..., None]
    ref = lpips_ref.layer_distance(nchw(fa), nchw(fb), lin.double())
    out = ops.lpips_layer(fa.to(cuda), fb.to(cuda), lin.to(cuda))
    assert out.dtype == torch.float64 and tuple(out.shape) == (pairs,)
    got = out.cpu()
    if pairs > 1:
        assert got[2].item() == 0.0
    keep = ref > 0
    rel = ((got - ref).abs()[keep] / ref[keep]).max().item()
    print(f"distance C={C} pixels={pixels} pairs={pairs}: worst relative error {rel:.2e}")
    assert rel <= 3e-5
    # accumulate adds onto out
    twice = ops.lpips_layer(fa.to(cuda), fb.to(cuda), lin.to(cuda), out=out.clone(), accumulate=True).cpu()
    assert torch.equal(twice, got + got)


# ---------------------------------------------------------------- end to end
def _noise_video(g, V, Fr, H, W):
    return torch.randint(0, 256, (V, Fr, H, W, 3), generator=g, dtype=torch.uint8)


def _smooth_video(g, V, Fr, H, W, shift=1.0):
    """tests/test_gpu_metrics.py's _smooth_video with three channels: a band-limited random
    texture translated by `shift` px per frame."""
    base = torch.randn(V, 3, H + 8 * Fr, W + 8 * Fr, generator=g)
    base = F.avg_pool2d(base, 5, 1, 2)
    base = F.avg_pool2d(base, 5, 1, 2)
    frames = []
    for f in range(Fr):
        o = int(round(f * shift))
        frames.append(base[:, :, o:o + H, o:o + W])
    v = torch.stack(frames, 1)
    v = (v - v.amin()) / (v.amax() - v.amin())
    return (v.permute(0, 1, 3, 4, 2) * 255).round().to(torch.uint8).contiguous()


def _check_against_restatement(what, x, got, weights):
    alex, lin = weights
    ref = lpips_ref.lpips_pairs(x, alex, lin)
    floor = lpips_ref.conditioning_floor(x, alex, lin, ref)
    dev = ((got.cpu() - ref).abs() / ref.abs()).max().item()
    print(f"| {what} | {ref.mean().item():.4f} | {floor:.2e} | {dev:.2e} | {dev / floor:.2f} |")
    assert floor <= MAX_FLOOR, f"ill-conditioned case (floor {floor:.2e}): the test is misconfigured"
    assert dev <= 4 * floor, f"device deviates {dev:.2e} from fp64, floor {floor:.2e}"
    return ref, floor


@pytest.mark.parametrize("kind", ["noise", "texture"])
@pytest.mark.parametrize("V,Fr,H,W", [(2, 3, 64, 48), (1, 2, 31, 31), (1, 4, 100, 75), (1, 2, 512, 512)])
def test_lpips_end_to_end_against_fp64(cuda, model, weights, V, Fr, H, W, kind):
    g = torch.Generator().manual_seed(H * W + Fr)
    x = _noise_video(g, V, Fr, H, W) if kind == "noise" else _smooth_video(g, V, Fr, H, W)
    got = model(x.to(cuda))
    assert got.dtype == torch.float64 and tuple(got.shape) == (V, Fr - 1)
    _check_against_restatement(f"{kind} {V}x{Fr}x{H}x{W}", x, got, weights)


def test_lpips_deterministic_and_batch_independent(cuda, model):
    g = torch.Generator().manual_seed(5)
    x = _noise_video(g, 3, 3, 64, 48)
    x[2, 2] = x[2, 1]            # identical consecutive frames
    xd = x.to(cuda)
    a, b = model(xd), model(xd)
    assert torch.equal(a, b)
    assert torch.equal(model(xd[1:2])[0], a[1])          # video 1 alone == video 1 in the batch
    assert torch.equal(model(xd, workspace_cap=1)[1], a[1])  # ... and under one-video groups
    assert a[2, 1].item() == 0.0 and a[2, 0].item() > 0.0


def test_lpips_rejects_bad_input(cuda, model):
    with pytest.raises(ValueError):
        model(torch.zeros(1, 2, 30, 64, 3, dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError):
        model(torch.zeros(1, 1, 64, 64, 3, dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError, match="no CPU fallback"):
        model(torch.zeros(1, 2, 64, 64, 3, dtype=torch.uint8))


def test_measure_videos_with_lpips_on_golden_frames(cuda, model, weights):
    frames = torch.from_numpy(metrics.load_frames(GOLD / "frames")[:4])[None]
    x = frames.to(cuda)
    rec = metrics.measure_videos(x, lpips=model, flow=False)[0]
    per_pair = torch.tensor([[m["lpips"] for m in rec["frame_metrics"]]], dtype=torch.float64)
    ref, floor = _check_against_restatement("golden portrait_cfg9.0_steps25[:4]", frames, per_pair, weights)
    ref = ref[0].numpy()
    # mean / population std of values each within 4 floors of the restatement's
    tol = 4 * floor
    assert rec["mean_lpips"] == pytest.approx(ref.mean(), rel=tol)
    assert rec["std_lpips"] == pytest.approx(ref.std(), abs=tol * ref.max())
    mse = [m["mse"] for m in rec["frame_metrics"]]
    lp = [m["lpips"] for m in rec["frame_metrics"]]
    assert rec["temporal_consistency_score"] == pytest.approx(metrics_ref.consistency_score(mse, lp), rel=1e-12)
    # the other forms of the argument are unchanged
    assert metrics.measure_videos(x, flow=False)[0]["mean_lpips"] is None
    assert metrics.measure_videos(x, lpips=[lp], flow=False)[0]["mean_lpips"] == rec["mean_lpips"]
