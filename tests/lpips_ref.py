"""Plain-torch restatement of lpips.LPIPS(net='alex', version='0.1') in eval mode, as the reference's
LPIPSMetric calls it (experiments/06_measure_grid_search.py:122-154), over consecutive frames.

Test infrastructure (like tests/parity_blocks.py): the dtype is a parameter, so the same code is
the fp64 reference of tests/test_gpu_lpips.py and an fp32 CPU run.  It also states the seeded
synthetic weights (no AlexNet checkpoint exists offline) and can perturb every conv output by
+-1e-6 (|x| * |w| + |b|) with random signs — the derived error bound of an fp32 k-ordered chain —
which gives each test case its own conditioning floor.

Contract, per uint8 RGB image u: x = 2 u / 255 - 1; (x - shift) / scale per channel; the five
ReLU taps of torchvision AlexNet `features` (zero padding applies to the scaled tensor);
MaxPool2d(3, 2) before conv 2 and conv 3.  Per pair and tap: n = f / (sqrt(sum_c f^2) + 1e-10)
per pixel, d = mean over pixels of sum_c lin[c] (n_a - n_b)^2; LPIPS = sum of the five d.
"""
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (index in torchvision's features, Cin, Cout, k, stride, pad); a MaxPool2d(3, 2) before conv 2 and 3
CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1),
         (10, 256, 256, 3, 1, 1))
EPS_CONV = 1e-6  # the elementwise conv bound, relative to |x| * |w| + |b|


def synthetic_state_dicts(seed: int):
    """(torchvision-AlexNet-layout, lpips-alex.pth-layout) fp32 state dicts: conv weights
    randn * sqrt(2 / (Cin k^2)), biases 0.1 randn, lin vectors |randn| / sqrt(C)."""
    g = torch.Generator().manual_seed(seed)
    alex, lin = {}, {}
    for l, (idx, cin, cout, k, _, _) in enumerate(CONVS):
        alex[f"features.{idx}.weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        alex[f"features.{idx}.bias"] = 0.1 * torch.randn(cout, generator=g)
        lin[f"lin{l}.model.1.weight"] = (torch.randn(cout, generator=g).abs() / cout ** 0.5).reshape(1, cout, 1, 1)
    return alex, lin


def full_state_dict(alex: dict, lin: dict, lins_alias: bool = True) -> dict:
    """The same weights under the keys of lpips.LPIPS(net='alex').state_dict()."""
    sd = {"scaling_layer.shift": torch.tensor(SHIFT).reshape(1, 3, 1, 1),
          "scaling_layer.scale": torch.tensor(SCALE).reshape(1, 3, 1, 1)}
    for l, (idx, *_rest) in enumerate(CONVS):
        for p in ("weight", "bias"):
            sd[f"net.slice{l + 1}.{idx}.{p}"] = alex[f"features.{idx}.{p}"]
        sd[f"lin{l}.model.1.weight"] = lin[f"lin{l}.model.1.weight"]
        if lins_alias:
            sd[f"lins.{l}.model.1.weight"] = lin[f"lin{l}.model.1.weight"]
    return sd


def scale_input(frames_u8: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """uint8 [N, H, W, 3] -> the ScalingLayer's output, NCHW."""
    x = 2 * (frames_u8.to(dtype) / 255) - 1
    x = (x - torch.tensor(SHIFT, dtype=dtype)) / torch.tensor(SCALE, dtype=dtype)
    return x.permute(0, 3, 1, 2).contiguous()


def conv_bound(x, w, b, stride, pad):
    """|x| * |w| + |b|: the magnitude the fp32 chain's rounding error is relative to."""
    m = F.conv2d(x.abs(), w.abs(), None, stride, pad)
    return m if b is None else m + b.abs().reshape(1, -1, 1, 1)


def taps(frames_u8, alex, dtype=torch.float64, perturb_seed=None):
    """The five ReLU taps (NCHW) of uint8 frames [N, H, W, 3]."""
    g = None if perturb_seed is None else torch.Generator().manual_seed(perturb_seed)
    x = scale_input(frames_u8, dtype)
    out = []
    for l, (idx, _, _, _, stride, pad) in enumerate(CONVS):
        if l in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        w, b = alex[f"features.{idx}.weight"].to(dtype), alex[f"features.{idx}.bias"].to(dtype)
        y = F.conv2d(x, w, b, stride, pad)
        if g is not None:
            sign = torch.randint(0, 2, y.shape, generator=g).to(dtype) * 2 - 1
            y = y + sign * EPS_CONV * conv_bound(x, w, b, stride, pad)
        x = F.relu(y)
        out.append(x)
    return out


def layer_distance(fa, fb, lin):
    """NCHW features of the two sides of each pair, lin [C] -> [pairs]."""
    na = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    nb = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((na - nb).pow(2) * lin.reshape(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips_pairs(videos_u8, alex, lin, dtype=torch.float64, perturb_seed=None):
    """uint8 [V, F, H, W, 3] -> [V, F-1]: LPIPS of every consecutive pair of each video."""
    V, Fr = videos_u8.shape[:2]
    feats = taps(videos_u8.reshape(V * Fr, *videos_u8.shape[2:]), alex, dtype, perturb_seed)
    total = torch.zeros(V, Fr - 1, dtype=dtype)
    for l, f in enumerate(feats):
        f = f.reshape(V, Fr, *f.shape[1:])
        wl = lin[f"lin{l}.model.1.weight"].to(dtype).reshape(-1)
        for v in range(V):
            total[v] += layer_distance(f[v, :-1], f[v, 1:], wl)
    return total


def conditioning_floor(videos_u8, alex, lin, ref=None, seeds=(0, 1, 2)) -> float:
    """Worst relative LPIPS change over the pairs when every conv output of the fp64 run is moved by
    +-EPS_CONV (|x| * |w| + |b|) with random signs, over the given seeds."""
    ref = lpips_pairs(videos_u8, alex, lin) if ref is None else ref
    worst = 0.0
    for s in seeds:
        got = lpips_pairs(videos_u8, alex, lin, perturb_seed=s)
        worst = max(worst, ((got - ref).abs() / ref.abs()).max().item())
    return worst
