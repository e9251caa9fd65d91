"""Structured inputs, fp64 references, planted faults and the half-ulp bound of the norm tests
(tests/test_norm_bound_host.py on the CPU, tests/test_gpu_norm_stats.py on the GPU).

Why: on i.i.d. data every subset of a reduction set has the statistics of the whole set, and
close_bf16 (2^-7 relative + 2e-3 of the tensor's maximum) is hundreds of times wider than the
effect of a split, a chunk or a boundary pixel left out of the sums.  Here

  data   every reduction set (a LayerNorm row, a GroupNorm (instance, group)) has its own mean
         m in [-4, 4] and scale s in {1/4 .. 4}, every channel its own spread u in [0.5, 2], and a
         ramp runs over the reduced axis, so no subset has the statistics of the set:
             x = off + m + s * u * z + R * 2 * (t - 1/2),   t = p / pix  (GroupNorm), c / C (LayerNorm)
         with R = max(s, off / 8).  At off = 0 this is s * (u * z + 2 * (t - 1/2)); at off = 64 / 200
         (|mean| >> std: the shifted sums, the cancellation in b = beta - mean * a) the ramp grows with
         the offset, because the bound below grows with max|x| and a one-pixel omission has to stay
         as visible relative to it as it is at off = 0 (where |m| / s <= 16).  The "spike" variant
         replaces one element per set by 64 * s, at a position that cycles through the boundary
         classes (first / last pixel of the instance and of each split, first / last channel, the
         channels on either side of c0; for rows: first / last channel, 16-byte chunk and 64-lane
         boundaries), so a single boundary element missed or counted twice moves the statistics.
         Everything is rounded to bf16 and all references start from the rounded values.
  bound  |got - ref| <= half_ulp_bf16(ref) + tau * S      (assert_norm_close; a NaN fails)
         with ref in fp64 and S = max|x| * rstd * max|gamma| + max|beta| (+ max|pe|) of the element's
         reduction set: one bf16 rounding of the output plus tau for all the fp32 arithmetic before it.
         With SiLU: half_ulp_bf16(silu(ref)) + 1.1 * tau * S + 2^-18 * |silu(ref)|.
  tau    2^-20.  Not fitted to the kernels: it is the smallest power of two that is at least 8x the
         worst (|err| - half_ulp) / S of the fp32 restatements below (two-pass variance,
         a = rstd * gamma, b = beta - mean * a, fma(x, a, b)) over every case of GN_CASES, LN_CASES
         and RLM_C.  The restatement's sums are sequential in fp32 over runs of 128 elements (the
         longest run of inputs any of these kernels adds into one accumulator: vd_gn_small's 16
         pieces of 8) and a halving tree over the run sums (the kernels merge in trees and short
         chains; vd_gn_small's second level, up to 256 partial sums in sequence, is the longest
         chain and measures 1.5e-7 on the GPU); one sequential accumulator over a whole 40960-element set, which no kernel keeps,
         measures 1.2e-5 and would put tau above every single-pixel fault.
         Measured (tests/test_norm_bound_host.py asserts both at every case):
             restatement, worst case      1.04e-7   (3, 100, 640) off200    (tau / 8 = 1.19e-7)
             weakest planted fault        6.4e-6    one pixel of 4096 at (2, 4096, 320), spike variant
                                          1.2e-5    the same on the other variants (4 * tau = 3.81e-6)
             MI355X kernels, worst case   3.2e-7 outputs, 4.6e-7 {a, b} tables
  faults fp64 statistics of the wrong set applied to the whole tensor (gn_fault_stats,
         ln_fault_stats): what an off-by-one in a split bound, a lane run, an unrolled tail, a group
         merge or a shuffle width computes.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

BF16 = torch.bfloat16
TAU = 2.0 ** -20
VARIANTS = ("plain", "off64", "off200", "spike")
OFFSET = {"plain": 0.0, "off64": 64.0, "off200": 200.0, "spike": 0.0}
SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
SPIKE = 64.0
GN_EPS, LN_EPS, RLM_EPS = 1e-5, 1e-5, 1e-6
PE_DIV, PE_PERIOD = 3, 5


# ---------------------------------------------------------------- the mirrors of vdiff.ops' split rules
def gn_image_splits(pix):  # vdiff.ops.gn_image_splits (the GPU tests assert the mirror)
    return max(1, min(pix // 16, 32))


def gn_splits(n_inst, pix):  # vdiff.ops.gn_splits
    return max(1, min(pix // 16, math.ceil(2048 / n_inst), 256))


def gn_splits_per_frame(hw):  # vdiff.ops.gn_splits_per_frame
    return max(1, min(hw // 16, 16))


def split_bounds(pix, n_split):
    return [(pix * k // n_split, pix * (k + 1) // n_split) for k in range(n_split)]


# ---------------------------------------------------------------- cases (shared by both test files)
# GroupNorm: (n, pix, C, c0, G, n_split).  n_split is the route's own split count (it places the
# "last pixel of a split" fault and the spikes); 1 for vd_gn_small, which has no splits.
GN_SMALL = [(3, 100, 1280, 1280, 32, 1), (2, 64, 2560, 1280, 32, 1), (2, 256, 1280, 1280, 32, 1),
            (1, 7, 256, 256, 32, 1), (2, 4096, 256, 256, 32, 1)]
GN_SMALL_REJECTED = (1, 4097, 256, 256, 32)
_GN_SHAPES = [(2, 4096, 320, 320, 32), (3, 100, 640, 640, 32), (2, 1000, 128, 128, 32), (1, 7, 64, 32, 32),
              (2, 77, 2560, 1280, 32), (2, 33, 2048, 2048, 32), (2, 33, 1024, 1024, 32), (2, 257, 256, 256, 16),
              (2, 100, 320, 192, 32)]
GN_2PASS = [s + (gn_image_splits(s[1]),) for s in _GN_SHAPES]
GN_GREC = [s + (gn_splits(s[0], s[1]),) for s in _GN_SHAPES]
GN_VIDEO = (2, 4 * 256, 320, 320, 32, 4 * gn_splits_per_frame(256))  # B = 2, F * HW = 4 * 256
GN_CREC = [(2, 100, 384, 384, 24, gn_splits(2, 100)), (2, 4096, 320, 320, 32, 64), (1, 7, 64, 64, 32, 1)]
GN_CASES = sorted(set(GN_SMALL + GN_2PASS + GN_GREC + [GN_VIDEO] + GN_CREC))

# LayerNorm: (rows, C).  Rows kernels: RPW = 64 / LPR rows per wave, 4 waves per workgroup.
LN_ROWS = [(r, C) for C, rpw in ((320, 8), (640, 4), (1280, 2)) for r in (1, 4 * rpw * 2 + 1, 4 * rpw * 3 - 1)]
LN_ONE = [(65, C) for C in (8, 64, 512, 520, 1152, 2048)]
LN_CASES = LN_ROWS + LN_ONE
# vd_res_ln_mod: both sides of every CPL switch
RLM_ROWS, RLM_ROWS_PER_B = 70, 35
RLM_C = [128, 512, 520, 1024, 1032, 1536, 1544, 2048]
RLM_VARIANTS = ("plain", "off64", "off200")

GN_FAULTS = ("first_pixel", "last_pixel", "split_last_pixel", "last_channel", "next_group", "next_instance")
LN_FAULTS = ("first_chunk", "last_chunk", "rows_pooled")


def _gen(*key):
    h = 0
    for k in key:
        h = (h * 1000003 + (VARIANTS.index(k) if isinstance(k, str) else int(k))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def _affine(g, C):
    """gamma in [0.5, 1.5]; beta of either sign with |beta| in [0.25, 1].  beta stays away from 0 for the
    {a, b} table check: its bound on b is relative to |beta| + |mean * a|, while an fp32 mean carries an
    absolute error of the order of 2^-24 of the set's partial means, so a set with mean ~ 0 and a
    channel with beta ~ 0 would ask for more than fp32 holds (measured on the GPU with beta ~ N(0, 1/4):
    a set of mean -0.011 in data up to 21 and beta 0.003 had its mean right to 3.7e-8 and b off by
    1.6e-6 of that magnitude)."""
    sign = torch.randint(2, (C,), generator=g).float() * 2 - 1
    return torch.rand(C, generator=g) + 0.5, sign * (0.25 + 0.75 * torch.rand(C, generator=g))


# ---------------------------------------------------------------- data
def gn_spike_positions(n, pix, C, c0, G, n_split):
    """(pixel, channel within the group) of the spike of every (instance, group): the pixel cycles
    through the first / last pixel of the instance and of every split, the channel alternates
    between the group's first and last, and the groups that hold the channels on either side of
    the c0 concat boundary put it there (alternating by instance when one group holds both)."""
    cpg = C // G
    P = [0, pix - 1]
    for pb, pe in split_bounds(pix, n_split):
        P += [pb, pe - 1]
    pos = {}
    for i in range(n):
        for g in range(G):
            j = i * G + g
            pos[i, g] = (P[j % len(P)], (0, cpg - 1)[(j + j // len(P)) % 2])
    if c0 < C:
        ga, gb = (c0 - 1) // cpg, c0 // cpg
        for i in range(n):
            if ga != gb:
                pos[i, ga] = (pos[i, ga][0], (c0 - 1) % cpg)
                pos[i, gb] = (pos[i, gb][0], c0 % cpg)
            else:
                pos[i, ga] = (pos[i, ga][0], ((c0 - 1) % cpg, c0 % cpg)[i % 2])
    return pos


@functools.lru_cache(maxsize=None)
def gn_data(n, pix, C, c0, G, n_split, variant):
    """-> x [n * pix, C] bf16, gamma, beta (fp32, CPU).  Shared and cached: treat as read-only."""
    g = _gen(n, pix, C, c0, G, variant)
    cpg, off = C // G, OFFSET[variant]
    m = torch.rand(n, 1, G, 1, generator=g, dtype=torch.float64) * 8 - 4
    s = torch.tensor(SCALES, dtype=torch.float64)[torch.randint(len(SCALES), (n, 1, G, 1), generator=g)]
    u = torch.rand(1, 1, G, cpg, generator=g, dtype=torch.float64) * 1.5 + 0.5
    z = torch.randn(n, pix, G, cpg, generator=g, dtype=torch.float64)
    t = (torch.arange(pix, dtype=torch.float64) / pix - 0.5).view(1, pix, 1, 1)
    x = off + m + s * u * z + torch.clamp(s, min=off / 8) * 2 * t
    if variant == "spike":
        for (i, gg), (p, c) in gn_spike_positions(n, pix, C, c0, G, n_split).items():
            x[i, p, gg, c] = SPIKE * s[i, 0, gg, 0]
    gamma, beta = _affine(g, C)
    return x.reshape(n * pix, C).to(BF16), gamma, beta


def ln_spike_channels(C):
    """Boundary classes of a row: first / last channel, the ends of the first and last 16-byte
    chunk, and the chunk boundary where lane 63 hands over to lane 0's second chunk."""
    return sorted({0, C - 1, min(7, C - 1), min(8, C - 1), C - 8, min(511, C - 1), min(512, C - 1)})


@functools.lru_cache(maxsize=None)
def ln_data(rows, C, variant):
    """-> x [rows, C] bf16, gamma, beta, pe [PE_PERIOD, C] (fp32, CPU).  Read-only, cached."""
    g = _gen(rows, C, variant)
    off = OFFSET[variant]
    m = torch.rand(rows, 1, generator=g, dtype=torch.float64) * 8 - 4
    s = torch.tensor(SCALES, dtype=torch.float64)[torch.randint(len(SCALES), (rows, 1), generator=g)]
    u = torch.rand(1, C, generator=g, dtype=torch.float64) * 1.5 + 0.5
    z = torch.randn(rows, C, generator=g, dtype=torch.float64)
    t = (torch.arange(C, dtype=torch.float64) / C - 0.5).view(1, C)
    x = off + m + s * u * z + torch.clamp(s, min=off / 8) * 2 * t
    if variant == "spike":
        cs = ln_spike_channels(C)
        for r in range(rows):
            x[r, cs[r % len(cs)]] = SPIKE * s[r, 0]
    gamma, beta = _affine(g, C)
    pe = torch.randn(PE_PERIOD, C, generator=g)
    return x.to(BF16), gamma, beta, pe


@functools.lru_cache(maxsize=None)
def rlm_data(C, variant):
    """-> x (structured rows), y (plain) bf16 and the fp32 [B, 3 C + 4] table gate | shift | scale."""
    x = ln_data(RLM_ROWS, C, variant)[0]
    g = _gen(C, 7, variant)
    y = (0.5 * torch.randn(RLM_ROWS, C, generator=g)).to(BF16)
    mod = 0.5 * torch.randn(RLM_ROWS // RLM_ROWS_PER_B, 3 * C + 4, generator=g)
    return x, y, mod


# ---------------------------------------------------------------- fp64 references
def _gn4(x, n, pix, G):
    return x.double().view(n, pix, G, x.shape[1] // G)


def gn_stats(xd):
    return xd.mean((1, 3), keepdim=True), xd.var((1, 3), unbiased=False, keepdim=True)


def gn_ref(x, n, pix, G, eps, gamma, beta, stats=None):
    """fp64 GroupNorm of NHWC rows -> (ref, S), both [n * pix, C].  stats = (mean, var) [n,1,G,1]
    overrides the statistics the output is formed with (the planted faults); S is always the
    true set's."""
    xd = _gn4(x, n, pix, G)
    cpg = xd.shape[3]
    mean, var = gn_stats(xd)
    rstd = (var + eps).rsqrt()
    gam, bet = gamma.double().view(1, 1, G, cpg), beta.double().view(1, 1, G, cpg)
    S = xd.abs().amax((1, 3), keepdim=True) * rstd * gam.abs().amax(3, keepdim=True) + bet.abs().amax(3, keepdim=True)
    if stats is not None:
        mean, rstd = stats[0], (stats[1] + eps).rsqrt()
    ref = (xd - mean) * rstd * gam + bet
    return ref.reshape(n * pix, -1), S.expand_as(xd).reshape(n * pix, -1)


def gn_ab_ref(x, n, pix, G, eps, gamma, beta):
    """fp64 {a, b} tables [n, C] and the magnitude of b's two terms, |beta| + |mean * a|."""
    xd = _gn4(x, n, pix, G)
    mean, var = gn_stats(xd)
    a = ((var + eps).rsqrt()[:, 0] * gamma.double().view(1, G, -1))
    ma = mean[:, 0] * a
    b = beta.double().view(1, G, -1) - ma
    bmag = beta.double().abs().view(1, G, -1) + ma.abs()
    return a.reshape(n, -1), b.reshape(n, -1), bmag.reshape(n, -1)


def gn_fault_stats(x, n, pix, G, n_split, kind):
    """fp64 (mean, var) of the wrong set; None where the shape has no such set."""
    xd = _gn4(x, n, pix, G)
    if kind == "first_pixel":
        return gn_stats(xd[:, 1:]) if pix > 1 else None
    if kind == "last_pixel":
        return gn_stats(xd[:, :-1]) if pix > 1 else None
    if kind == "split_last_pixel":  # the last pixel of the middle split
        p = split_bounds(pix, n_split)[n_split // 2][1] - 1
        return gn_stats(torch.cat([xd[:, :p], xd[:, p + 1:]], 1)) if pix > 1 else None
    if kind == "last_channel":
        return gn_stats(xd[..., :-1]) if xd.shape[3] > 1 else None
    mean, var = gn_stats(xd)
    if kind == "next_group":
        return mean.roll(-1, 2), var.roll(-1, 2)
    if kind == "next_instance":
        return (mean.roll(-1, 0), var.roll(-1, 0)) if n > 1 else None
    raise ValueError(kind)


def ln_stats(xd):
    return xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)


def ln_ref(x, eps, gamma, beta, add=None, stats=None):
    """fp64 LayerNorm -> (ref, S).  gamma / beta: [C] or per-row [rows, C] (res_ln_mod's 1 + scale
    and shift); add: per-row addend after the affine (the positional embedding), counted in S."""
    xd = x.double()
    mean, var = ln_stats(xd)
    rstd = (var + eps).rsqrt()
    gam = gamma.double().expand_as(xd) if gamma.dim() == 2 else gamma.double().view(1, -1).expand_as(xd)
    bet = beta.double().expand_as(xd) if beta.dim() == 2 else beta.double().view(1, -1).expand_as(xd)
    S = xd.abs().amax(1, keepdim=True) * rstd * gam.abs().amax(1, keepdim=True) + bet.abs().amax(1, keepdim=True)
    if stats is not None:
        mean, rstd = stats[0], (stats[1] + eps).rsqrt()
    ref = (xd - mean) * rstd * gam + bet
    if add is not None:
        ref = ref + add.double()
        S = S + add.double().abs().amax(1, keepdim=True)
    return ref, S.expand_as(xd)


def ln_fault_stats(x, kind):
    xd = x.double()
    rows, C = xd.shape
    if kind == "first_chunk":
        return ln_stats(xd[:, 8:]) if C > 8 else None
    if kind == "last_chunk":
        return ln_stats(xd[:, :-8]) if C > 8 else None
    if kind == "rows_pooled":  # rows 2k and 2k + 1 share the statistics of both
        if rows < 2:
            return None
        ev = rows // 2 * 2
        mean, var = ln_stats(xd)
        pm, pv = ln_stats(xd[:ev].reshape(ev // 2, 2 * C))
        mean, var = mean.clone(), var.clone()
        mean[:ev], var[:ev] = pm.repeat_interleave(2, 0), pv.repeat_interleave(2, 0)
        return mean, var
    raise ValueError(kind)


def pe_rows(pe, rows):
    return pe[(torch.arange(rows) // PE_DIV) % PE_PERIOD]


def rlm_mods(mod, C, rows=RLM_ROWS, rows_per_b=RLM_ROWS_PER_B):
    """Per-row gate, shift, scale [rows, C] of the [B, 3 C + 4] table."""
    b = torch.arange(rows) // rows_per_b
    return mod[b, :C], mod[b, C:2 * C], mod[b, 2 * C:3 * C]


def rlm_residual(x, y, gate):
    """fp64 x + gate * y and the magnitude |x| + |gate * y| its bf16 store is held to."""
    gy = gate.double() * y.double()
    return x.double() + gy, x.double().abs() + gy.abs()


# ---------------------------------------------------------------- fp32 restatements
RUN = 128  # the longest run of inputs one accumulator of these kernels takes (vd_gn_small: 16 pieces of 8)


def _seq_sum(a, run=RUN):
    """fp32 sum of each row of a 2-D fp32 array in the kernels' shape: sequential fp32 sums over
    runs of `run` consecutive elements (np.add.accumulate does no pairwise grouping), then an fp32
    halving tree over the run sums (the LDS trees, wave butterflies and Chan merges).  run = None:
    one sequential sum over the whole row, which no kernel does (see the module docstring)."""
    rows, n = a.shape
    run = n if run is None else min(run, n)
    if n % run:
        a = np.concatenate([a, np.zeros((rows, run - n % run), np.float32)], 1)
    p = np.add.accumulate(a.reshape(rows, -1, run), axis=2, dtype=np.float32)[:, :, -1]
    w = 1 << (p.shape[1] - 1).bit_length()
    p = np.concatenate([p, np.zeros((rows, w - p.shape[1]), np.float32)], 1)
    while w > 1:
        w //= 2
        p = p[:, :w] + p[:, w:]
    return p[:, 0]


def _restate_sets(sets, eps, run=RUN):
    n = np.float32(sets.shape[1])
    mean = _seq_sum(sets, run) / n
    d = sets - mean[:, None]
    var = _seq_sum(d * d, run) / n
    return mean, np.float32(1) / np.sqrt(var + np.float32(eps), dtype=np.float32)


def _fma(x, a, b):
    """fmaf(x, a, b): the product of a bf16 value and an fp32 is exact in fp64, so one rounding."""
    return (x.astype(np.float64) * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)


def gn_restate32(x, n, pix, G, eps, gamma, beta, run=RUN):
    """The kernels' formulas in sequential fp32 on the CPU -> fp32 output before its bf16 rounding."""
    C = x.shape[1]
    cpg = C // G
    sets = np.ascontiguousarray(x.float().view(n, pix, G, cpg).permute(0, 2, 1, 3).reshape(n * G, pix * cpg).numpy())
    mean, rstd = _restate_sets(sets, eps, run)
    a = np.repeat(rstd.reshape(n, G), cpg, 1) * gamma.numpy()[None]       # [n, C]
    b = beta.numpy()[None] - np.repeat(mean.reshape(n, G), cpg, 1) * a
    y = _fma(x.float().view(n, pix, C).numpy(), a[:, None].astype(np.float32), b[:, None].astype(np.float32))
    return torch.from_numpy(y).reshape(n * pix, C)


def ln_restate32(x, eps, gamma, beta, add=None):
    xs = np.ascontiguousarray(x.float().numpy())
    mean, rstd = _restate_sets(xs, eps)
    gam = gamma.numpy() if gamma.dim() == 2 else gamma.numpy()[None]
    bet = beta.numpy() if beta.dim() == 2 else beta.numpy()[None]
    a = (rstd[:, None] * gam).astype(np.float32)
    b = (bet - mean[:, None] * a).astype(np.float32)
    y = _fma(xs, a, b)
    if add is not None:
        y = y + add.numpy()
    return torch.from_numpy(y.astype(np.float32))


# ---------------------------------------------------------------- the bound
def half_ulp_bf16(r):
    """2^(floor(log2|r|) - 8): half the spacing of bf16 at r (0 at r = 0)."""
    r = r.double()
    _, e = torch.frexp(r)  # |r| = f * 2^e, f in [0.5, 1)
    return torch.where(r == 0, torch.zeros_like(r), torch.ldexp(torch.ones_like(r), e - 9))


def silu64(r):
    return r * torch.sigmoid(r)


def norm_excess(got, ref, S, silu=False):
    """Per element, the tau the bound would need: (|got - ref| - half_ulp) / S (see the docstring)."""
    got, ref, S = got.double().cpu(), ref.double().cpu(), S.double().cpu()
    if silu:
        ref = silu64(ref)
        return ((got - ref).abs() - half_ulp_bf16(ref) - 2.0 ** -18 * ref.abs()) / (1.1 * S)
    return ((got - ref).abs() - half_ulp_bf16(ref)) / S


def assert_norm_close(got, ref, S, tau=TAU, silu=False, what=""):
    assert got.dtype == BF16 and got.shape == ref.shape
    ex = norm_excess(got, ref, S, silu)
    bad = ~(ex <= tau)  # a NaN is out of bounds
    if bad.any():
        i = int(torch.where(bad.flatten(), ex.flatten().nan_to_num(float("inf")), -1.0).argmax())
        r, c = divmod(i, ref.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} / {ref.numel()} elements outside half-ulp + tau * S; worst at "
                             f"[{r}, {c}]: got {float(got[r, c]):.6g}, ref {float(ref.flatten()[i]):.6g}"
                             f"{' (before SiLU)' if silu else ''}, S {float(S.flatten()[i]):.4g}, needs tau "
                             f"{float(ex.flatten()[i]):.3e} > {tau:.3e}")


def assert_ab_close(ss, a64, b64, bmag, tau=TAU, what=""):
    """The fp32 {a, b} table [n, C, 2] against fp64: |a - a64| <= tau |a64|, |b - b64| <= tau (|beta| + |mean a64|)."""
    a, b = ss[..., 0].double().cpu(), ss[..., 1].double().cpu()
    ea, eb = ((a - a64).abs() / a64.abs()).max().item(), ((b - b64).abs() / bmag).max().item()
    assert ea <= tau and eb <= tau, f"{what}: a off by {ea:.3e}, b off by {eb:.3e} (relative), tau {tau:.3e}"
