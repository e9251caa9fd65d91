"""The norm bound has teeth (CPU; the GPU side is tests/test_gpu_norm_stats.py).

For every shape and data variant the GPU tests use (tests/norm_ref.py):
  * the fp32 restatement of the kernels' formulas stays within tau / 8 of the fp64 reference, so an
    honest fp32 kernel has 8x of room, and
  * every planted fault (fp64 statistics of the wrong set: a boundary pixel, a channel, a chunk left
    out, a neighbour's statistics, two rows pooled) needs more than 4 * tau, so none can pass.
The same faults pass close_bf16, the tolerance the older norm tests use.
"""
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from memframe import close_bf16

TAU = R.TAU


def _excess(y, ref, S, silu=False):
    return R.norm_excess(y.to(R.BF16), ref, S, silu=silu).max().item()


def test_tau_and_half_ulp():
    assert TAU == 2.0 ** -20
    r = torch.tensor([1.0, 1.5, 1.9999, 2.0, -3.0, 0.75, 0.0, 2.0 ** -10])
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -9, 0.0, 2.0 ** -18])
    assert torch.equal(R.half_ulp_bf16(r), want.double())
    # half an ulp is exactly what round-to-nearest costs: the rounded reference passes at tau = 0
    x = torch.randn(4096, dtype=torch.float64).view(64, 64) * 3
    R.assert_norm_close(x.to(R.BF16), x, torch.ones_like(x), tau=0.0)
    nan = x.to(R.BF16).clone()
    nan[3, 5] = float("nan")
    with pytest.raises(AssertionError):
        R.assert_norm_close(nan, x, torch.ones_like(x))


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_group_norm_restatement_and_faults(case, variant):
    n, pix, C, c0, G, n_split = case
    x, gamma, beta = R.gn_data(*case, variant)
    ref, S = R.gn_ref(x, n, pix, G, R.GN_EPS, gamma, beta)
    y = R.gn_restate32(x, n, pix, G, R.GN_EPS, gamma, beta)
    e, es = _excess(y, ref, S), _excess(F.silu(y), ref, S, silu=True)
    print(f"restatement {e:.3e}, with SiLU {es:.3e}")
    assert max(e, es) <= TAU / 8
    for kind in R.GN_FAULTS:
        st = R.gn_fault_stats(x, n, pix, G, n_split, kind)
        if st is None:  # the shape has no such set (one instance, one pixel, one channel per group)
            continue
        bad, _ = R.gn_ref(x, n, pix, G, R.GN_EPS, gamma, beta, stats=st)
        f, fs = _excess(bad, ref, S), _excess(R.silu64(bad), ref, S, silu=True)
        print(f"{kind} {f:.3e}, with SiLU {fs:.3e}")
        assert min(f, fs) > 4 * TAU, kind
        with pytest.raises(AssertionError):
            R.assert_norm_close(bad.to(R.BF16), ref, S)


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("case", R.LN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_layer_norm_restatement_and_faults(case, variant):
    rows, C = case
    x, gamma, beta, pe = R.ln_data(rows, C, variant)
    for add in (None, R.pe_rows(pe, rows)):
        ref, S = R.ln_ref(x, R.LN_EPS, gamma, beta, add=add)
        e = _excess(R.ln_restate32(x, R.LN_EPS, gamma, beta, add=add), ref, S)
        print(f"pe {add is not None}: restatement {e:.3e}")
        assert e <= TAU / 8
        for kind in R.LN_FAULTS:
            st = R.ln_fault_stats(x, kind)
            if st is None:  # one row, or one chunk per row
                continue
            f = _excess(R.ln_ref(x, R.LN_EPS, gamma, beta, add=add, stats=st)[0], ref, S)
            print(f"{kind} {f:.3e}")
            assert f > 4 * TAU, kind


@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("variant", R.RLM_VARIANTS)
@pytest.mark.parametrize("C", R.RLM_C)
def test_res_ln_mod_restatement_and_faults(C, variant, with_y):
    x, y, mod = R.rlm_data(C, variant)
    gate, shift, scale = R.rlm_mods(mod, C)
    xn = R.rlm_residual(x, y, gate)[0].to(R.BF16) if with_y else x  # the stored residual is normalised
    ref, S = R.ln_ref(xn, R.RLM_EPS, 1 + scale, shift)
    e = _excess(R.ln_restate32(xn, R.RLM_EPS, 1 + scale, shift), ref, S)
    print(f"restatement {e:.3e}")
    assert e <= TAU / 8
    for kind in R.LN_FAULTS:
        f = _excess(R.ln_ref(xn, R.RLM_EPS, 1 + scale, shift, stats=R.ln_fault_stats(xn, kind))[0], ref, S)
        print(f"{kind} {f:.3e}")
        assert f > 4 * TAU, kind


def _gn_without_one(x, n, pix, G, pos):
    """fp64 (mean, var) of every (instance, group) with its element pos[i, g] = (pixel, channel) left out."""
    xd = R._gn4(x, n, pix, G)
    N = pix * xd.shape[3]
    e = torch.tensor([[xd[i, pos[i, g][0], g, pos[i, g][1]] for g in range(G)] for i in range(n)]).view(n, 1, G, 1)
    mean = (xd.sum((1, 3), keepdim=True) - e) / (N - 1)
    var = (((xd - mean) ** 2).sum((1, 3), keepdim=True) - (e - mean) ** 2) / (N - 1)
    return mean, var


def test_spike_makes_one_element_visible():
    """One boundary element of 40960 left out of a set's sums: on plain data at pix = 4096 the bound
    sees it in some sets only (where the set's own mean is small) and lets it pass in others; with
    the spike variant, whose spike sits on that element, it is far outside in every set at once."""
    case = (2, 4096, 320, 320, 32, 32)
    n, pix, C, c0, G, n_split = case
    pos = R.gn_spike_positions(*case)
    assert {p for p, _ in pos.values()} >= {0, pix - 1, pix // n_split, pix // n_split - 1}
    assert {c for _, c in pos.values()} == {0, C // G - 1}
    worst = {}
    for variant in ("plain", "spike"):
        x, gamma, beta = R.gn_data(*case, variant)
        ref, S = R.gn_ref(x, n, pix, G, R.GN_EPS, gamma, beta)
        bad, _ = R.gn_ref(x, n, pix, G, R.GN_EPS, gamma, beta, stats=_gn_without_one(x, n, pix, G, pos))
        ex = R.norm_excess(bad.to(R.BF16), ref, S).view(n, pix, G, -1).amax((1, 3))  # per set
        worst[variant] = ex
        print(variant, f"per-set excess {ex.min().item():.3e} .. {ex.max().item():.3e}")
    assert worst["plain"].min().item() <= TAU            # undetected in some sets
    assert (worst["plain"] <= 4 * TAU).sum().item() >= n * G // 4
    assert worst["spike"].min().item() > 4 * TAU         # detected in every set


def test_ln_spike_positions_cover_the_lane_and_chunk_boundaries():
    assert R.ln_spike_channels(2048) == [0, 7, 8, 511, 512, 2040, 2047]
    assert R.ln_spike_channels(8) == [0, 7]
    x = R.ln_data(65, 520, "spike")[0].double()
    hit = {int(r.abs().argmax()) for r in x}
    assert hit == set(R.ln_spike_channels(520))


def test_quarter_of_the_pixels_left_out_passes_close_bf16():
    """The gap this bound closes: GroupNorm statistics over three quarters of the pixels, on the
    i.i.d. data of the older tests at (2, 4096, 320), pass close_bf16 and fail the half-ulp bound."""
    n, pix, C, G = 2, 4096, 320, 32
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(n * pix, C, generator=g) * 3 + 1.5).to(R.BF16)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    ref, S = R.gn_ref(x, n, pix, G, 1e-6, gamma, beta)
    bad, _ = R.gn_ref(x, n, pix, G, 1e-6, gamma, beta, stats=R.gn_stats(R._gn4(x, n, pix, G)[:, :pix * 3 // 4]))
    close_bf16(bad.to(R.BF16), ref)
    R.assert_norm_close(ref.to(R.BF16), ref, S)
    with pytest.raises(AssertionError):
        R.assert_norm_close(bad.to(R.BF16), ref, S)
    # and on the structured data even a whole split (1 / 32 of the pixels) is far outside
    case = (2, 4096, 320, 320, 32, 32)
    xs, gamma, beta = R.gn_data(*case, "plain")
    ref, S = R.gn_ref(xs, n, pix, G, R.GN_EPS, gamma, beta)
    st = R.gn_stats(R._gn4(xs, n, pix, G)[:, :pix * 31 // 32])
    assert _excess(R.gn_ref(xs, n, pix, G, R.GN_EPS, gamma, beta, stats=st)[0], ref, S) > 100 * TAU


def test_full_length_sequential_sums_are_not_the_kernels():
    """Why the restatement sums in runs: one sequential fp32 accumulator over a 40960-element set
    (which no kernel keeps) is two orders of magnitude less accurate than the run / tree shape."""
    case = (2, 4096, 320, 320, 32, 32)
    n, pix, C, c0, G, _ = case
    x, gamma, beta = R.gn_data(*case, "plain")
    ref, S = R.gn_ref(x, n, pix, G, R.GN_EPS, gamma, beta)
    e = _excess(R.gn_restate32(x, n, pix, G, R.GN_EPS, gamma, beta, run=None), ref, S)
    print(f"full-length sequential {e:.3e}")
    assert e > TAU
