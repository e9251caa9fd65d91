"""Every statistics route of csrc/norm.hip and csrc/dit.hip against fp64, to half a bf16 ulp of the
output plus tau = 2^-20 of the reduction set's largest intermediate (tests/norm_ref.py), on data
where no subset of a reduction set has the statistics of the set.  tests/test_norm_bound_host.py
shows on the CPU that at these very shapes a boundary pixel, a channel or a 16-byte chunk left out
of the sums, or a neighbour's statistics, is at least 4 * tau away, and honest fp32 within tau / 8.

GroupNorm   vd_gn_small | vd_gn_partial_g -> vd_gn_apply_g | vd_gn_partial_g -> vd_gn_finalize_g
            (_ranks) -> vd_gn_apply | vd_gn_partial -> vd_gn_finalize -> vd_gn_apply
LayerNorm   layernorm_rows_kernel<8|16|32, 5> | layernorm_kernel
adaLN       vd_res_ln_mod, both sides of every CPL switch
"""
import functools

import pytest
import torch

import norm_ref as R
from vdiff import ops

pytestmark = pytest.mark.gpu

_id = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c)  # noqa: E731


@functools.lru_cache(maxsize=4)  # shared where two routes have the same case; ~40 MB each at the largest
def _gn_reference(case, variant):
    n, pix, C, c0, G, n_split = case
    x, gamma, beta = R.gn_data(*case, variant)
    return R.gn_ref(x, n, pix, G, R.GN_EPS, gamma, beta)


def _gn_inputs(cuda, case, variant):
    n, pix, C, c0, G, n_split = case
    x, gamma, beta = R.gn_data(*case, variant)
    x0 = x[:, :c0].contiguous().to(cuda)
    x1 = x[:, c0:].contiguous().to(cuda) if c0 < C else None
    return x0, x1, gamma.to(cuda), beta.to(cuda)


def _check_gn(run, case, variant, what):
    ref, S = _gn_reference(case, variant)
    for silu in (False, True):
        R.assert_norm_close(run(silu).cpu(), ref, S, silu=silu, what=f"{what} {case} {variant} silu={silu}")


def test_split_rules_are_mirrored():
    """norm_ref places the split-boundary faults and spikes by these rules."""
    for pix in (1, 7, 33, 77, 100, 256, 257, 1000, 1024, 4096):
        assert R.gn_image_splits(pix) == ops.gn_image_splits(pix)
        assert R.gn_splits_per_frame(pix) == ops.gn_splits_per_frame(pix)
        for n in (1, 2, 3):
            assert R.gn_splits(n, pix) == ops.gn_splits(n, pix)


# ---------------------------------------------------------------- GroupNorm
@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("case", R.GN_SMALL, ids=_id)
def test_gn_small(cuda, case, variant):
    n, pix, C, c0, G, _ = case
    assert ops.gn_small_chunk(pix, C, G) != 0
    x0, x1, g, b = _gn_inputs(cuda, case, variant)
    _check_gn(lambda silu: ops.gn_small(x0, n, pix, G, R.GN_EPS, g, b, silu=silu, x1=x1), case, variant, "gn_small")


def test_gn_small_rejects_more_rows_than_its_registers_hold():
    n, pix, C, c0, G = R.GN_SMALL_REJECTED
    assert ops.gn_small_chunk(pix, C, G) == 0
    assert ops.gn_small_chunk(pix - 1, C, G) == C // G  # the largest pix: one group per workgroup


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("case", R.GN_2PASS, ids=_id)
def test_gn_two_launch(cuda, case, variant):
    n, pix, C, c0, G, n_split = case
    assert n_split == ops.gn_image_splits(pix)
    x0, x1, g, b = _gn_inputs(cuda, case, variant)
    _check_gn(lambda silu: ops.group_norm_2pass(x0, n, pix, G, R.GN_EPS, g, b, silu=silu, x1=x1), case, variant,
              "partial_g/apply_g")


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("case", R.GN_GREC + [R.GN_VIDEO], ids=_id)
def test_gn_group_records(cuda, case, variant):
    n, pix, C, c0, G, n_split = case
    x0, x1, g, b = _gn_inputs(cuda, case, variant)
    if case == R.GN_VIDEO:  # B = 2 videos of F = 4 frames of HW = 256 pixels
        assert n_split == 4 * ops.gn_splits_per_frame(256)
    else:
        assert n_split == ops.gn_splits(n, pix)
    _check_gn(lambda silu: ops.group_norm(x0, n, pix, G, R.GN_EPS, g, b, silu=silu, x1=x1, two_pass=False,
                                          n_split=n_split), case, variant, "partial_g/finalize_g/apply")


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("case", R.GN_CREC, ids=_id)
def test_gn_channel_records(cuda, case, variant):
    n, pix, C, c0, G, n_split = case
    x0, x1, g, b = _gn_inputs(cuda, case, variant)
    ss = ops.gn_finalize(ops.gn_partial(x0, C, n, pix, n_split), G, R.GN_EPS, g, b)
    _check_gn(lambda silu: ops.gn_apply(x0, ss, pix, silu), case, variant, "partial/finalize/apply")
    if 256 % G:  # group_norm itself comes this way when the group count does not divide a workgroup
        assert n_split == ops.gn_splits(n, pix)
        assert torch.equal(ops.group_norm(x0, n, pix, G, R.GN_EPS, g, b, two_pass=False), ops.gn_apply(x0, ss, pix, False))


@pytest.mark.parametrize("variant", ["plain", "off64", "off200"])
@pytest.mark.parametrize("case", [R.GN_CREC[0], R.GN_CREC[1], R.GN_GREC[0], R.GN_GREC[2], R.GN_GREC[7], R.GN_VIDEO], ids=_id)
def test_gn_scale_shift_tables(cuda, case, variant):
    """The fp32 {a, b} tables themselves: |a - a64| <= tau |a64|, |b - b64| <= tau (|beta| + |mean a64|),
    from vd_gn_finalize, vd_gn_finalize_g and, with the records made in two pixel halves stacked
    rank-major, vd_gn_finalize_g_ranks."""
    n, pix, C, c0, G, n_split = case
    x, gamma, beta = R.gn_data(*case, variant)
    want = R.gn_ab_ref(x, n, pix, G, R.GN_EPS, gamma, beta)
    x0, _, g, b = _gn_inputs(cuda, case, variant)
    tables = {"finalize": ops.gn_finalize(ops.gn_partial(x0, C, n, pix, n_split), G, R.GN_EPS, g, b)}
    if 256 % G == 0:
        tables["finalize_g"] = ops.gn_finalize_g(ops.gn_partial_g(x0, C, n, pix, n_split, G), C, R.GN_EPS, g, b)
        if pix % 2 == 0 and n_split % 2 == 0:
            halves = [x0.view(n, 2, pix // 2, C)[:, r].reshape(-1, C).contiguous() for r in range(2)]
            parts = [ops.gn_partial_g(h, C, n, pix // 2, n_split // 2, G) for h in halves]
            tables["finalize_g_ranks"] = ops.gn_finalize_g(torch.stack(parts, 0), C, R.GN_EPS, g, b)
    for name, ss in tables.items():
        R.assert_ab_close(ss, *want, what=f"{name} {case} {variant}")


# ---------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("case", R.LN_CASES, ids=_id)
def test_layer_norm(cuda, case, variant):
    rows, C = case
    x, gamma, beta, pe = R.ln_data(rows, C, variant)
    xc, g, b, pec = x.to(cuda), gamma.to(cuda), beta.to(cuda), pe.to(cuda)
    ref, S = R.ln_ref(x, R.LN_EPS, gamma, beta)
    R.assert_norm_close(ops.layer_norm(xc, g, b, eps=R.LN_EPS).cpu(), ref, S, what=f"layer_norm {case} {variant}")
    ref, S = R.ln_ref(x, R.LN_EPS, gamma, beta, add=R.pe_rows(pe, rows))
    got = ops.layer_norm(xc, g, b, eps=R.LN_EPS, pe=pec, pe_div=R.PE_DIV, pe_period=R.PE_PERIOD)
    R.assert_norm_close(got.cpu(), ref, S, what=f"layer_norm + pe {case} {variant}")


# ---------------------------------------------------------------- adaLN
@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("variant", R.RLM_VARIANTS)
@pytest.mark.parametrize("C", R.RLM_C)
def test_res_ln_mod(cuda, C, variant, with_y):
    x, y, mod = R.rlm_data(C, variant)
    gate, shift, scale = R.rlm_mods(mod, C)
    xc, modc = x.to(cuda).clone(), mod.to(cuda)
    h = ops.res_ln_mod(xc, y=y.to(cuda) if with_y else None, gate=modc[:, :C] if with_y else None,
                       shift=modc[:, C:2 * C], scale=modc[:, 2 * C:3 * C], rows_per_b=R.RLM_ROWS_PER_B,
                       x_out=xc if with_y else None, eps=R.RLM_EPS)
    xn = xc.cpu()
    if with_y:  # the stored residual: one bf16 rounding of x + gate * y formed in fp32
        want, mag = R.rlm_residual(x, y, gate)
        err = (xn.double() - want).abs()
        assert bool((err <= R.half_ulp_bf16(want) + 2.0 ** -22 * mag).all()), \
            f"x_out: worst {(err - R.half_ulp_bf16(want) - 2.0 ** -22 * mag).max().item():.3e} outside"
    else:
        assert torch.equal(xn, x)
    ref, S = R.ln_ref(xn, R.RLM_EPS, 1 + scale, shift)  # the kernel normalises its own x_out
    R.assert_norm_close(h.cpu(), ref, S, what=f"res_ln_mod C={C} {variant} with_y={with_y}")
