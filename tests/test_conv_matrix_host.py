"""The conv loaders' case matrix, everything that needs no GPU (tests/conv_ref.py): the explicit
gather restatement is the reference's operation, every loader fault planted in it lands far outside
the tolerance the GPU test applies to the same case, every fault has a carrier in every family that
could commit it, every case's plan (kernel, N tile, K split, workspace) is pinned through
vd_gemm_plan, and the table is the full family x mode product — a thinned one cannot pass."""
import functools

import pytest
import torch

import conv_ref as R

NAMES = [c.name for c in R.CASES]
FAULT_MARGIN = 100.0  # a planted fault must exceed rtol |ref| + FAULT_MARGIN x atol somewhere


@functools.lru_cache(maxsize=None)
def ref_of(name):
    case = R.BY_NAME[name]
    op = R.operands(case)
    return case, op, R.reference(case, op)


@functools.lru_cache(maxsize=None)
def fault_margins(name):
    """{fault: (max over elements of (|faulted - ref| - rtol |ref|) / atol, rows wrong, max error)}"""
    case, op, ref = ref_of(name)
    rtol, atol = R.tolerance(case, ref)
    out = {}
    for fault in R.faults_of(case):
        err = (R.restated(case, op, fault) - ref).abs()
        over = (err - rtol * ref.abs()) / atol
        out[fault] = (over.max().item(), int((over > 1).any(1).sum()), err.max().item())
    return out


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference(name):
    case, op, ref = ref_of(name)
    assert tuple(ref.shape) == (case.M, case.cout) and ref.dtype == torch.float64
    got = R.restated(case, op)
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


@pytest.mark.parametrize("name", NAMES)
def test_every_applicable_fault_is_far_outside_the_tolerance(name):
    case = R.BY_NAME[name]
    margins = fault_margins(name)
    assert list(margins) == R.faults_of(case) and "hw_swap" in margins
    for fault, (over, rows, top) in margins.items():
        print(f"{name} {fault}: max error {top:.3f}, {rows} of {case.M} rows out, {over:.0f} x atol past the bound")
        assert over >= FAULT_MARGIN, (name, fault, over)


def test_weakest_fault_margin():
    worst = min((over, name, fault) for name in NAMES for fault, (over, _, _) in fault_margins(name).items())
    fewest = min((rows / R.BY_NAME[name].M, name, fault) for name in NAMES
                 for fault, (_, rows, _) in fault_margins(name).items())
    print(f"weakest planted fault: {worst[2]} on {worst[1]}, {worst[0]:.0f} x the absolute term past the bound; "
          f"fewest rows wrong: {fewest[2]} on {fewest[1]}, {100 * fewest[0]:.1f} % of the rows")
    assert worst[0] >= FAULT_MARGIN


# which families can commit which fault: every loader decodes rows, walks spatial taps, strides and
# feeds an epilogue that indexes the row bias; the 32-column v2 tile runs neither upsample nor
# concat (conv_out and its like); temporal taps exist on v1 and v2 only
ALL_2D = set(R.FAMILIES_2D)
CAN_COMMIT = {
    "hw_swap": ALL_2D | set(R.FAMILIES_3D), "row_wrap": ALL_2D | set(R.FAMILIES_3D),
    "seam": ALL_2D | set(R.FAMILIES_3D), "tap_transposed": ALL_2D | set(R.FAMILIES_3D),
    "s2_centre": ALL_2D | set(R.FAMILIES_3D), "rb_div_in": ALL_2D | set(R.FAMILIES_3D),
    "up_ceil": ALL_2D - {"v2-bn32"}, "concat_half": ALL_2D - {"v2-bn32"}, "concat_swapped": ALL_2D - {"v2-bn32"},
    "t_wrap": set(R.FAMILIES_3D), "t_reversed": set(R.FAMILIES_3D), "t_off_ignored": set(R.FAMILIES_3D),
}


def test_every_fault_has_a_carrier_in_every_family_that_can_commit_it():
    assert set(CAN_COMMIT) == set(R.FAULTS)
    for fault, families in CAN_COMMIT.items():
        for fam in families:
            carriers = [c.name for c in R.CASES if c.family == fam and fault in R.faults_of(c)]
            assert carriers, f"no case of family {fam} can see the fault {fault}"
    # the geometry that makes them visible
    for c in R.CASES:
        assert c.h_out != c.w_out and c.h != c.w, c.name          # hw_swap, tap_transposed
        assert not c.c1 or (c.c0 != c.c1 and c.c0 > c.c1), c.name  # concat_half, concat_swapped


# ---------------------------------------------------------------- plans
# family -> (kernel, N tile, split class)
FAMILY_PLAN = {"v1": (1, 128, False), "v6": (6, 64, False), "v6-split": (6, 64, True), "v2-bn128": (2, 128, False),
               "v2-bn160": (2, 160, False), "v2-bn32": (2, 32, False), "v2-split": (2, 128, True),
               "v5": (5, 320, False), "v5-split": (5, 320, True), "v2-unsplit": (2, 160, False)}


@pytest.mark.parametrize("name", NAMES)
def test_plan_is_pinned(name):
    """vd_gemm_plan / vd_gemm_ws_bytes without a device (256 CUs), under the case's path and
    plan_m: the family the case is for, its N tile by the plan's rule, the K split and the
    workspace the table records."""
    c = R.BY_NAME[name]
    assert (c.kernel, c.bn, c.is_split) == FAMILY_PLAN[c.family], "the table's expectation is not its family's"
    assert R.ntile(c) == c.bn
    kernel, split, ws = R.planned(c)
    assert (kernel, split) == (c.kernel, c.split), f"the plan gives v{kernel} split {split}: choose another shape"
    assert ws == R.ws_bytes(c) and (ws > 0) == c.is_split
    if c.mul > 1:  # the smallest multiple that reaches the plan: one less plans something else
        from dataclasses import replace
        less = R.planned(replace(c, mul=c.mul - 1))
        assert less[:2] != (c.kernel, c.split), (name, less)


# ---------------------------------------------------------------- coverage
ROW_TILE = {1: 128, 2: 256, 5: 256, 6: 64}


def test_table_is_the_full_product():
    two = [c for c in R.CASES if not c.is3d]
    three = [c for c in R.CASES if c.is3d]
    assert {(c.family, c.mode) for c in two} == R.product_2d()
    assert {(c.family, c.mode) for c in three} == R.product_3d()
    assert len(R.product_2d()) == 9 * 4 - 2 + 2 + 5 and len(R.product_3d()) == 12
    # every family's s1 runs with a bf16 output too, and nothing else does
    assert {c.family for c in two if not c.out_f32} == set(R.FAMILIES_2D)
    assert all(c.mode == "s1" for c in R.CASES if not c.out_f32)
    # v1's K % 32 != 0 tile, the long tap walk, the unequal concat halves
    assert {c.mode for c in two if c.family == "v1" and c.cin == 8} == {"s1", "s2"}
    assert all(c.cin == 192 and c.c1 == 0 and not c.is_split for c in two if c.mode == "long")
    assert all((c.c0, c.c1) == ((96, 32) if c.kernel == 5 else (128, 64)) for c in two if c.mode == "concat")
    assert all(c.c0 % 64 != 0 for c in two if c.kernel == 5)
    # the epilogue extras
    for c in two:
        want = {"s1": (True, True, False), "concat": (True, True, False), "long": (True, True, False),
                "wide": (True, True, False), "s2": (True, True, True), "up": (True, False, False)}[c.mode]
        assert (c.bias, c.rowbias, c.res) == want, c.name
    assert len(R.CASES) == len(two) + len(three) == 43 + 9 + 12


def test_geometry_cannot_hide_the_arithmetic():
    for c in R.CASES:
        assert c.M <= R.MAX_ROWS and (c.cin <= R.MAX_CIN or c.name in R.OVER_CIN), c.name
        tile = ROW_TILE[c.kernel]
        px = c.h_out * c.w_out
        # no power of two anywhere a Div could shift, rows off the tile, a ragged last tile
        for v in (c.h_out, c.w_out, px) + ((c.frames,) if c.is3d else ()):
            assert v & (v - 1), (c.name, v)
        assert c.M > tile and (c.M % tile or c.mode == "wide"), c.name
        if c.mode == "wide":  # one image row spans v6's 64-row tile; its ends fall inside tiles
            assert c.w_out > 64 and c.w_out % 64 and c.n_out >= 2
        else:  # several images, and no seam on a tile boundary but the first
            assert c.n_out >= 2 and px % tile and tile % px, c.name
        if c.is3d:
            assert c.n >= 2 and c.frames >= 3 and c.frames_in == c.frames + (2 if c.halo else 0)
    assert [c.name for c in R.CASES if c.cin > R.MAX_CIN] == list(R.OVER_CIN)
    # the families' minimum row counts: v2 / v5 from 256 rows, the unsplit v6 below them where the plan is its own
    assert all(c.M >= 256 for c in R.CASES if c.kernel in (2, 5))
    assert all(c.M < 256 for c in R.CASES if c.family == "v6" and c.path == 0)
