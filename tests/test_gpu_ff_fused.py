"""vd_ff_fused (csrc/ff.hip): the 64 x 64 level's FeedForward — GEGLU projection (+ folded
LayerNorm), ff2, bias and residual — in one launch, against the two launches it replaces.

K = 320, hidden = 1280, N = 320 are fixed by the kernel; M is chosen for its seams: 16 (one row
block), 300 (ragged, fewer row blocks than waves), 4136 (every workgroup of the grid busy for one
pass, the weight ring wrapping 20 times, the 8-way XCD row split, a ragged tail) and multi_pass_m()
(one pass of the grid is 128 rows per CU, so 2 x 128 x CUs + 4461 rows — 69997 on 256 CUs — give
every workgroup two passes and some a third whose last waves are out of range: the code that runs
only between passes — the next pass's weights prefetched under the last chunk, x reloaded in
place, the output staged in the ring stage the next pass's second chunk lands in).
The reference is the existing path on the same tensors — ops.gemm(act=ACT_GEGLU) / LnFold.gemm, then ops.gemm(res=) — planned as the
131072-row step plans it (ops.plan_scaled: the weight-stationary v8 GEGLU and the unsplit v2 ff2),
since at these small M the automatic plan would pick other kernels or refuse the fold.
Inputs: seeded N(0, 1) activations, N(0, 0.02²) weights; every M uses the first M rows of one
4136-row set, so row independence (test 2) compares like with like.
"""
from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F

from vdiff import ops
from vdiff._lib import GemmDesc, VdiffError, lib
from vdiff.models.layers import LnFold, pack_geglu

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
C, HID = 320, 1280
MS = (16, 300, 4136)
MBIG = MS[-1]
PLAN_ROWS = 131072  # the step's row count at this level: the plan the reference is made for


def multi_pass_m():
    """Rows that take the grid (one workgroup of 8 waves x 16 rows per CU) through 2-3 passes."""
    return 2 * 128 * torch.cuda.get_device_properties(0).multi_processor_count + 4461


@functools.lru_cache(maxsize=None)
def data():
    """One seeded input set for every test (built once, never modified)."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1234)
    d = {}
    d["x"] = torch.randn(MBIG, C, device=dev, generator=g).to(BF)
    d["res"] = torch.randn(MBIG, C, device=dev, generator=g).to(BF)
    w1 = 0.02 * torch.randn(2 * HID, C, device=dev, generator=g)
    b1 = 0.02 * torch.randn(2 * HID, device=dev, generator=g)
    d["w2f"] = 0.02 * torch.randn(C, HID, device=dev, generator=g)
    d["w2"] = d["w2f"].to(BF).contiguous()
    d["b2"] = (0.02 * torch.randn(C, device=dev, generator=g)).float().contiguous()
    norm = torch.nn.LayerNorm(C).to(dev)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(C, device=dev, generator=g))
        norm.bias.copy_(0.1 * torch.randn(C, device=dev, generator=g))
    d["norm"], d["w1f"], d["b1f"] = norm, w1, b1
    d["w1"] = pack_geglu(w1.to(BF))
    d["b1"] = pack_geglu(b1.float())
    d["fold"] = LnFold(norm, w1, b1, pack=pack_geglu)        # with b1
    d["fold_nob"] = LnFold(norm, w1, None, pack=pack_geglu)   # b' = W·beta only
    # ill-conditioned rows (test_gemm_ln_fold's inputs): offsets of 0 / 30 / 300 std by row third
    off = torch.zeros(300, 1, device=dev)
    off[100:200], off[200:] = 30.0, 300.0
    d["x_ill"] = (1.7 * (torch.randn(300, C, device=dev, generator=g) + off
                         + 0.5 * torch.randn(300, 1, device=dev, generator=g))).to(BF)
    mp = multi_pass_m()
    d["x_mp"] = torch.randn(mp, C, device=dev, generator=g).to(BF)
    d["res_mp"] = torch.randn(mp, C, device=dev, generator=g).to(BF)
    return d


def two_launch(x, res, folded, b1, b2):
    """The existing path on the same tensors, planned for the step's row count."""
    d = data()
    M = x.shape[0]
    mul = -(-PLAN_ROWS // M)
    with ops.plan_scaled(mul):
        if folded:
            f = d["fold"] if b1 else d["fold_nob"]
            assert ops.gemm_plan_of(GemmDesc(a0=256, lda0=C, k0=C, a_mode=0, w=f.w.data_ptr(), ldw=C, M=M, N=2 * HID,
                                             K=C, bias=256, act=ops.ACT_GEGLU, out=256, ldc=HID,
                                             ln_fold_s=f.s.data_ptr(), ln_fold_eps=1e-5)) == (8, 1)
            h = f.gemm(x, act=ops.ACT_GEGLU)
        else:
            h = ops.gemm(x, d["w1"], bias=d["b1"] if b1 else None, act=ops.ACT_GEGLU)
        assert ops.gemm_plan_of(GemmDesc(a0=256, lda0=HID, k0=HID, a_mode=0, w=d["w2"].data_ptr(), ldw=HID, M=M,
                                         N=C, K=HID, bias=256, res=256, ld_res=C, out=256, ldc=C)) == (2, 1)
        return ops.gemm(h, d["w2"], bias=d["b2"] if b2 else None, res=res)


def fused(x, res, folded, b1, b2, out=None):
    d = data()
    if folded:
        f = d["fold"] if b1 else d["fold_nob"]
        return ops.ff_fused(x, f.w, d["w2"], b1=f.b, b2=d["b2"] if b2 else None, res=res, ln_fold=(f.s, f.eps),
                            out=out)
    return ops.ff_fused(x, d["w1"], d["w2"], b1=d["b1"] if b1 else None, b2=d["b2"] if b2 else None, res=res,
                        out=out)


@functools.lru_cache(maxsize=None)
def fused_big(folded, b1, b2):
    d = data()
    out = fused(d["x"], d["res"], folded, b1, b2)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def fused_multi_pass(folded):
    d = data()
    out = fused(d["x_mp"], d["res_mp"], folded, True, True)
    torch.cuda.synchronize()
    return out


def mismatch(got, want):
    bad = (got != want)
    return (f"{int(bad.sum())} of {bad.numel()} outputs differ, max |diff| "
            f"{(got.float() - want.float()).abs().max().item():.4g}, first rows {bad.any(1).nonzero()[:4].flatten().tolist()}")


@pytest.mark.parametrize("bias", ["both", "none", "b1", "b2"])
@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("M", MS)
def test_bit_identical_to_the_two_launches(cuda, M, folded, bias):
    """Test 1: torch.equal on the bf16 output, every M, folded and unfolded, with and without b1 / b2."""
    d = data()
    b1, b2 = bias in ("both", "b1"), bias in ("both", "b2")
    x, res = d["x"][:M], d["res"][:M]
    want = two_launch(x, res, folded, b1, b2)
    got = fused_big(folded, b1, b2) if M == MBIG else fused(x, res, folded, b1, b2)
    torch.cuda.synchronize()
    assert torch.equal(got, want), mismatch(got, want)


@pytest.mark.parametrize("folded", [False, True])
def test_bit_identical_over_several_passes(cuda, folded):
    """Test 1 at multi_pass_m() rows: every workgroup walks the weights two or three times."""
    d = data()
    want = two_launch(d["x_mp"], d["res_mp"], folded, True, True)
    got = fused_multi_pass(folded)
    torch.cuda.synchronize()
    assert torch.equal(got, want), mismatch(got, want)


@pytest.mark.parametrize("folded", [False, True])
def test_row_strides(cuda, folded):
    """Test 1's strided case: ldx, ld_res and ldc larger than C; the columns past C of the output rows
    are not touched."""
    d = data()
    M = 300
    xw = torch.zeros(M, C + 64, device=cuda, dtype=BF)
    rw = torch.zeros(M, C + 8, device=cuda, dtype=BF)
    xw[:, :C], rw[:, :C] = d["x"][:M], d["res"][:M]
    xw[:, C:], rw[:, C:] = 7.0, -3.0
    ow = torch.full((M, C + 32), 5.0, device=cuda, dtype=BF)
    fused(xw[:, :C], rw[:, :C], folded, True, True, out=ow[:, :C])
    want = two_launch(d["x"][:M], d["res"][:M], folded, True, True)
    torch.cuda.synchronize()
    assert torch.equal(ow[:, :C], want), mismatch(ow[:, :C], want)
    assert bool((ow[:, C:] == 5.0).all())


@pytest.mark.parametrize("folded", [False, True])
def test_rows_do_not_depend_on_m(cuda, folded):
    """Test 2: rows 0..299 of the M = 4136 result equal the M = 300 result bit for bit, and rows
    0..15 the M = 16 result."""
    d = data()
    big = fused_big(folded, True, True)
    for M in (300, 16):
        small = fused(d["x"][:M], d["res"][:M], folded, True, True)
        torch.cuda.synchronize()
        assert torch.equal(big[:M], small), mismatch(big[:M], small)
    # ... and across passes: the first 4136 rows of the multi-pass launch (its first pass, and rows
    # a later pass of another workgroup would take at this M) against a launch of those rows alone
    mp = fused_multi_pass(folded)
    small = fused(d["x_mp"][:MBIG], d["res_mp"][:MBIG], folded, True, True)
    tail = fused(d["x_mp"][-300:], d["res_mp"][-300:], folded, True, True)
    torch.cuda.synchronize()
    assert torch.equal(mp[:MBIG], small), mismatch(mp[:MBIG], small)
    assert torch.equal(mp[-300:], tail), mismatch(mp[-300:], tail)


def test_folded_ill_conditioned_rows(cuda):
    """Test 3: rows offset by 30 std (the fp32 one-pass variance) and 300 std (the exact second
    pass), mixed with plain rows in one launch: bit-equal to the two-launch folded path."""
    d = data()
    x, res = d["x_ill"], d["res"][:300]
    want = two_launch(x, res, True, True, True)
    got = fused(x, res, True, True, True)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want), mismatch(got, want)


@pytest.mark.parametrize("folded", [False, True])
def test_against_fp64(cuda, folded):
    """Test 4: fp64 (LayerNorm ->) Linear -> GEGLU(erf) -> Linear + residual.  The fused launch's
    error equals the two-launch path's on the same inputs, and both are at bf16 rounding — so
    test 1 does not compare two equally wrong things."""
    d = data()
    M = 300
    x, res = d["x"][:M], d["res"][:M]
    xd = x.double()
    if folded:
        n = d["norm"]
        xd = F.layer_norm(xd, (C,), n.weight.double(), n.bias.double(), n.eps)
        w1 = d["w1f"].double()
    else:
        w1 = d["w1f"].to(BF).double()
    y = xd @ w1.T + d["b1f"].double()
    hid = y[:, :HID] * F.gelu(y[:, HID:])
    ref = hid @ d["w2"].double().T + d["b2"].double() + res.double()
    got = fused(x, res, folded, True, True)
    two = two_launch(x, res, folded, True, True)
    torch.cuda.synchronize()

    def err(t):
        e = t.double() - ref
        return e.abs().max().item(), (e.norm() / ref.norm()).item()

    eg, et = err(got), err(two)
    print(f"folded={folded}: fused max-abs {eg[0]:.5f} rel-L2 {eg[1]:.6f}; two launches {et[0]:.5f} {et[1]:.6f}")
    assert eg == et
    # bf16 output rounding (2^-9 relative, rms over uniform rounding ≈ 2^-9 / sqrt(3)) plus the bf16
    # hidden activation's; outputs are O(1) (the residual), the ff term O(0.1)
    assert eg[1] < 2 ** -8 and eg[0] < 2 ** -7 * ref.abs().max().item()


def test_plan_query_and_refusals(cuda):
    """Test 5: the query takes C = 320 with hidden = 4C only, from its row gate up; ops.ff_fused
    raises on any other shape instead of running something else."""
    h = lib()
    assert h.vd_ff_fused_takes(PLAN_ROWS, C, HID) == 1
    assert ops.ff_fused_takes(PLAN_ROWS, C, HID)
    assert h.vd_ff_fused_takes(PLAN_ROWS, 640, 2560) == 0
    assert h.vd_ff_fused_takes(PLAN_ROWS, C, 2 * C) == 0
    assert h.vd_ff_fused_takes(PLAN_ROWS, 2 * C, HID) == 0
    assert h.vd_ff_fused_takes(16, C, HID) == 0  # below the gate the plan keeps the two launches
    with ops.plan_scaled(PLAN_ROWS // 16):  # ... unless the block is planned as part of a larger one
        assert ops.ff_fused_takes(16, C, HID)
    x = torch.zeros(64, 640, device=cuda, dtype=BF)
    w1 = torch.zeros(2 * 2560, 640, device=cuda, dtype=BF)
    w2 = torch.zeros(640, 2560, device=cuda, dtype=BF)
    with pytest.raises(VdiffError, match="unsupported|1001"):
        ops.ff_fused(x, w1, w2, res=x)
    x = torch.zeros(64, C, device=cuda, dtype=BF)
    with pytest.raises(VdiffError, match="unsupported|1001"):
        ops.ff_fused(x, torch.zeros(4 * C, C, device=cuda, dtype=BF), torch.zeros(C, 2 * C, device=cuda, dtype=BF))
    with pytest.raises(ValueError):
        ops.ff_fused(x, torch.zeros(2 * HID, C, device=cuda, dtype=BF), torch.zeros(C, HID // 2, device=cuda, dtype=BF))
