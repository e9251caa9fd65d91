"""The framing helper (tests/memframe.py) can fail: small fake "kernels" in torch on CPU tensors,
each wrong in one of the ways the framed GPU tests exist to catch, and the coverage pin that ties
tests/test_gpu_memframe.py's table to the library's entry points."""
import ast
from pathlib import Path

import pytest
import torch

import memframe as mf
from vdiff._lib import SIGNATURES

BF = torch.bfloat16
CPU = torch.device("cpu")


def _operands(M=37, N=20, K=16, col_slack=0, dtype=BF):
    g = torch.Generator().manual_seed(0)
    a, fa = mf.load2d(torch.randn(M, K, generator=g).to(BF), name="a")
    w, fw = mf.load2d(torch.randn(N, K, generator=g).to(BF), name="w")
    out, fo = mf.framed((M, N), dtype, CPU, col_slack=col_slack, name="out")
    want = a.double() @ w.double().T
    return a, w, out, (fa, fw, fo), want


def _gemm(a, w, out):
    """The correct fake kernel: stores every element of out, touches nothing else."""
    out.copy_((a.float() @ w.float().T).to(out.dtype))


def _parent(out, frame):
    """The fake kernels' view of the memory around `out`: rows / columns past the view, as a real
    kernel with a wrong bound would address them."""
    stride = out.stride(0)
    return torch.as_strided(out, (frame.rows + 2, stride), (stride, 1), out.storage_offset() - stride)


# ---------------------------------------------------------------- 0. the poison itself
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn])
def test_poison_is_nan_in_every_float_format(dtype):
    v, _ = mf.framed((3, 8), dtype, CPU, guard_rows=2)
    assert torch.isnan(v.float()).all()


def test_poison_in_integer_formats_and_alignment():
    assert (mf.framed_1d(5, torch.uint8, CPU)[0] == 255).all()
    assert (mf.framed_1d(5, torch.int64, CPU)[0] == -1).all()
    assert (mf.framed_1d(5, torch.int32, CPU)[0] == -1).all()
    for slack in (0, 8, 3):
        v, f = mf.framed((5, 24), BF, CPU, col_slack=slack)
        assert v.data_ptr() % 256 == 0 and v.stride() == (24 + 2 * slack, 1) and v.shape == (5, 24)
        assert f.raw.numel() >= (5 + 2 * mf.GUARD_ROWS) * (24 + 2 * slack) * 2
    v, _ = mf.framed_nd((2, 3, 4), torch.float32, CPU)
    assert v.is_contiguous() and v.data_ptr() % 256 == 0


# ---------------------------------------------------------------- 1. a correct op passes
@pytest.mark.parametrize("col_slack", [0, 8, 3])
def test_correct_op_passes_all_checks(col_slack):
    a, w, out, frames, want = _operands(col_slack=col_slack)
    _gemm(a, w, out)
    mf.assert_all_intact(*frames)
    frames[2].assert_written(want)
    mf.close_bf16(out, want)


# ---------------------------------------------------------------- 2. a store in the row after the view
@pytest.mark.parametrize("where", ["after", "before"])
def test_store_in_the_next_row_is_caught(where):
    a, w, out, frames, want = _operands()
    _gemm(a, w, out)
    p = _parent(out, frames[2])
    p[frames[2].rows + 1 if where == "after" else 0, 0] = 1.0
    with pytest.raises(AssertionError, match=r"guard bytes written.*\(row (37|-1), col 0\)"):
        frames[2].assert_intact()
    frames[0].assert_intact()
    mf.close_bf16(out, want)  # the arithmetic test alone never sees it


def test_store_after_a_1d_workspace_is_caught():
    ws, f = mf.framed_1d(100, torch.float32, CPU, name="ws")
    ws.zero_()
    f.assert_intact()
    torch.as_strided(ws, (101,), (1,), ws.storage_offset())[100] = 0.0  # one element past the end
    with pytest.raises(AssertionError, match=r"4 guard bytes.*col 100"):
        f.assert_intact()


# ---------------------------------------------------------------- 3. a store into the column slack
@pytest.mark.parametrize("col_slack", [8, 3])
def test_store_in_the_column_slack_is_caught(col_slack):
    a, w, out, frames, want = _operands(col_slack=col_slack)
    _gemm(a, w, out)
    p = _parent(out, frames[2])
    p[5 + 1, frames[2].cols] = 0.0  # row 5's first slack column on the right
    with pytest.raises(AssertionError, match=r"\(row 5, col 20\)"):
        frames[2].assert_intact()
    a, w, out, frames, want = _operands(col_slack=col_slack)
    _gemm(a, w, out)
    torch.as_strided(out, (1,), (1,), out.storage_offset() + 7 * out.stride(0) - 1)[0] = 0.0
    with pytest.raises(AssertionError, match=r"\(row 7, col -1\)"):
        frames[2].assert_intact()


def test_a_guard_byte_that_keeps_its_float_value_class_is_caught():
    """The comparison is on bytes: a NaN with another payload is still a write."""
    a, w, out, frames, _ = _operands(dtype=torch.float32)
    _gemm(a, w, out)
    _parent(out, frames[2])[frames[2].rows + 1, 3] = float("nan")  # the canonical NaN 0x7FC00000
    with pytest.raises(AssertionError, match="guard bytes written"):
        frames[2].assert_intact()


# ---------------------------------------------------------------- 4. an output never stored
def test_skipped_last_row_is_caught():
    a, w, out, frames, want = _operands()
    _gemm(a[:-1], w, out[:-1])
    mf.assert_all_intact(*frames)
    with pytest.raises(AssertionError, match=r"20 of 740 output elements never written; first at \(row 36, col 0\)"):
        frames[2].assert_written(want)


def test_skipped_last_n_mod_8_columns_are_caught():
    a, w, out, frames, want = _operands()  # N = 20: 20 % 8 = 4 columns in the tail
    _gemm(a, w[:16], out[:, :16])
    with pytest.raises(AssertionError, match=r"148 of 740 .* \(row 0, col 16\)"):
        frames[2].assert_written(want)


def test_written_allows_what_the_reference_says():
    v, f = mf.framed((2, 4), torch.uint8, CPU, guard_rows=1)
    want = torch.tensor([[1, 2, 255, 4], [5, 6, 7, 8]], dtype=torch.uint8)
    v.copy_(want)
    f.assert_written(want)          # the 255 is data
    with pytest.raises(AssertionError, match=r"1 of 8 .*\(row 0, col 2\)"):
        f.assert_written()


# ---------------------------------------------------------------- 5. 0 * (a read past the input)
def test_zero_times_the_row_past_the_input_is_caught():
    a, w, out, frames, want = _operands()
    stride = a.stride(0)
    past = torch.as_strided(a, (1, a.shape[1]), (stride, 1), a.storage_offset() + a.shape[0] * stride)
    _gemm(a, w, out)
    out[-1] += (0.0 * past.float() @ w.float().T).to(BF)[0]  # "masked" by a multiply, not a select
    mf.assert_all_intact(*frames)
    frames[2].assert_written()      # the all-ones NaN became the canonical one: it was written
    with pytest.raises(AssertionError, match="out of tolerance"):
        mf.close_bf16(out, want)
    with pytest.raises(AssertionError):
        mf.close_f32(out, want)
    plain_a = a.clone()             # the same op on a whole allocation: the gap this closes
    plain_past = torch.zeros(1, a.shape[1])
    got = (plain_a.float() @ w.float().T)
    got[-1] += (0.0 * plain_past @ w.float().T)[0]
    mf.close_bf16(got.to(BF), want)


# ---------------------------------------------------------------- 6. a workspace assumed clear
def _splitk_sum(a, w, out, splits=2):
    """Fake split-K: accumulates the K slices into a workspace it never clears."""
    ws = torch.empty(out.shape, dtype=torch.float32)
    k = a.shape[1] // splits
    for s in range(splits):
        ws += a[:, s * k:(s + 1) * k].float() @ w[:, s * k:(s + 1) * k].float().T
    out.copy_(ws.to(out.dtype))


def test_uncleared_workspace_is_caught_under_poisoned_empty():
    a, w, out, frames, want = _operands()
    with mf.poisoned_empty():
        _splitk_sum(a, w, out)
    with pytest.raises(AssertionError, match="out of tolerance"):
        mf.close_bf16(out, want)
    with mf.poisoned_empty():
        t = torch.empty(3, 5, dtype=torch.int64)
        u = torch.empty_like(out)
        z = torch.empty(0)
        s = torch.empty((), dtype=torch.float32)
    assert (t == -1).all() and torch.isnan(u.float()).all() and z.numel() == 0 and torch.isnan(s)
    assert mf.is_poison(u).all() and not mf.is_poison(torch.zeros(4)).any()
    with pytest.raises(AssertionError, match="never written"):
        mf.assert_no_poison(u)


# ---------------------------------------------------------------- 7. torch.empty comes back
def test_torch_empty_is_restored():
    empty, empty_like = torch.empty, torch.empty_like
    with mf.poisoned_empty():
        assert torch.empty is not empty and torch.empty_like is not empty_like
    assert torch.empty is empty and torch.empty_like is empty_like
    with pytest.raises(RuntimeError, match="boom"):
        with mf.poisoned_empty():
            raise RuntimeError("boom")
    assert torch.empty is empty and torch.empty_like is empty_like
    with mf.poisoned_empty():        # nesting unwinds in order
        with mf.poisoned_empty():
            pass
        assert torch.empty is not empty
    assert torch.empty is empty


# ---------------------------------------------------------------- coverage pin
def _coverage_table():
    """COVERAGE of tests/test_gpu_memframe.py and the names of its test functions, read from the
    source (importing a GPU test module here would be one more thing that can break the pin)."""
    tree = ast.parse((Path(__file__).resolve().parent / "test_gpu_memframe.py").read_text())
    table, tests = None, set()
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", "") == "COVERAGE" for t in node.targets):
            table = ast.literal_eval(node.value)
        if isinstance(node, ast.FunctionDef) and node.name.startswith("test_"):
            tests.add(node.name)
    assert table is not None, "tests/test_gpu_memframe.py has no COVERAGE table"
    return table, tests


def test_every_entry_point_is_framed_or_excused():
    """A new name in vdiff._lib.SIGNATURES must be given a framed test (or a reason it launches
    nothing) in tests/test_gpu_memframe.py's COVERAGE."""
    table, tests = _coverage_table()
    assert set(table) == set(SIGNATURES), (
        f"missing from COVERAGE: {sorted(set(SIGNATURES) - set(table))}; "
        f"not an entry point: {sorted(set(table) - set(SIGNATURES))}")
    for name, value in table.items():
        if isinstance(value, str):
            assert value.startswith("no launch:") and len(value) > 15, f"{name}: give the reason it launches nothing"
        else:
            assert value and all(t in tests for t in value), f"{name}: {value} names no test of the file"
