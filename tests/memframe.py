"""Poison-and-canary framing of kernel operands (tests/test_gpu_memframe.py, tests/test_memframe_host.py).

A kernel's arithmetic tests say nothing about what it does with memory it does not own: a row
read past M whose garbage is multiplied by 0, a store one row or column outside the output, an
output element never stored, a workspace assumed to be zero.  All of these pass while the bytes
around an operand are whatever the allocator left there.  Here every operand is a view inside a
larger allocation that the test owns, and the whole allocation starts as byte 0xFF:

  bf16 / fp32 / fp64 / e4m3   0xFF.. is a NaN      (a stray read that reaches an output poisons it)
  uint8 255, int32 / int64 -1                      (a stray index or count is far out of range)

framed() / framed_1d() / framed_nd() build the views, Frame.assert_intact() compares the guard
bytes (raw bytes, never float values: NaN != NaN), Frame.assert_written() finds output elements
the kernel never stored, and poisoned_empty() makes every torch.empty / torch.empty_like inside a
block — the outputs and workspaces the wrappers allocate themselves — start as 0xFF too.

The tolerance functions of the GPU kernel tests live here as well (tests/test_gpu_kernels.py
imports them): the framed tests hold each op to the bound its arithmetic test uses.
"""
from __future__ import annotations

import contextlib

import torch

POISON = 0xFF
GUARD_ROWS = 256      # the largest row tile in the library
GUARD_BYTES = 1 << 16  # 1-D operands and workspaces: guard bytes on each side
ALIGN = 256           # base alignment of every view (what a fresh allocation has at least)


# ---------------------------------------------------------------- tolerances (unchanged defaults)
def close_bf16(got, want, rel=1 / 128, abs_frac=2e-3):
    want = want.double().cpu()
    got = got.double().cpu()
    scale = want.abs().max().item() + 1e-12
    err = (got - want).abs()
    bound = rel * want.abs() + abs_frac * scale
    bad = (~(err <= bound)).sum().item()  # a NaN is out of tolerance
    assert bad == 0, f"{bad} / {want.numel()} elements out of tolerance; max err {err.max().item():.3e} (scale {scale:.3e})"


def close_f32(got, want, rtol=1e-3, atol=1e-4):
    torch.testing.assert_close(got.double().cpu(), want.double().cpu(), rtol=rtol, atol=atol)


# ---------------------------------------------------------------- frames
class Frame:
    """One poisoned allocation with a view inside it.  `raw` is the whole allocation as bytes;
    the view's element (r, c) starts at byte view_off + r * row_bytes + c * esize of it."""

    def __init__(self, raw, view, view_off, rows, cols, row_bytes, name="", flat=False):
        self.raw, self.view, self.name, self.flat = raw, view, name, flat
        self.view_off, self.rows, self.cols, self.row_bytes = view_off, rows, cols, row_bytes
        self.esize = view.element_size()

    # the bytes of the view inside `t` (a tensor shaped like raw), as a [rows, cols * esize] window
    def _window(self, t):
        return torch.as_strided(t, (self.rows, self.cols * self.esize), (self.row_bytes, 1), self.view_off)

    def load(self, values):
        """Copy `values` (any shape with the view's element count) into the view; returns the view."""
        self.view.copy_(values.to(self.view.dtype).reshape(self.view.shape))
        return self.view

    def poison(self):
        """Back to all 0xFF, view included (an output reused for a second launch)."""
        self.raw.fill_(POISON)
        return self.view

    def where(self, byte_index):
        """(row, column) of a byte of the allocation relative to the view's element (0, 0)."""
        b = int(byte_index) - self.view_off
        if self.flat:                      # a 1-D operand: one row, elements before it negative
            return 0, b // self.esize
        r = b // self.row_bytes            # floor: bytes before the view are in negative rows
        c = (b - r * self.row_bytes) // self.esize
        if c >= self.cols + (self.row_bytes // self.esize - self.cols) // 2:
            r, c = r + 1, c - self.row_bytes // self.esize  # the left slack of the next row
        return r, c

    def assert_intact(self):
        """Every byte of the allocation outside the view is still 0xFF."""
        bad = self.raw != POISON
        self._window(bad).fill_(False)
        n = int(bad.sum().item())
        if n:
            first = bad.nonzero().flatten()[:8].tolist()
            at = ", ".join(f"(row {r}, col {c})" for r, c in (self.where(i) for i in first))
            raise AssertionError(f"frame {self.name!r}: {n} guard bytes written outside the "
                                 f"{self.rows} x {self.cols} view; first at {at} relative to the view")

    def assert_written(self, want=None):
        """No element of the view still holds the all-ones pattern, except where `want` (the
        reference, in any float / integer type) itself rounds to that pattern."""
        left = (self._window(self.raw).reshape(self.rows, self.cols, self.esize) == POISON).all(-1)
        if want is not None:
            w = want.reshape(self.rows, self.cols).to(self.view.dtype).contiguous()
            wb = w.view(torch.uint8).reshape(self.rows, self.cols, self.esize)
            left &= ~(wb == POISON).all(-1).to(left.device)
        n = int(left.sum().item())
        if n:
            first = left.nonzero()[:8].tolist()
            at = ", ".join(f"(row {r}, col {c})" for r, c in first)
            raise AssertionError(f"frame {self.name!r}: {n} of {self.rows * self.cols} output elements "
                                 f"never written; first at {at}")


def _alloc(parent_bytes, view_off, device):
    """A poisoned byte allocation and the offset in it at which a parent of parent_bytes starts so
    that its byte view_off — the view's base — is ALIGN-byte aligned."""
    raw = torch.empty(parent_bytes + ALIGN, dtype=torch.uint8, device=device)
    raw.fill_(POISON)
    start = (-(raw.data_ptr() + view_off)) % ALIGN
    return raw, start


def framed(shape2d, dtype, device, *, col_slack=0, guard_rows=GUARD_ROWS, name=""):
    """(view, frame): a rows x cols view of `dtype` with guard_rows poisoned rows before and after
    it and col_slack poisoned columns on each side (row stride cols + 2 * col_slack), its base
    256-byte aligned, everything — the view included — filled with 0xFF.  col_slack a multiple of
    8 keeps a bf16 row stride 16-byte aligned; any other value gives the unaligned-stride variant."""
    rows, cols = (int(v) for v in shape2d)
    es = torch.empty((), dtype=dtype).element_size()
    stride = cols + 2 * col_slack
    parent_bytes = (rows + 2 * guard_rows) * stride * es
    off = (guard_rows * stride + col_slack) * es
    raw, start = _alloc(parent_bytes, off, device)
    parent = raw[start:start + parent_bytes].view(dtype).view(rows + 2 * guard_rows, stride)
    view = parent[guard_rows:guard_rows + rows, col_slack:col_slack + cols]
    assert view.data_ptr() % ALIGN == 0 and view.stride() == (stride, 1)
    return view, Frame(raw, view, start + off, rows, cols, stride * es, name)


def framed_1d(n, dtype, device, *, guard_bytes=GUARD_BYTES, name=""):
    """(view, frame): n contiguous elements (a vector, or a workspace of exactly n elements) with
    guard_bytes poisoned bytes before and after."""
    n = int(n)
    es = torch.empty((), dtype=dtype).element_size()
    guard_bytes = (guard_bytes + ALIGN - 1) // ALIGN * ALIGN
    raw, start = _alloc(2 * guard_bytes + n * es, guard_bytes, device)
    view = raw[start + guard_bytes:start + guard_bytes + n * es].view(dtype)
    assert view.data_ptr() % ALIGN == 0 and view.numel() == n
    return view, Frame(raw, view, start + guard_bytes, 1, n, max(n * es, 1), name, flat=True)


def framed_nd(shape, dtype, device, *, guard_bytes=GUARD_BYTES, name=""):
    """framed_1d reshaped to a contiguous N-D tensor (latents, images, weight stacks)."""
    n = 1
    for s in shape:
        n *= int(s)
    v, f = framed_1d(n, dtype, device, guard_bytes=guard_bytes, name=name)
    f.view = v.view(*shape)
    return f.view, f


def load2d(values, *, col_slack=0, guard_rows=GUARD_ROWS, name=""):
    """A 2-D input in a frame: (view holding `values`, frame)."""
    v, f = framed(values.shape, values.dtype, values.device, col_slack=col_slack, guard_rows=guard_rows, name=name)
    f.load(values)
    return v, f


def loadnd(values, *, name=""):
    """An input of any shape, contiguous, in a 1-D frame: (view holding `values`, frame)."""
    v, f = framed_nd(values.shape, values.dtype, values.device, name=name)
    f.load(values)
    return v, f


# ---------------------------------------------------------------- poisoned torch.empty
def _poison(t):
    if t.numel() == 0:
        return t
    if t.is_contiguous():
        t.reshape(-1).view(torch.uint8).fill_(POISON)
    elif t.dtype.is_floating_point:
        t.fill_(float("nan"))
    elif t.dtype == torch.bool:
        t.fill_(True)
    else:
        t.fill_(255 if t.dtype == torch.uint8 else -1)
    return t


@contextlib.contextmanager
def poisoned_empty():
    """Inside the block torch.empty and torch.empty_like return 0xFF-filled tensors: every output
    and workspace the code under test allocates itself starts poisoned, never as the previous
    call's answer.  Restored on exit, also through an exception.  Wrap the call under test only."""
    empty, empty_like = torch.empty, torch.empty_like

    def p_empty(*a, **k):
        return _poison(empty(*a, **k))

    def p_empty_like(*a, **k):
        return _poison(empty_like(*a, **k))

    torch.empty, torch.empty_like = p_empty, p_empty_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def is_poison(t):
    """Elementwise: does the element still hold the all-ones byte pattern?"""
    c = t.contiguous()
    return (c.reshape(-1).view(torch.uint8).reshape(-1, c.element_size()) == POISON).all(-1).reshape(c.shape)


def assert_no_poison(t, what="output"):
    """An output the wrapper allocated itself (under poisoned_empty) was written everywhere."""
    n = int(is_poison(t).sum().item())
    assert n == 0, f"{what}: {n} of {t.numel()} elements never written (still 0xFF)"


def assert_all_intact(*frames):
    for f in frames:
        if f is not None:
            f.assert_intact()
