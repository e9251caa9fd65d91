"""Every conv loader in every conv mode at non-power-of-two geometry, on the MI355X: the case table
of tests/conv_ref.py (v1, v2 on its three N tiles and split, v5 and its split form, v6 unsplit and
with its in-kernel split reduce; pad 1 at stride 1 and 2, the nearest-2x upsample, the unequal
channel concat, long taps, a wide image, and the temporal taps of v1 and v2) against fp64 torch on
the same bf16 values.

Each case runs with every operand in a poisoned frame (memframe: x0, x1, the packed weight, the
residual and the output with column slack, bias and row bias in 1-D frames, the split-K workspace
of exactly vd_gemm_ws_bytes bytes in a frame of its own) and checks that the launch is the table's
(kernel, K split), that every output element was written, that no guard byte moved — the taps
past an image's edge are out-of-range buffer reads on v2 / v5 / v6, so intact frames are part of
the claim — that a second call gives the same bits (split-K is deterministic by design), and that
the output is within the project's existing conv bound (conv_ref.tolerance).  What a wrong loader
would do to these cases is measured on the CPU in tests/test_conv_matrix_host.py.
"""
import contextlib
import ctypes

import pytest
import torch

import conv_ref as R
import memframe as mf
from vdiff import ops
from vdiff._lib import check, lib

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


@contextlib.contextmanager
def framed_launches(frames):
    """Inside the block every vd_gemm of vdiff.ops reports the (kernel, split) of the descriptor it
    launches and runs on a framed split-K workspace of exactly the size the library asks for."""
    plans, orig = [], ops._run_gemm

    def run_gemm(d, device, what):
        plans.append(ops.gemm_plan_of(d))
        nbytes = lib().vd_gemm_ws_bytes(ctypes.byref(d))
        if nbytes > 0:
            ws, f = mf.framed_1d(nbytes // 4, F32, device, name="split-K workspace")
            frames.append(f)
            d.ws, d.ws_bytes = ws.data_ptr(), nbytes
        check(lib().vd_gemm(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), what)

    ops._run_gemm = run_gemm
    try:
        yield plans
    finally:
        ops._run_gemm = orig


def run_framed(case, op):
    """One launch of the case: (output view, output frame, every frame, [(kernel, split)])."""
    dev = "cuda"
    frames = []

    def rows(t, slack, name):
        if t is None:
            return None
        v, f = mf.load2d(t.to(dev), col_slack=slack, name=name)
        frames.append(f)
        return v

    def flat(t, name):
        if t is None:
            return None
        v, f = mf.loadnd(t.to(dev), name=name)
        frames.append(f)
        return v

    x0, x1 = rows(op.x0, 8, "x0"), rows(op.x1, 8, "x1")
    wp = rows(R.packed_weight(case, op), 8, "w")
    res = rows(op.res, 4, "res")
    bias, rowbias = flat(op.bias, "bias"), flat(op.rowbias, "rowbias")
    out, fo = mf.framed((case.M, case.cout), F32 if case.out_f32 else BF, dev, col_slack=4, name="out")
    frames.append(fo)
    epi = dict(bias=bias, rowbias=rowbias, rb_div=case.rb_div if case.rowbias else 1, res=res, out=out,
               out_f32=case.out_f32)
    with ops.gemm_plan(path=case.path), ops.plan_scaled(case.mul), mf.poisoned_empty(), \
            framed_launches(frames) as plans:
        if case.is3d:
            _, ho, wo = ops.conv3d(x0, case.n, case.frames_in, case.h, case.w, wp, kt=case.kt, ks=case.ks,
                                   frames_out=case.frames, t_off=case.t_off, stride=case.stride, **epi)
        else:
            _, ho, wo = ops.conv3x3(x0, case.n, case.h, case.w, wp, x1=x1, stride=case.stride, upsample=case.up, **epi)
    torch.cuda.synchronize()
    assert (ho, wo) == (case.h_out, case.w_out)
    return out, fo, frames, plans


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_conv_matrix(cuda, name):
    case = R.BY_NAME[name]
    op = R.operands(case)
    want = R.reference(case, op)
    got, fo, frames, plans = run_framed(case, op)
    assert plans == [(case.kernel, case.split)], f"launched {plans}, the case is for v{case.kernel} split {case.split}"
    assert sum(f.name == "split-K workspace" for f in frames) == int(case.is_split)
    operands = (op.x0, op.x1, op.wt, op.res, op.bias, op.rowbias)
    assert len(frames) == 1 + sum(t is not None for t in operands) + int(case.is_split)
    fo.assert_written(want)
    mf.assert_all_intact(*frames)
    rtol, atol = R.tolerance(case, want)
    ratio = R.worst_ratio(got, want, rtol, atol)
    print(f"conv-matrix {case.family} {name}: v{case.kernel} bn {case.bn} split {case.split}, {case.M} rows, "
          f"worst |got - ref| / bound = {ratio:.4f} (atol {atol:.2e})")
    if case.out_f32:
        mf.close_f32(got, want, rtol=rtol, atol=atol)
    else:
        mf.close_bf16(got, want)
    first = got.clone()
    again, fo2, frames2, plans2 = run_framed(case, op)
    assert plans2 == plans
    fo2.assert_written(want)
    mf.assert_all_intact(*frames2)
    assert torch.equal(first, again), "two calls, two answers"
