"""Tensor-level wrappers over the C ABI (include/vdiff.h).

Every function launches HIP kernels on torch's current stream (so it is
hipGraph-capturable) and never falls back to a CPU or torch implementation:
non-CUDA tensors are rejected and a missing library raises.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import math

import torch

from ._lib import VD_EUNSUPPORTED, GemmDesc, check, lib

ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_GELU, ACT_QUICK_GELU = 0, 1, 2, 3, 4
A_DENSE, A_CONV3X3 = 0, 1
CONV_PAD_END = 0x100  # VD_CONV_PAD_END, OR-ed into vd_gemm_desc.stride
BF16 = torch.bfloat16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("vdiff ops run on the GPU only (got a CPU tensor); no CPU fallback")


def _rows(t, dtype=BF16):
    """Validate a 2-D row-major operand (unit inner stride) and return its row stride."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"expected a 2-D row-major tensor, got shape {tuple(t.shape)} strides {t.stride()}")
    if t.dtype != dtype:
        raise ValueError(f"expected {dtype}, got {t.dtype}")
    return t.stride(0)


# ---------------------------------------------------------------- GEMM / conv
class _GemmPlan:
    path = 0       # vd_gemm_desc.path for the GEMMs issued (0 = the automatic plan)
    plan_div = 0   # > 0: plan every GEMM whose M it divides as if M were M / plan_div
    plan_mul = 1   # > 1: plan every GEMM as if M were M * plan_mul (before plan_div)


_PLAN = _GemmPlan()


@contextlib.contextmanager
def plan_scaled(mul: int):
    """Plan every GEMM (and the fused-kernel shape questions) inside the block as if its M were
    `mul` times larger: the motion block run on one of `mul` position chunks
    (FrameShard(overlap_chunks=mul)) then makes every kernel, split-K and LayerNorm-fold decision
    the whole block would, so chunking changes the launch count, never the arithmetic."""
    old = _PLAN.plan_mul
    _PLAN.plan_mul = old * int(mul)
    try:
        yield
    finally:
        _PLAN.plan_mul = old


@contextlib.contextmanager
def gemm_plan(path: int = 0, plan_div: int = 0):
    """Test / benchmark hook on the Python side only — the C ABI takes both values per call in
    vd_gemm_desc and keeps no state.  Inside the block every vd_gemm carries `path` (1 v1, 2 v2,
    3 v3, 5 v5, 6 v6, 8 v8: forced where that kernel takes the shape) and, with plan_div = N, plan_m =
    M / N for each GEMM whose M N divides: an unsharded model planned like one of N frame shards
    (same kernels, split-K and LayerNorm fusion, so the same summation order), which makes the
    sharded-vs-unsharded comparison of tests/test_gpu_dist2.py bit-exact under the product plan."""
    old = (_PLAN.path, _PLAN.plan_div)
    _PLAN.path, _PLAN.plan_div = int(path), int(plan_div)
    try:
        yield
    finally:
        _PLAN.path, _PLAN.plan_div = old


def _planned_m(M):
    """The row count an M-row request is planned for under plan_scaled / gemm_plan(plan_div)."""
    m = int(M) * _PLAN.plan_mul
    if _PLAN.plan_div > 1 and m % _PLAN.plan_div == 0:
        m //= _PLAN.plan_div
    return m


def _plan_controls(d):
    d.path = _PLAN.path
    m = _planned_m(d.M)
    if m != d.M:
        d.plan_m = m


def _plan_query(d):
    """(kernel, split) of vd_gemm_plan for descriptor d exactly as it stands (kernel 0 = refused)."""
    k, sp = C.c_int32(0), C.c_int32(0)
    check(lib().vd_gemm_plan(C.byref(d), C.byref(k), C.byref(sp)), "vd_gemm_plan")
    return k.value, sp.value


def gemm_plan_of(d):
    """(kernel, split) vd_gemm would run for descriptor d under the current gemm_plan controls
    (vd_gemm_plan; kernel 0 = refused)."""
    _plan_controls(d)
    return _plan_query(d)


def _ln_fold_probe(M, N, K, act, rowbias, w=256, ldw=None, s=256):
    """The descriptor that asks the plan about a folded LayerNorm: dummy aligned operands (the
    plan reads sizes and alignments only) unless the weights' own are given."""
    d = GemmDesc(a0=256, lda0=K, k0=K, a_mode=A_DENSE, w=w, ldw=K if ldw is None else ldw, M=M, N=N, K=K,
                 bias=256, act=act, out=256, ldc=N // 2 if act == ACT_GEGLU else N, ln_fold_s=s, ln_fold_eps=1e-5)
    if rowbias:  # the motion block's PE by frame (LnFold(pe=...)): no v8 / v5 plan takes a row bias
        d.rowbias, d.ld_rb, d.rb_div = 256, N, 1
    return d


def ln_fold_runs(M, w, s, *, act=ACT_NONE, rowbias=False):
    """True when vd_gemm runs Linear(LayerNorm(x)) over M rows of x with the norm folded into
    the GEMM (vd_gemm_desc.ln_fold_s: w = W∘gamma, s = its row sums) — the v8 plan (K = 320) or
    an unsplit v6 (the small M of a frame shard); the caller otherwise writes the normalised rows
    and runs the plain GEMM.  Decided by the library's own plan (with plan_div, so a frame shard
    and its unsharded replay decide alike)."""
    N, K = w.shape
    return gemm_plan_of(_ln_fold_probe(M, N, K, act, rowbias, w=_p(w), ldw=_rows(w), s=_p(s)))[0] != 0


# row counts a folded LayerNorm is asked about at prepare time: the UNet's levels at 2-32 images
LN_FOLD_PROBE_M = (256, 1024, 4096, 16384, 32768, 131072)


def ln_fold_shape_ok(N, K, *, act=ACT_NONE, rowbias=False):
    """Whether a folded LayerNorm (ln_fold_s) can run for an N x K Linear at any of the row counts
    the UNet gives it (LN_FOLD_PROBE_M, automatic plan): decides at prepare time which folded
    weights to build."""
    # the automatic plan: asked as it stands, without the gemm_plan controls
    return any(_plan_query(_ln_fold_probe(M, N, K, act, rowbias))[0] != 0 for M in LN_FOLD_PROBE_M)


def _run_gemm(d, device, what):
    """Attach the split-K workspace the C side asks for (if any), then launch."""
    _plan_controls(d)
    nbytes = lib().vd_gemm_ws_bytes(C.byref(d))
    ws = None
    if nbytes > 0:
        ws = torch.empty(nbytes // 4, device=device, dtype=torch.float32)
        d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    check(lib().vd_gemm(C.byref(d), _stream()), what)
    return ws  # keep alive until the launch is enqueued (stream-ordered reuse is safe)


def _set_epilogue(d, M, device, *, bias=None, rowbias=None, rb_div=1, res=None, act=ACT_NONE, out=None,
                  out_f32=False, out_cols=None):
    """Fill the fields every GEMM form shares — bias, row bias, residual, activation and the output
    (allocated M x out_cols, default N, where not given) — validating the operands' layout, and
    return the output."""
    odt = torch.float32 if out_f32 else BF16
    if out is None:
        out = torch.empty(M, d.N if out_cols is None else out_cols, device=device, dtype=odt)
    d.bias, d.rowbias = _p(bias), _p(rowbias)
    d.ld_rb, d.rb_div = rowbias.stride(0) if rowbias is not None else 0, rb_div
    d.res, d.ld_res = _p(res), _rows(res) if res is not None else 0
    d.act = act
    d.out, d.ldc, d.out_f32 = _p(out), _rows(out, odt), int(out_f32)
    return out


def gemm(a, w, *, a1=None, bias=None, rowbias=None, rb_div=1, res=None, act=ACT_NONE,
         out=None, out_f32=False, rmap=None, ln_fold=None):
    """out[m, n] = epi(sum_k cat(a, a1)[m, k] * w[n, k]); a/a1/w bf16, bias/rowbias fp32.
    rmap = (n1, n2, inner): product row m is written (and its residual read) at row rev3(m)
    (vd_gemm_desc.rmap_*, vdiff.dist.frame_shard.rev3_reference).
    ln_fold = (s, eps): a is the UN-normalised input of a LayerNorm folded into this GEMM —
    w = W∘gamma, bias = b + W·beta, s = w's fp32 row sums (vd_gemm_desc.ln_fold_s,
    vdiff.models.layers.LnFold); raises when the plan cannot take it (see ln_fold_runs)."""
    _dev(a, w, a1, bias, rowbias, res, out)
    M = a.shape[0]
    N, K = w.shape
    lda0 = _rows(a)
    k0 = a.shape[1]
    lda1 = _rows(a1) if a1 is not None else 0
    if a1 is not None and (a1.shape[0] != M or k0 + a1.shape[1] != K):
        raise ValueError("concat operand shapes do not add up to K")
    if a1 is None and k0 != K:
        raise ValueError(f"A has {k0} columns, W has K={K}")
    d = GemmDesc(a0=_p(a), lda0=lda0, k0=k0, a1=_p(a1), lda1=lda1, a_mode=A_DENSE,
                 w=_p(w), ldw=_rows(w), M=M, N=N, K=K)
    out = _set_epilogue(d, M, a.device, bias=bias, rowbias=rowbias, rb_div=rb_div, res=res, act=act, out=out,
                        out_f32=out_f32, out_cols=N // 2 if act == ACT_GEGLU else N)
    if rmap is not None:
        d.rmap_n1, d.rmap_n2, d.rmap_inner = (int(v) for v in rmap)
    if ln_fold is not None:
        s, eps = ln_fold
        _dev(s)
        if s.dtype != torch.float32 or not s.is_contiguous() or s.numel() != N:
            raise ValueError("ln_fold s must be a contiguous fp32 vector of N entries")
        d.ln_fold_s, d.ln_fold_eps = _p(s), float(eps)
    _run_gemm(d, a.device, "vd_gemm")
    return out


def gemm_ln(a, w, gamma, beta, *, eps=1e-5, pe=None, pe_div=1, pe_period=1, bias=None, res=None, out=None,
            ln_out=None):
    """(out, ln_out): out = a @ w^T (+ bias) (+ res) in bf16 and ln_out = LayerNorm(out)
    (+ pe[(m / pe_div) % pe_period]) — the GEMM producing a transformer block's residual
    stream with the next norm fused into its epilogue where one tile owns whole rows."""
    _dev(a, w, gamma, beta, pe, bias, res, out, ln_out)
    M = a.shape[0]
    N, K = w.shape
    if a.shape[1] != K:
        raise ValueError(f"A has {a.shape[1]} columns, W has K={K}")
    if ln_out is None:
        ln_out = torch.empty(M, N, device=a.device, dtype=BF16)
    d = GemmDesc(a0=_p(a), lda0=_rows(a), k0=K, a1=None, lda1=0, a_mode=A_DENSE,
                 w=_p(w), ldw=_rows(w), M=M, N=N, K=K,
                 ln_gamma=_p(gamma), ln_beta=_p(beta), ln_eps=eps, ln_pe=_p(pe), ln_pe_div=pe_div,
                 ln_pe_period=pe_period, ln_out=_p(ln_out), ld_ln=_rows(ln_out))
    out = _set_epilogue(d, M, a.device, bias=bias, res=res, out=out)
    _run_gemm(d, a.device, "vd_gemm(ln)")
    return out, ln_out


def ff_fused_takes(M, C, hidden):
    """Whether the product plan runs the FeedForward over M rows as the one fused launch
    (vd_ff_fused_takes: C = 320, hidden = 4C, M at or above its gate).  M goes through the
    plan_scaled / gemm_plan(plan_div) controls like every GEMM's, so a frame shard and its
    unsharded replay decide alike."""
    return bool(lib().vd_ff_fused_takes(_planned_m(M), int(C), int(hidden)))


def ff_fused(x, w1, w2, *, b1=None, b2=None, res=None, ln_fold=None, out=None):
    """out = res + b2 + w2 · bf16(GEGLU(w1' · x + b1)) in one launch (vd_ff_fused: C = 320,
    hidden = 1280, any M): w1 is the packed GEGLU projection [2 hidden][C] (pack_geglu), w2
    [C][hidden]; ln_fold = (s, eps) folds the LayerNorm of x's rows as gemm(ln_fold=) does.
    Bit-identical to gemm(act=ACT_GEGLU) + gemm(res=) under the 131072-row plan; raises on any
    other (C, hidden) — there is no fallback here."""
    _dev(x, w1, w2, b1, b2, res, out)
    M, C_ = x.shape
    ldx = _rows(x)
    if _rows(w1) != w1.shape[1] or _rows(w2) != w2.shape[1]:
        raise ValueError("ff_fused weights must be contiguous")
    hidden = w2.shape[1]
    if w1.shape != (2 * hidden, C_) or w2.shape[0] != C_:
        raise ValueError(f"ff_fused: w1 {tuple(w1.shape)} / w2 {tuple(w2.shape)} do not fit x with C={C_}")
    for t, n in ((b1, 2 * hidden), (b2, C_)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n):
            raise ValueError("ff_fused biases must be contiguous fp32 vectors")
    if res is not None and tuple(res.shape) != (M, C_):
        raise ValueError("ff_fused: res must have x's shape")
    s, eps = (None, 0.0)
    if ln_fold is not None:
        s, eps = ln_fold
        _dev(s)
        if s.dtype != torch.float32 or not s.is_contiguous() or s.numel() != 2 * hidden:
            raise ValueError("ln_fold s must be a contiguous fp32 vector of 2*hidden entries")
    if out is None:
        out = torch.empty(M, C_, device=x.device, dtype=BF16)
    elif tuple(out.shape) != (M, C_):
        raise ValueError("ff_fused: out must have x's shape")
    check(lib().vd_ff_fused(_p(x), ldx, M, C_, hidden, _p(w1), _p(b1), _p(s), float(eps), _p(w2), _p(b2),
                            _p(res), _rows(res) if res is not None else 0, _p(out), _rows(out), _stream()),
          "vd_ff_fused")
    return out


def conv3x3(x, n_img, h_in, w_in, w, *, x1=None, stride=1, upsample=False, pad_end=False, bias=None,
            rowbias=None, rb_div=1, res=None, act=ACT_NONE, out=None, out_f32=False):
    """3x3 pad-1 conv over NHWC rows x (+ channel-concat x1); w packed [Cout][3][3][Cin].
    pad_end (stride 2 only): the VAE encoder's Downsample2D(padding=0) instead —
    conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2), zeros past the far edges only
    (VD_CONV_PAD_END), output (h_in - 2) // 2 + 1 by (w_in - 2) // 2 + 1."""
    _dev(x, w, x1, bias, rowbias, res, out)
    N, K = w.shape
    c0 = x.shape[1]
    if K % 9 or (c0 + (x1.shape[1] if x1 is not None else 0)) * 9 != K:
        raise ValueError("conv weight K does not match input channels")
    if pad_end and (stride != 2 or upsample or h_in < 2 or w_in < 2):
        raise ValueError("pad_end is the stride-2 conv without upsample over at least 2 x 2 pixels")
    if upsample:
        h_out, w_out = 2 * h_in, 2 * w_in
    elif pad_end:
        h_out, w_out = (h_in - 2) // 2 + 1, (w_in - 2) // 2 + 1
    else:
        h_out, w_out = (h_in - 1) // stride + 1, (w_in - 1) // stride + 1
    M = n_img * h_out * w_out
    if x.shape[0] != n_img * h_in * w_in:
        raise ValueError("conv input rows != n_img*h*w")
    d = GemmDesc(a0=_p(x), lda0=_rows(x), k0=c0, a1=_p(x1),
                 lda1=_rows(x1) if x1 is not None else 0, a_mode=A_CONV3X3,
                 n_img=n_img, h_in=h_in, w_in=w_in, h_out=h_out, w_out=w_out,
                 stride=stride | (CONV_PAD_END if pad_end else 0), upsample=int(bool(upsample)),
                 w=_p(w), ldw=_rows(w), M=M, N=N, K=K)
    out = _set_epilogue(d, M, x.device, bias=bias, rowbias=rowbias, rb_div=rb_div, res=res, act=act, out=out,
                        out_f32=out_f32)
    _run_gemm(d, x.device, "vd_gemm(conv3x3)")
    return out, h_out, w_out


def conv3d(x, batch, frames_in, h_in, w_in, w, *, kt=3, ks=3, frames_out=None, t_off=0, stride=1, bias=None,
           rowbias=None, rb_div=1, res=None, act=ACT_NONE, out=None, out_f32=False):
    """kt x ks x ks conv (pad kt/2, ks/2; spatial stride 1/2, temporal stride 1) over the frames
    of each video: x = NHWC rows of batch*frames_in images, w packed [Cout][kt][ks][ks][Cin]
    (K = (dt*ks*ks + tap)*Cin + ci, pack_conv3d).  Output frame f of a video reads input frames
    f + t_off + dt - kt/2 (zero outside [0, frames_in)): frames_out = frames_in, t_off = 0 is
    the plain 3-D conv; a frame-sharded rank passes halo'd frames (frames_in = frames_out + 2,
    t_off = 1).  ks = 1, kt = 3 is the temporal half of a (2+1)D conv."""
    _dev(x, w, bias, rowbias, res, out)
    frames_out = frames_in if frames_out is None else frames_out
    N, K = w.shape
    cin = x.shape[1]
    if K != kt * ks * ks * cin:
        raise ValueError(f"conv3d weight K={K} != kt*ks*ks*Cin = {kt * ks * ks * cin}")
    if x.shape[0] != batch * frames_in * h_in * w_in:
        raise ValueError("conv3d input rows != batch*frames_in*h*w")
    h_out, w_out = (h_in - 1) // stride + 1, (w_in - 1) // stride + 1
    n_img = batch * frames_out
    M = n_img * h_out * w_out
    d = GemmDesc(a0=_p(x), lda0=_rows(x), k0=cin, a1=None, lda1=0, a_mode=A_CONV3X3,
                 n_img=n_img, h_in=h_in, w_in=w_in, h_out=h_out, w_out=w_out, stride=stride, upsample=0,
                 w=_p(w), ldw=_rows(w), M=M, N=N, K=K,
                 kt=kt, ks=ks, frames_in=frames_in, frames_out=frames_out, t_off=t_off)
    out = _set_epilogue(d, M, x.device, bias=bias, rowbias=rowbias, rb_div=rb_div, res=res, act=act, out=out,
                        out_f32=out_f32)
    _run_gemm(d, x.device, "vd_gemm(conv3d)")
    return out, h_out, w_out


# ---------------------------------------------------------------- norms
def gn_splits(n_inst: int, pix: int) -> int:
    """Pixel splits per instance for vd_gn_partial: ~2048 partial blocks in total, at
    most 256 per instance (the finalize pass combines n_split x C/groups records per
    group)."""
    return max(1, min(pix // 16, math.ceil(2048 / n_inst), 256))


def gn_splits_per_frame(hw: int) -> int:
    """Splits per frame of the motion-module norm (instance = a whole video): a function of the
    frame size alone, so a frame-sharded rank's records for its frames are exactly the
    unsharded run's records for those frames and the all-gathered set equals the unsharded one
    record for record — the sharded norm is bit-identical (at F = 16 this is the same 256 / 64
    splits per video as gn_splits)."""
    return max(1, min(hw // 16, 16))


def gn_partial(x, C, n_inst, pix, n_split, x1=None):
    _dev(x, x1)
    ws = torch.empty(n_inst, n_split, C, 4, device=x.device, dtype=torch.float32)
    check(lib().vd_gn_partial(_p(x), _rows(x), x.shape[1], _p(x1), _rows(x1) if x1 is not None else 0,
                              C, n_inst, pix, n_split, _p(ws), _stream()), "vd_gn_partial")
    return ws


def gn_finalize(ws, groups, eps, gamma, beta):
    n_inst, n_split, C, _ = ws.shape
    ss = torch.empty(n_inst, C, 2, device=ws.device, dtype=torch.float32)
    check(lib().vd_gn_finalize(_p(ws), n_inst, n_split, C, groups, eps, _p(gamma), _p(beta), _p(ss),
                               _stream()), "vd_gn_finalize")
    return ss


def gn_partial_g(x, C, n_inst, pix, n_split, groups, x1=None):
    """vd_gn_partial_g: one {n, mean, M2} record per (instance, split, group)."""
    _dev(x, x1)
    ws = torch.empty(n_inst, n_split, groups, 4, device=x.device, dtype=torch.float32)
    x1p, ld1 = (_p(x1), _rows(x1)) if x1 is not None else (None, 0)
    check(lib().vd_gn_partial_g(_p(x), _rows(x), x.shape[1], x1p, ld1, C, n_inst, pix, n_split, groups, _p(ws),
                                _stream()), "vd_gn_partial_g")
    return ws


def gn_finalize_g(ws, C, eps, gamma, beta):
    """ws: [inst, splits, groups, 4] records, or rank-major [ranks, inst, splits of a rank, groups, 4]
    (FrameShard.gather_gn_records: the all-gather output as it lands, vd_gn_finalize_g_ranks)."""
    if ws.dim() == 5:
        n_ranks, n_inst, nsl, groups, _ = ws.shape
        ss = torch.empty(n_inst, C, 2, device=ws.device, dtype=torch.float32)
        check(lib().vd_gn_finalize_g_ranks(_p(ws), n_inst, n_ranks, nsl, C, groups, eps, _p(gamma), _p(beta),
                                           _p(ss), _stream()), "vd_gn_finalize_g_ranks")
        return ss
    n_inst, n_split, groups, _ = ws.shape
    ss = torch.empty(n_inst, C, 2, device=ws.device, dtype=torch.float32)
    check(lib().vd_gn_finalize_g(_p(ws), n_inst, n_split, C, groups, eps, _p(gamma), _p(beta), _p(ss),
                                 _stream()), "vd_gn_finalize_g")
    return ss


def gn_apply(x, ss, pix, silu, x1=None, out=None, rev3=None):
    """rev3 = (n1, n2, inner): input row m lands at output row rev3(m) (vd_gn_apply_rev3)."""
    _dev(x, x1, ss)
    n_inst, C, _ = ss.shape
    if out is None:
        out = torch.empty(x.shape[0], C, device=x.device, dtype=BF16)
    n1, n2, inner = rev3 if rev3 is not None else (1, 1, 0)
    check(lib().vd_gn_apply_rev3(_p(x), _rows(x), x.shape[1], _p(x1), _rows(x1) if x1 is not None else 0,
                                 C, n_inst, pix, _p(ss), int(silu), _p(out), _rows(out), n1, n2, inner,
                                 _stream()), "vd_gn_apply_rev3")
    return out


def group_norm(x, n_inst, pix, groups, eps, gamma, beta, silu=False, x1=None, gather=None, two_pass=True,
               n_split=None, rev3=None):
    """GroupNorm(+SiLU) over NHWC rows; instance = `pix` consecutive rows.
    Image-instance norms (two_pass): per-group partial records, and an apply that finalizes
    them itself (two launches).  The motion-module norm (two_pass=False: its instance is a
    whole video, so it needs hundreds of splits) runs partial / [gather] / finalize / apply,
    where `gather(ws) -> ws'` merges the partial statistics across frame-sharded ranks.
    Image instances always take the two-launch path, whose splits depend on the image size
    alone: a frame-sharded rank normalises its images bit-identically to the unsharded run
    (round 3; the four-launch path was 1-2 us faster on a 2-frame rank's few deep-level
    instances, tools/gn_bench.py).  A one-launch form (blocks waiting for their image's other
    blocks on an arrival counter) was slower at every image norm of the step and is gone
    (round 4, profiles/r04_gn_one_launch_refuted.txt).  Round 5: small image instances (levels
    3-4, the mid block) take vd_gn_small instead — one workgroup per (image, whole-group chunk),
    no cross-block wait, chosen from (pix, C, groups) alone, so the sharded run still matches."""
    C = x.shape[1] + (x1.shape[1] if x1 is not None else 0)
    grec = C <= 2560 and 256 % groups == 0
    if two_pass and gather is None and rev3 is None:
        if gn_small_chunk(pix, C, groups):  # round 5: one launch at the small levels
            return gn_small(x, n_inst, pix, groups, eps, gamma, beta, silu=silu, x1=x1)
        if grec:
            return group_norm_2pass(x, n_inst, pix, groups, eps, gamma, beta, silu=silu, x1=x1)
    n_split = n_split or gn_splits(n_inst, pix)
    if grec:  # per-group records (round 5: C/groups times fewer for the gather and the finalize)
        ws = gn_partial_g(x, C, n_inst, pix, n_split, groups, x1=x1)
        if gather is not None:
            ws = gather(ws)  # [inst, ranks*splits, G, 4], or rank-major [ranks, inst, splits, G, 4]
        ss = gn_finalize_g(ws, C, eps, gamma, beta)
    else:
        ws = gn_partial(x, C, n_inst, pix, n_split, x1=x1)
        if gather is not None:
            ws = gather(ws)
            if ws.dim() == 5:  # rank-major records: vd_gn_finalize takes [inst, ranks*splits, C, 4]
                ws = ws.transpose(0, 1).reshape(n_inst, -1, C, 4).contiguous()
        ss = gn_finalize(ws, groups, eps, gamma, beta)
    return gn_apply(x, ss, pix, silu, x1=x1, rev3=rev3)


GNS_NT, GNS_MAXR, GNS_GMAX = 256, 16, 32


def gn_small_chunk(pix: int, C: int, groups: int) -> int:
    """The channel chunk vd_gn_small takes for this image norm (0 = not taken): the widest whole-group
    chunk dividing C whose rows fit 16 pieces of 8 channels per thread, C / groups a multiple of 8
    (csrc/norm.hip gn_small_chunk; tests/test_ln_fold.py checks the mirror against the library)."""
    if groups <= 0 or C <= 0 or C % groups or pix <= 0 or pix > GNS_NT * GNS_MAXR:
        return 0
    cpg = C // groups
    if cpg % 8:
        return 0
    for cg in range((C // cpg) * cpg, cpg - 1, -cpg):
        if C % cg or cg // 8 > GNS_NT or cg // cpg > GNS_GMAX:
            continue
        rpt = GNS_NT // (cg // 8)
        if -(-pix // rpt) <= GNS_MAXR:
            return cg
    return 0


def gn_small(x, n_inst, pix, groups, eps, gamma, beta, silu=False, x1=None, out=None):
    """vd_gn_small: the one-launch GroupNorm of a small image instance."""
    _dev(x, x1, gamma, beta, out)
    C = x.shape[1] + (x1.shape[1] if x1 is not None else 0)
    if out is None:
        out = torch.empty(x.shape[0], C, device=x.device, dtype=BF16)
    x1p, ld1 = (_p(x1), _rows(x1)) if x1 is not None else (None, 0)
    check(lib().vd_gn_small(_p(x), _rows(x), x.shape[1], x1p, ld1, C, n_inst, pix, groups, eps, _p(gamma), _p(beta),
                            int(silu), _p(out), _rows(out), _stream()), "vd_gn_small")
    return out


def gn_image_splits(pix: int) -> int:
    """Partial records per image instance of vd_gn_partial_g: a function of the image size alone
    (frame-sharded ranks then match the unsharded run bit for bit), at most 32 (the apply prologue
    merges splits x groups records)."""
    return max(1, min(pix // 16, 32))


def gn_apply_blocks(n_inst: int, pix: int, C: int) -> int:
    """Apply blocks per instance of vd_gn_apply_g: ~1024 in all.  Each block re-merges the
    instance's records in its prologue, so a block's rows set how far that prologue is amortised;
    the choice changes no bit (the apply is elementwise on the same {a, b})."""
    return max(1, min(pix, math.ceil(1024 / n_inst)))


def group_norm_2pass(x, n_inst, pix, groups, eps, gamma, beta, silu=False, x1=None, out=None, n_split=None):
    """vd_gn_partial_g + vd_gn_apply_g.  Splits: <= 32 per instance (the apply prologue reads
    splits x groups records); the split count is a function of the image size alone (the same
    records whatever the instance count: frame-sharded ranks match the unsharded run bit for bit);
    ~1024 apply blocks in all (tools/gn_bench.py).  n_split: override (the motion norm's splits
    per frame x frames)."""
    _dev(x, x1, gamma, beta, out)
    C = x.shape[1] + (x1.shape[1] if x1 is not None else 0)
    n_split = n_split or gn_image_splits(pix)
    ws = gn_partial_g(x, C, n_inst, pix, n_split, groups, x1=x1)
    x1p, ld1 = (_p(x1), _rows(x1)) if x1 is not None else (None, 0)
    if out is None:
        out = torch.empty(x.shape[0], C, device=x.device, dtype=BF16)
    rows_per_blk = math.ceil(pix / gn_apply_blocks(n_inst, pix, C))
    check(lib().vd_gn_apply_g(_p(x), _rows(x), x.shape[1], x1p, ld1, C, n_inst, pix, _p(ws), n_split, groups, eps,
                              _p(gamma), _p(beta), int(silu), _p(out), _rows(out), rows_per_blk, _stream()),
          "vd_gn_apply_g")
    return out


def layer_norm(x, gamma, beta, eps=1e-5, pe=None, pe_div=1, pe_period=1, out=None):
    _dev(x, gamma, beta, pe)
    rows, Cc = x.shape
    if out is None:
        out = torch.empty(rows, Cc, device=x.device, dtype=BF16)
    check(lib().vd_layernorm(_p(x), _rows(x), rows, Cc, _p(gamma), _p(beta), eps, _p(pe), pe_div,
                             pe_period, _p(out), _rows(out), _stream()), "vd_layernorm")
    return out


# ---------------------------------------------------------------- attention
ATTN_KERNELS = {"auto": 0, "v1": 1, "flash32": 2, "flash40": 3}
ATTN_CAUSAL = 0x100  # VD_ATTN_CAUSAL, OR-ed into vd_attention_ex's kernel argument
ATTN_TAIL_SHIFT = 16  # VD_ATTN_TAIL(n) = n << 16, n in 1..64 (mask 0x7f0000)
ATTN_TAP = None  # bench hook: callable(q, k, v, batch, heads, sq, skv, d, scale) seen by every attention call


def attention(q, k, v, batch, heads, sq, skv, d, kv_div=1, scale=None, out=None, out_f32=False, kernel="auto",
              causal=False, tail=0):
    """q/k/v: 2-D row views (may be column slices of a fused QKV buffer).  out_f32: O in fp32
    (the tests' north-star-tolerance mode).  kernel: "auto" (the product choice) or, for the
    parity tests, "v1" / "flash32" / "flash40" (vd_attention_ex).  causal: query i attends to
    keys j <= i (VD_ATTN_CAUSAL: sq == skv, kv_div == 1, d 32 or 64; the CLIP text encoder).
    tail: n in 1..64 makes the call two-segment (VD_ATTN_TAIL(n), the IP-Adapter image prompt).
    Row layout: each key batch still owns skv consecutive rows of k and v; rows [0, skv - n) are
    segment A (the text), rows [skv - n, skv) segment B (the image tokens), and the result is
    softmax(q K_A^T) V_A + softmax(q K_B^T) V_B — any adapter scale is already folded into V_B.
    d in {32, 40, 64, 80, 160}, n < skv, never with causal."""
    if not 0 <= tail <= 0x7f:
        raise ValueError(f"tail must be in 0..127 to fit VD_ATTN_TAIL_MASK, got {tail}")
    _dev(q, k, v, out)
    if out is None:
        out = torch.empty(batch * sq, heads * d, device=q.device, dtype=torch.float32 if out_f32 else BF16)
    scale = d ** -0.5 if scale is None else scale
    if ATTN_TAP is not None:
        ATTN_TAP(q, k, v, batch, heads, sq, skv, d, scale)
    check(lib().vd_attention_ex(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0),
                                batch, heads, sq, skv, d, kv_div, scale, int(out_f32),
                                ATTN_KERNELS[kernel] | (ATTN_CAUSAL if causal else 0) | (tail << ATTN_TAIL_SHIFT),
                                _stream()), "vd_attention_ex")
    return out


ATTN_FAMILIES = {1: "flash", 2: "flash32", 3: "flash40", 4: "flash80", 5: "flash512"}  # VD_ATTN_K_*
AttentionPlan = collections.namedtuple("AttentionPlan", "rc family qblk unit_scale grid exact_grid")


def _attention_plan_query(o, ldo, batch, heads, sq, skv, d, kv_div, scale, out_f32, word):
    """vd_attention_plan on raw values (o is an address): rc is its return code, not checked."""
    fam, qb, us = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    g, eg = C.c_int64(0), C.c_int64(0)
    rc = lib().vd_attention_plan(o, ldo, batch, heads, sq, skv, d, kv_div, scale, int(out_f32), word, C.byref(fam),
                                 C.byref(qb), C.byref(us), C.byref(g), C.byref(eg))
    return AttentionPlan(rc, fam.value, qb.value, us.value, g.value, eg.value)


def attention_plan(q, k, v, batch, heads, sq, skv, d, kv_div=1, scale=None, out=None, out_f32=False, kernel="auto",
                   causal=False, tail=0):
    """What attention() would run for the same arguments (vd_attention_plan: no launch, works
    without a device): an AttentionPlan whose family is a name of ATTN_FAMILIES.  q / k / v are
    not looked at; out=None stands for the aligned, dense output attention() would allocate."""
    o, ldo = (256, heads * d) if out is None else (_p(out), out.stride(0))
    scale = d ** -0.5 if scale is None else scale
    p = _attention_plan_query(o, ldo, batch, heads, sq, skv, d, kv_div, scale, out_f32,
                              ATTN_KERNELS[kernel] | (ATTN_CAUSAL if causal else 0) | (tail << ATTN_TAIL_SHIFT))
    check(p.rc, "vd_attention_plan")
    return p._replace(family=ATTN_FAMILIES[p.family])


def temporal_attention(q, k, v, batch, frames, positions, heads, d, scale=None, out=None, rope_theta=None,
                       valu=False):
    """rope_theta: apply the temporal 1-D RoPE (rope_qk mode 1) to q/k inside the kernel
    (vd_temporal_attention_rope: d = 64, 17..32 frames); q and k are read un-rotated.
    valu: the VALU kernel for every shape (vd_temporal_attention_valu; parity tests)."""
    _dev(q, k, v, out)
    if not (q.stride(0) == k.stride(0) == v.stride(0)):
        raise ValueError("q/k/v must share a row stride")
    if out is None:
        out = torch.empty(q.shape[0], heads * d, device=q.device, dtype=BF16)
    scale = d ** -0.5 if scale is None else scale
    if rope_theta is not None:
        if not valu:
            check(lib().vd_temporal_attention_rope(_p(q), _p(k), _p(v), q.stride(0), _p(out), out.stride(0), batch,
                                                   frames, positions, heads, d, scale, rope_theta, _stream()),
                  "vd_temporal_attention_rope")
            return out
        # the VALU kernel has no fused RoPE: rotate a COPY of q|k (the caller's buffer stays
        # un-rotated, as the fused kernel leaves it), then attend on the copy
        C = heads * d
        qkv = torch.empty(q.shape[0], 3 * C, device=q.device, dtype=BF16)
        qkv[:, :C].copy_(q[:, :C])
        qkv[:, C:2 * C].copy_(k[:, :C])
        qkv[:, 2 * C:].copy_(v[:, :C])
        rope_qk(qkv, 2 * C, d, 1, frames, 1, positions, rope_theta)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    fn = lib().vd_temporal_attention_valu if valu else lib().vd_temporal_attention
    check(fn(_p(q), _p(k), _p(v), q.stride(0), _p(out), out.stride(0), batch, frames, positions, heads, d, scale,
             _stream()), "vd_temporal_attention")
    return out


def motion_qkv_takes(batch, frames, positions, heads, d):
    """Whether vd_motion_qkv_attention takes this shape (vd_motion_qkv_attention_takes; no launch).
    Under gemm_plan(plan_div=N) the question is asked for one of N frame shards (batch 1, the
    positions divided by N), so an unsharded replay folds the motion norms exactly where a shard would."""
    # not _planned_m: the shard is (batch 1, positions / N), and without a shard batch stays as it is
    positions *= _PLAN.plan_mul
    if _PLAN.plan_div > 1 and (batch * positions) % _PLAN.plan_div == 0:
        batch, positions = 1, batch * positions // _PLAN.plan_div
    return bool(lib().vd_motion_qkv_attention_takes(batch, frames, positions, heads, d))


def motion_qkv_attention(x, wqkv, batch, frames, positions, heads, d, scale=None, out=None, ln_fold=None):
    """Temporal attention over frames with the fused Q/K/V projection folded in
    (vd_motion_qkv_attention): x = normed rows (b, f, p), wqkv = [3C][C].  Returns None where
    the fused kernel does not take the shape (the caller runs gemm + temporal_attention).
    ln_fold = (table, eps): x holds the UN-normalised rows and the block's LayerNorm + PE are
    folded in (wqkv = W∘gamma; vdiff.models.blocks.MotionLnFold builds the table)."""
    _dev(x, wqkv, out)
    C = heads * d
    if out is None:
        out = torch.empty(x.shape[0], C, device=x.device, dtype=BF16)
    scale = d ** -0.5 if scale is None else scale
    tab, eps = (None, 0.0) if ln_fold is None else ln_fold
    if tab is not None:
        _dev(tab)
        if tab.dtype != torch.float32 or not tab.is_contiguous() or tab.numel() != 8 * 2048:
            raise ValueError("ln_fold table must be a contiguous fp32 [8][2048]")
    rc = lib().vd_motion_qkv_attention(_p(x), _rows(x), _p(wqkv), _rows(wqkv), _p(out), _rows(out), batch, frames,
                                       positions, heads, d, scale, _p(tab), float(eps), _stream())
    if rc == VD_EUNSUPPORTED:
        return None
    check(rc, "vd_motion_qkv_attention")
    return out


def temporal_attention_kv(q, k, v, batch, qframes, kframes, positions, heads, d, scale=None, out=None):
    """A rank's own `qframes` query frames (rows (b, qframes, p) of q) against `kframes` key
    frames (rows (b, kframes, p) of k/v, e.g. all-gathered from every frame shard)."""
    _dev(q, k, v, out)
    if k.stride(0) != v.stride(0):
        raise ValueError("k/v must share a row stride")
    if out is None:
        out = torch.empty(q.shape[0], heads * d, device=q.device, dtype=BF16)
    scale = d ** -0.5 if scale is None else scale
    check(lib().vd_temporal_attention_kv(_p(q), q.stride(0), _p(k), _p(v), k.stride(0), _p(out), out.stride(0),
                                         batch, qframes, kframes, positions, heads, d, scale, _stream()),
          "vd_temporal_attention_kv")
    return out


def softmax_rows(s, out=None):
    """fp32 scores [rows, cols] in log2 units -> bf16 probabilities (row softmax)."""
    _dev(s, out)
    rows, cols = s.shape
    if out is None:
        out = torch.empty(rows, cols, device=s.device, dtype=BF16)
    check(lib().vd_softmax_rows(_p(s), s.stride(0), rows, cols, _p(out), out.stride(0), _stream()),
          "vd_softmax_rows")
    return out


# ---------------------------------------------------------------- exact-fp32 conv / LPIPS tap
def _f32(t, what):
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32, got {t.dtype}")
    return t.contiguous()


def conv2d_f32(x, w, bias=None, stride=1, pad=0, relu=False, out=None):
    """Exact-fp32 convolution on the f32-input MFMA: x NHWC [N, H, W, Cin], w OHWI
    [Cout, kh, kw, Cin], bias [Cout] -> NHWC [N, OH, OW, Cout] (zero padding).  Cout % 64 == 0,
    Cin % 4 == 0 or Cin == 3."""
    _dev(x, w, bias, out)
    x, w = _f32(x, "conv2d_f32 x"), _f32(w, "conv2d_f32 w")
    bias = None if bias is None else _f32(bias, "conv2d_f32 bias")
    if x.dim() != 4 or w.dim() != 4 or x.shape[3] != w.shape[3]:
        raise ValueError(f"conv2d_f32: x {tuple(x.shape)} (NHWC) does not fit w {tuple(w.shape)} (OHWI)")
    N, H, W, Cin = x.shape
    Cout, kh, kw, _ = w.shape
    if H + 2 * pad < kh or W + 2 * pad < kw:
        raise ValueError(f"conv2d_f32: a {kh}x{kw} kernel does not fit {H}x{W} with padding {pad}")
    OH, OW = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty(N, OH, OW, Cout, device=x.device, dtype=torch.float32)
    check(lib().vd_conv2d_f32(_p(x), N, H, W, Cin, _p(w), _p(bias), Cout, kh, kw, stride, pad, int(relu), _p(out),
                              _stream()), "vd_conv2d_f32")
    return out


def lpips_layer(fa, fb, lin, out=None, accumulate=False):
    """One LPIPS tap: feature maps fa, fb fp32 [pairs, pixels, C] and lin [C] -> fp64 [pairs], the
    pixel mean of sum_c lin[c] (fa/|fa| - fb/|fb|)^2; added to `out` when accumulate."""
    _dev(fa, fb, lin, out)
    fa, fb, lin = _f32(fa, "lpips_layer fa"), _f32(fb, "lpips_layer fb"), _f32(lin, "lpips_layer lin")
    if fa.dim() != 3 or fa.shape != fb.shape or lin.numel() != fa.shape[2]:
        raise ValueError(f"lpips_layer: fa {tuple(fa.shape)}, fb {tuple(fb.shape)}, lin {tuple(lin.shape)}")
    pairs, pixels, Cc = fa.shape
    if out is None:
        if accumulate:
            raise ValueError("lpips_layer: accumulate needs an out tensor")
        out = torch.empty(pairs, device=fa.device, dtype=torch.float64)
    nb = lib().vd_lpips_layer_workspace(pairs)
    ws = torch.empty(max(nb, 8), device=fa.device, dtype=torch.uint8)
    check(lib().vd_lpips_layer(_p(fa), _p(fb), pairs, pixels, Cc, _p(lin), _p(out), int(accumulate), _p(ws), nb,
                               _stream()), "vd_lpips_layer")
    return out


# ---------------------------------------------------------------- step glue
def timestep_embed(ts, dim, step_idx=None, batch=None, out=None):
    _dev(ts, step_idx)
    B = ts.numel() if step_idx is None else batch
    if out is None:
        out = torch.empty(B, dim, device=ts.device, dtype=BF16)
    check(lib().vd_timestep_embed(_p(ts), ts.numel(), _p(step_idx), B, dim, _p(out), _stream()), "vd_timestep_embed")
    return out


def pack_latents(x, dup=1, cpad=8, out=None, in_div=1.0):
    _dev(x, out)
    x = x.contiguous().float()
    B, Cc, Fr, H, W = x.shape
    if out is None:
        out = torch.empty(dup * B * Fr * H * W, cpad, device=x.device, dtype=BF16)
    check(lib().vd_pack_latents(_p(x), B, Cc, Fr, H, W, dup, _p(out), cpad, float(in_div), _stream()), "vd_pack_latents")
    return out


def unpack_nhwc(src, B, Cc, Fr, H, W, out=None):
    _dev(src, out)
    if out is None:
        out = torch.empty(B, Cc, Fr, H, W, device=src.device, dtype=torch.float32)
    check(lib().vd_unpack_nhwc(_p(src), int(src.dtype == torch.float32), src.stride(0), B, Cc, Fr, H, W,
                               _p(out), _stream()), "vd_unpack_nhwc")
    return out


STEP_PAG = 0x800  # VD_STEP_PAG, OR-ed into either step's ncfg: perturbed-attention guidance


def pag_prefix(n_steps):
    """Floats of the PAG prefix of a step's coef buffer: n_steps scales, padded to a multiple of 4."""
    return (n_steps + 3) // 4 * 4


def pag_scales(scales):
    """The per-step PAG scales as a validated fp32 CPU tensor: finite and >= 0, or ValueError (the
    C side cannot read a device table, include/vdiff.h)."""
    t = torch.as_tensor(scales, dtype=torch.float32).detach().cpu().reshape(-1)
    if t.numel() == 0 or not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
        raise ValueError(f"PAG scales must be a non-empty list of finite values >= 0, got {t.tolist()}")
    return t


def pag_coef(scales, coef):
    """The coef buffer of a VD_STEP_PAG step: the validated scales, zero padding to a multiple of 4
    floats, then `coef` (the scheduler's rows, or rows and slabs) flattened, in one fp32 buffer on
    coef's device.  Pass it to a step op with pag_n=len(scales)."""
    t = pag_scales(scales)
    body = coef.reshape(-1)
    if body.dtype != torch.float32:
        raise ValueError("pag_coef: coef must be fp32")
    out = torch.zeros(pag_prefix(t.numel()) + body.numel(), device=coef.device, dtype=torch.float32)
    out[:t.numel()].copy_(t)
    out[pag_prefix(t.numel()):].copy_(body)
    return out


def _pag_split(name, coef, pag_n, ncfg):
    """(flag word, coef body) of a step op: with pag_n > 0, coef is pag_coef's flat buffer."""
    if not pag_n:
        return ncfg, coef
    if coef.dtype != torch.float32 or coef.dim() != 1 or not coef.is_contiguous() or \
            coef.numel() <= pag_prefix(pag_n):
        raise ValueError(f"{name}: with pag_n={pag_n}, coef is the flat fp32 buffer of ops.pag_coef "
                         f"({pag_prefix(pag_n)} floats of scales, then the scheduler's table)")
    return ncfg | STEP_PAG, coef[pag_prefix(pag_n):]


def _pag_rows(name, n, pag_n):
    if pag_n and n != pag_n:
        raise ValueError(f"{name}: {pag_n} PAG scales in front of a table of {n} steps")


def ddim_cfg_step(eps, ncfg, guidance, latents, coef, step_idx=None, x0_out=None, next_in=None, pag_n=0):
    """pag_n > 0: perturbed-attention guidance (VD_STEP_PAG) — eps holds ncfg = 2 or 3 branches, the
    last one perturbed, and coef is ops.pag_coef(scales, rows) with pag_n scales.  Likewise below."""
    _dev(eps, latents, coef, step_idx, x0_out, next_in)
    if latents.dtype != torch.float32 or not latents.is_contiguous():
        raise ValueError("latents must be contiguous fp32")
    B, Cc, Fr, H, W = latents.shape
    ncfg, body = _pag_split("ddim_cfg_step", coef, pag_n, ncfg)
    _pag_rows("ddim_cfg_step", body.numel() // 4, pag_n)
    check(lib().vd_ddim_cfg_step(_p(eps), eps.stride(0), ncfg, guidance, _p(latents), B, Cc, Fr, H, W,
                                 _p(coef), body.numel() // 4, _p(step_idx), _p(x0_out), _p(next_in),
                                 next_in.shape[1] if next_in is not None else 0, _stream()),
          "vd_ddim_cfg_step")


def euler_cfg_step(eps, ncfg, guidance, latents, coef, step_idx=None, x0_out=None, next_in=None, pag_n=0):
    """CFG combine + EulerDiscreteScheduler.step (+ next input's scale_model_input), fused."""
    _dev(eps, latents, coef, step_idx, x0_out, next_in)
    if latents.dtype != torch.float32 or not latents.is_contiguous():
        raise ValueError("latents must be contiguous fp32")
    B, Cc, Fr, H, W = latents.shape
    ncfg, body = _pag_split("euler_cfg_step", coef, pag_n, ncfg)
    _pag_rows("euler_cfg_step", body.numel() // 4, pag_n)
    check(lib().vd_euler_cfg_step(_p(eps), eps.stride(0), ncfg, guidance, _p(latents), B, Cc, Fr, H, W,
                                  _p(coef), body.numel() // 4, _p(step_idx), _p(x0_out), _p(next_in),
                                  next_in.shape[1] if next_in is not None else 0, _stream()),
          "vd_euler_cfg_step")


STEP_LCM = 0x100  # VD_STEP_LCM, OR-ed into vd_ddim_cfg_step's ncfg
LCM_ROW = 8       # floats per LCM coefficient row


def lcm_buffer_numel(n_steps, latent_numel):
    """Floats of the LCM coef buffer: n_steps rows of LCM_ROW, then n_steps noise slabs."""
    return n_steps * (LCM_ROW + latent_numel)


def lcm_cfg_step(eps, ncfg, guidance, latents, coef, step_idx=None, x0_out=None, next_in=None, pag_n=0):
    """CFG combine + LCMScheduler.step, fused (vd_ddim_cfg_step with VD_STEP_LCM).  `coef` is the
    rows-plus-slabs buffer of include/vdiff.h: n rows of 8 floats, then n noise slabs of
    latents.numel() floats; n is derived from its size.  x0_out receives diffusers' `denoised`."""
    _dev(eps, latents, coef, step_idx, x0_out, next_in)
    if latents.dtype != torch.float32 or not latents.is_contiguous():
        raise ValueError("latents must be contiguous fp32")
    if coef.dtype != torch.float32 or not coef.is_contiguous():
        raise ValueError("lcm_cfg_step: coef must be a contiguous fp32 buffer")
    ncfg, body = _pag_split("lcm_cfg_step", coef, pag_n, ncfg)
    per = LCM_ROW + latents.numel()
    if body.numel() == 0 or body.numel() % per:
        raise ValueError(f"lcm_cfg_step: coef holds {body.numel()} floats, not a multiple of "
                         f"{LCM_ROW} + {latents.numel()} (rows, then one noise slab per row)")
    _pag_rows("lcm_cfg_step", body.numel() // per, pag_n)
    B, Cc, Fr, H, W = latents.shape
    check(lib().vd_ddim_cfg_step(_p(eps), eps.stride(0), ncfg | STEP_LCM, guidance, _p(latents), B, Cc, Fr, H, W,
                                 _p(coef), body.numel() // per, _p(step_idx), _p(x0_out), _p(next_in),
                                 next_in.shape[1] if next_in is not None else 0, _stream()),
          "vd_ddim_cfg_step (VD_STEP_LCM)")


STEP_DPM = 0x400  # VD_STEP_DPM, OR-ed into vd_ddim_cfg_step's ncfg
DPM_ROW = 8       # floats per DPM-Solver coefficient row


def dpm_buffer_numel(n_steps, latent_numel, sde):
    """Floats of the DPM coef buffer: n_steps rows of DPM_ROW and, for the SDE type, n_steps noise
    slabs behind them (LCM's layout); the deterministic type has rows alone."""
    return n_steps * (DPM_ROW + (latent_numel if sde else 0))


def dpm_cfg_step(eps, ncfg, guidance, latents, coef, step_idx=None, x0_out=None, next_in=None, pag_n=0):
    """CFG combine + DPMSolverMultistepScheduler.step, fused (vd_ddim_cfg_step with VD_STEP_DPM).
    `coef` is the buffer of include/vdiff.h.  Its shape tells which of the two layouts it has:
    [n, 8] is a table of rows alone (the deterministic type: no row of it may carry the SDE
    flag, whose slab the kernel would look for behind the rows); a flat buffer holds n rows and
    then n noise slabs of latents.numel() floats, n derived from its size.
    x0_out is required: the history, the previous step's x0 on entry and this step's on exit.
    With pag_n > 0 the buffer is flat either way and pag_n tells the layouts apart: pag_n rows
    alone, or pag_n rows and pag_n slabs."""
    _dev(eps, latents, coef, step_idx, x0_out, next_in)
    if latents.dtype != torch.float32 or not latents.is_contiguous():
        raise ValueError("latents must be contiguous fp32")
    if coef.dtype != torch.float32 or not coef.is_contiguous():
        raise ValueError("dpm_cfg_step: coef must be a contiguous fp32 buffer")
    if x0_out is None or x0_out.dtype != torch.float32 or not x0_out.is_contiguous() \
            or x0_out.numel() != latents.numel():
        raise ValueError("dpm_cfg_step: x0_out (the multistep history, in and out) must be a contiguous fp32 "
                         "tensor of the latents' size")
    ncfg, body = _pag_split("dpm_cfg_step", coef, pag_n, ncfg)
    if pag_n:
        if body.numel() not in (pag_n * DPM_ROW, pag_n * (DPM_ROW + latents.numel())):
            raise ValueError(f"dpm_cfg_step: behind {pag_n} PAG scales coef holds {body.numel()} floats, neither "
                             f"{pag_n} rows of {DPM_ROW} nor those and {pag_n} slabs of {latents.numel()}")
        n = pag_n
    elif coef.dim() == 2:
        if coef.shape[1] != DPM_ROW or coef.shape[0] == 0:
            raise ValueError(f"dpm_cfg_step: a 2-D coef is [n, {DPM_ROW}] rows, got {tuple(coef.shape)}")
        n = coef.shape[0]
    else:
        per = DPM_ROW + latents.numel()
        if coef.dim() != 1 or coef.numel() == 0 or coef.numel() % per:
            raise ValueError(f"dpm_cfg_step: a flat coef holds rows and slabs; {coef.numel()} floats are not a "
                             f"multiple of {DPM_ROW} + {latents.numel()} (a table of rows alone is [n, {DPM_ROW}])")
        n = coef.numel() // per
    B, Cc, Fr, H, W = latents.shape
    check(lib().vd_ddim_cfg_step(_p(eps), eps.stride(0), ncfg | STEP_DPM, guidance, _p(latents), B, Cc, Fr, H, W,
                                 _p(coef), n, _p(step_idx), _p(x0_out), _p(next_in),
                                 next_in.shape[1] if next_in is not None else 0, _stream()),
          "vd_ddim_cfg_step (VD_STEP_DPM)")


STEP_UNIPC = 0x2000  # VD_STEP_UNIPC, OR-ed into vd_ddim_cfg_step's ncfg
UNIPC_ROW = 16       # floats per UniPC coefficient row


def unipc_cfg_step(eps, ncfg, guidance, latents, coef, step_idx=None, x0_out=None, next_in=None, pag_n=0):
    """CFG combine + UniPCMultistepScheduler.step — the previous step's corrector and this step's
    predictor — fused (vd_ddim_cfg_step with VD_STEP_UNIPC).  `coef` is [n, 16] rows
    (include/vdiff.h); with pag_n > 0 the flat buffer of ops.pag_coef with pag_n such rows.
    x0_out is required: the solver's state, three slabs of the latents' size ([3, *latents.shape]):
    the last two x0 predictions and the sample the previous predictor started from, in and out."""
    _dev(eps, latents, coef, step_idx, x0_out, next_in)
    if latents.dtype != torch.float32 or not latents.is_contiguous():
        raise ValueError("latents must be contiguous fp32")
    if coef.dtype != torch.float32 or not coef.is_contiguous():
        raise ValueError("unipc_cfg_step: coef must be a contiguous fp32 buffer")
    if x0_out is None or x0_out.dtype != torch.float32 or not x0_out.is_contiguous() \
            or x0_out.numel() != 3 * latents.numel():
        raise ValueError("unipc_cfg_step: x0_out (the solver's state, in and out) must be a contiguous fp32 "
                         "tensor of three times the latents' size")
    ncfg, body = _pag_split("unipc_cfg_step", coef, pag_n, ncfg)
    if pag_n:
        if body.numel() != pag_n * UNIPC_ROW:
            raise ValueError(f"unipc_cfg_step: behind {pag_n} PAG scales coef holds {body.numel()} floats, not "
                             f"{pag_n} rows of {UNIPC_ROW}")
        n = pag_n
    else:
        if coef.dim() != 2 or coef.shape[1] != UNIPC_ROW or coef.shape[0] == 0:
            raise ValueError(f"unipc_cfg_step: coef is [n, {UNIPC_ROW}] rows, got {tuple(coef.shape)}")
        n = coef.shape[0]
    B, Cc, Fr, H, W = latents.shape
    check(lib().vd_ddim_cfg_step(_p(eps), eps.stride(0), ncfg | STEP_UNIPC, guidance, _p(latents), B, Cc, Fr, H, W,
                                 _p(coef), n, _p(step_idx), _p(x0_out), _p(next_in),
                                 next_in.shape[1] if next_in is not None else 0, _stream()),
          "vd_ddim_cfg_step (VD_STEP_UNIPC)")


STEP_ANCESTRAL = 0x4000  # VD_STEP_ANCESTRAL, OR-ed into vd_euler_cfg_step's ncfg
EULER_A_ROW = 4          # floats per Euler-ancestral coefficient row


def euler_a_buffer_numel(n_steps, latent_numel):
    """Floats of the Euler-ancestral coef buffer: n_steps rows of EULER_A_ROW, then n_steps noise slabs."""
    return n_steps * (EULER_A_ROW + latent_numel)


def euler_ancestral_cfg_step(eps, ncfg, guidance, latents, coef, step_idx=None, x0_out=None, next_in=None,
                             pag_n=0):
    """CFG combine + EulerAncestralDiscreteScheduler.step (+ next input's scale_model_input), fused
    (vd_euler_cfg_step with VD_STEP_ANCESTRAL).  `coef` is the rows-plus-slabs buffer of
    include/vdiff.h: n rows of 4 floats {sigma, sigma_down, sqrt(sigma_to^2 + 1), sigma_up}, then n
    noise slabs of latents.numel() floats; n is derived from its size.  x0_out receives x0."""
    _dev(eps, latents, coef, step_idx, x0_out, next_in)
    if latents.dtype != torch.float32 or not latents.is_contiguous():
        raise ValueError("latents must be contiguous fp32")
    if coef.dtype != torch.float32 or not coef.is_contiguous():
        raise ValueError("euler_ancestral_cfg_step: coef must be a contiguous fp32 buffer")
    ncfg, body = _pag_split("euler_ancestral_cfg_step", coef, pag_n, ncfg)
    per = EULER_A_ROW + latents.numel()
    if body.numel() == 0 or body.numel() % per:
        raise ValueError(f"euler_ancestral_cfg_step: coef holds {body.numel()} floats, not a multiple of "
                         f"{EULER_A_ROW} + {latents.numel()} (rows, then one noise slab per row)")
    _pag_rows("euler_ancestral_cfg_step", body.numel() // per, pag_n)
    B, Cc, Fr, H, W = latents.shape
    check(lib().vd_euler_cfg_step(_p(eps), eps.stride(0), ncfg | STEP_ANCESTRAL, guidance, _p(latents), B, Cc, Fr,
                                  H, W, _p(coef), body.numel() // per, _p(step_idx), _p(x0_out), _p(next_in),
                                  next_in.shape[1] if next_in is not None else 0, _stream()),
          "vd_euler_cfg_step (VD_STEP_ANCESTRAL)")


SCHED_STEP = {"ddim": ddim_cfg_step, "euler": euler_cfg_step, "lcm": lcm_cfg_step, "dpm": dpm_cfg_step,
              "unipc": unipc_cfg_step, "euler_a": euler_ancestral_cfg_step}


def step_advance(step_idx):
    _dev(step_idx)
    check(lib().vd_step_advance(_p(step_idx), _stream()), "vd_step_advance")


def block_transpose(src, nb, na, nc, out=None):
    """dst[(a*nb + b)*nc + c] = src[(b*na + a)*nc + c] over bf16 rows."""
    _dev(src, out)
    width = src.shape[1]
    if out is None:
        out = torch.empty_like(src)
    check(lib().vd_block_transpose(_p(src), _p(out), nb, na, nc, width, _stream()), "vd_block_transpose")
    return out


# ---------------------------------------------------------------- module-level path (rows.hip)
def rows_add(x, y, y_div=1, y_period=None, out=None):
    """out[r] = (x[r] if x is not None else 0) + y[(r // y_div) % y_period]: bf16 rows x, y bf16 or
    fp32 rows.  `out` may be a column slice of a wider buffer (channel concat)."""
    _dev(x, y, out)
    rows = out.shape[0] if out is not None else x.shape[0]
    C = y.shape[1] if x is None else x.shape[1]
    if out is None:
        out = torch.empty(rows, C, device=y.device, dtype=BF16)
    y_f32 = y.dtype == torch.float32
    period = y.shape[0] if y_period is None else y_period
    check(lib().vd_rows_eltwise(0, _p(x), _rows(x) if x is not None else 0, _p(y), _rows(y, y.dtype), int(y_f32),
                                y_div, period, rows, C, _p(out), _rows(out), _stream()), "vd_rows_eltwise(add)")
    return out


def silu_rows(x, out=None):
    _dev(x, out)
    if out is None:
        out = torch.empty_like(x)
    check(lib().vd_rows_eltwise(1, _p(x), _rows(x), None, 0, 0, 1, 1, x.shape[0], x.shape[1], _p(out),
                                _rows(out), _stream()), "vd_rows_eltwise(silu)")
    return out


ROWS_FREEU_FILTER, ROWS_SCALE = 2, 3  # VD_ROWS_FREEU_FILTER, VD_ROWS_SCALE


def _dev_scalar(t, what):
    """One fp32 on the device: the operand ops 2 and 3 of vd_rows_eltwise read inside the launch."""
    if t.dtype != torch.float32 or t.numel() != 1:
        raise ValueError(f"{what}: expected one fp32 element on the device, got {t.dtype} x {t.numel()}")


def freeu_filter(x, n_img, h, w, s_dev, out=None):
    """diffusers' fourier_filter(x, threshold=1, scale=s) (FreeU) on the bf16 NHWC rows of n_img
    h x w images, s = s_dev[0] read on the device; `out` may be a column slice, never x itself."""
    _dev(x, s_dev, out)
    _dev_scalar(s_dev, "freeu_filter s_dev")
    if x.shape[0] != n_img * h * w:
        raise ValueError(f"freeu_filter: {x.shape[0]} rows are not {n_img} images of {h} x {w}")
    if out is None:
        out = torch.empty(x.shape[0], x.shape[1], device=x.device, dtype=BF16)
    check(lib().vd_rows_eltwise(ROWS_FREEU_FILTER, _p(x), _rows(x), _p(s_dev), 0, 1, w, h, x.shape[0], x.shape[1],
                                _p(out), _rows(out), _stream()), "vd_rows_eltwise(freeu_filter)")
    return out


def scale_rows_(x_slice, g_dev):
    """x_slice *= g_dev[0] in place over bf16 rows (a column slice moves only its own bytes)."""
    _dev(x_slice, g_dev)
    _dev_scalar(g_dev, "scale_rows_ g_dev")
    check(lib().vd_rows_eltwise(ROWS_SCALE, _p(x_slice), _rows(x_slice), _p(g_dev), 0, 1, 1, 1, x_slice.shape[0],
                                x_slice.shape[1], _p(x_slice), _rows(x_slice), _stream()), "vd_rows_eltwise(scale)")
    return x_slice


ROWS_WIN_GATHER, ROWS_WIN_MERGE = 4, 5  # VD_ROWS_WIN_GATHER, VD_ROWS_WIN_MERGE
ROWS_WIN_STRIDE_SHIFT = 8               # VD_ROWS_WIN_STRIDE(s) = s << 8


def window_starts(F, L, s):
    """FreeNoise's windows over F frames: the start frame of every window of L frames — the
    regular ones at w * s, then the tail window at F - L when they leave frames uncovered — and
    tail_len, the number of last frames only the tail window holds (0 without one)."""
    if not (1 <= s <= L <= F):
        raise ValueError(f"windows need 1 <= stride <= context_length <= frames, got {s}, {L}, {F}")
    starts = list(range(0, F - L + 1, s))
    tail_len = F - (starts[-1] + L)
    if tail_len:
        starts.append(F - L)
    return starts, tail_len


def window_gather(x, B, F, hw, L, s, out=None):
    """The rows (b, f, p) of B videos of F frames -> the rows (b * nW + w, j, p) of their
    window_starts(F, L, s) windows of L frames (vd_rows_eltwise op 4, a copy).  x may have a row
    stride above its width; `out` may be a column slice, never x itself."""
    _dev(x, out)
    if x.shape[0] != B * F * hw:
        raise ValueError(f"window_gather: {x.shape[0]} rows are not {B} videos of {F} frames x {hw} positions")
    nW = len(window_starts(F, L, s)[0])
    if out is None:
        out = torch.empty(B * nW * L * hw, x.shape[1], device=x.device, dtype=BF16)
    if out.shape[0] != B * nW * L * hw:
        raise ValueError(f"window_gather: out holds {out.shape[0]} rows, the {nW} windows need {B * nW * L * hw}")
    check(lib().vd_rows_eltwise(ROWS_WIN_GATHER | (s << ROWS_WIN_STRIDE_SHIFT), _p(x), _rows(x), None, L, 0, hw, F,
                                x.shape[0], x.shape[1], _p(out), _rows(out), _stream()),
          "vd_rows_eltwise(window_gather)")
    return out


def window_merge(xw, wt_dev, B, F, hw, L, s, out=None):
    """window_gather's inverse with weights (vd_rows_eltwise op 5): frame f becomes the mean of
    the regular windows that hold it, weighted by wt_dev[frame in window] (L positive fp32 on the
    device, read inside the launch), summed in fp32 in ascending window order; the frames only
    the tail window holds take its value."""
    _dev(xw, wt_dev, out)
    if wt_dev.dtype != torch.float32 or wt_dev.dim() != 1 or wt_dev.numel() != L or not wt_dev.is_contiguous():
        raise ValueError(f"window_merge wt_dev: expected {L} contiguous fp32 weights on the device, got "
                         f"{wt_dev.dtype} x {tuple(wt_dev.shape)}")
    nW = len(window_starts(F, L, s)[0])
    if xw.shape[0] != B * nW * L * hw:
        raise ValueError(f"window_merge: {xw.shape[0]} rows are not {B} x {nW} windows of {L} frames x {hw} positions")
    if out is None:
        out = torch.empty(B * F * hw, xw.shape[1], device=xw.device, dtype=BF16)
    if out.shape[0] != B * F * hw:
        raise ValueError(f"window_merge: out holds {out.shape[0]} rows, {B} videos of {F} frames need {B * F * hw}")
    check(lib().vd_rows_eltwise(ROWS_WIN_MERGE | (s << ROWS_WIN_STRIDE_SHIFT), _p(xw), _rows(xw), _p(wt_dev), L, 1,
                                hw, F, out.shape[0], xw.shape[1], _p(out), _rows(out), _stream()),
          "vd_rows_eltwise(window_merge)")
    return out


ROWS_CTRL_ADD = 7            # VD_ROWS_CTRL_ADD
ROWS_CTRL_COL_SHIFT = 8      # VD_ROWS_CTRL_COL(i) = i << 8
CTRL_HEADER = 4              # floats before the table: word 0 the int32 step index, 1..3 unused
CTRL_MAX_COLS = 64


def ctrl_block(table, device=None):
    """The control block of vd_rows_eltwise op 7 for a [steps][cols] scale table -> (block,
    step_idx): one fp32 device buffer of CTRL_HEADER + steps * cols floats, the table behind the
    header, and step_idx, an int32 view of the header's first word (zero).  The denoising loop
    uses that view as its device step counter, so the op needs no pointer of its own for it."""
    tab = torch.as_tensor(table, dtype=torch.float32)
    if tab.dim() != 2 or tab.shape[0] < 1 or not 1 <= tab.shape[1] <= CTRL_MAX_COLS:
        raise ValueError(f"ctrl_block: a [steps >= 1][1..{CTRL_MAX_COLS}] table, got {tuple(tab.shape)}")
    device = tab.device if device is None else torch.device(device)
    if device.type != "cuda":
        raise ValueError("vdiff ops run on the GPU only (ctrl_block on a CPU device); no CPU fallback")
    block = torch.zeros(CTRL_HEADER + tab.numel(), device=device, dtype=torch.float32)
    block[CTRL_HEADER:].view(tab.shape).copy_(tab)
    return block, block[:1].view(torch.int32)


def ctrl_table(block, cols):
    """The [steps][cols] table view of a ctrl_block buffer."""
    return block[CTRL_HEADER:].view(-1, cols)


def ctrl_add_(acc, res, block, col, cols=None):
    """acc += s * res in place over bf16 rows (vd_rows_eltwise op 7), s = table[clamp(step)][col]
    of `block` (ctrl_block), step the block's first word: all read on the device inside the
    launch.  acc may be a row or column slice of a wider buffer.  cols: the table's row length
    (default: the whole table is one row)."""
    _dev(acc, res, block)
    if block.dtype != torch.float32 or block.dim() != 1 or not block.is_contiguous() or block.numel() <= CTRL_HEADER:
        raise ValueError("ctrl_add_: block must be a contiguous 1-D fp32 buffer from ctrl_block")
    cols = block.numel() - CTRL_HEADER if cols is None else int(cols)
    if cols < 1 or (block.numel() - CTRL_HEADER) % cols:
        raise ValueError(f"ctrl_add_: the block's {block.numel() - CTRL_HEADER} table floats are not rows of {cols}")
    if tuple(acc.shape) != tuple(res.shape):
        raise ValueError(f"ctrl_add_: acc {tuple(acc.shape)} and res {tuple(res.shape)} differ")
    if not 0 <= col < cols:
        raise ValueError(f"ctrl_add_: column {col} outside the table's {cols}")
    check(lib().vd_rows_eltwise(ROWS_CTRL_ADD | (col << ROWS_CTRL_COL_SHIFT), _p(res), _rows(res), _p(block), cols, 1,
                                1, (block.numel() - CTRL_HEADER) // cols, acc.shape[0], acc.shape[1], _p(acc),
                                _rows(acc), _stream()), "vd_rows_eltwise(ctrl_add)")
    return acc


ROWS_SPARSE_COND = 8         # VD_ROWS_SPARSE_COND
ROWS_SPARSE_CH_SHIFT = 8     # VD_ROWS_SPARSE_CH(cc) = cc << 8, cc in 1..7
SPARSE_MAX = 256             # the longest F and K


def sparse_frame_indices(idx, F):
    """controlnet_frame_indices the Python way: negative indices count from the end, anything
    outside [-F, F) is an IndexError (torch indexing's), before any device work."""
    idx = idx.tolist() if torch.is_tensor(idx) else list(idx)
    out = []
    for i in idx:
        if isinstance(i, bool) or int(i) != i:
            raise TypeError(f"sparse_cond: frame index {i!r} is not an integer")
        i = int(i)
        if not -F <= i < F:
            raise IndexError(f"sparse_cond: frame index {i} is out of bounds for {F} frames")
        out.append(i + F if i < 0 else i)
    return out


def sparse_cond(key_rows, idx, B, F, hw, cc, out=None):
    """SparseCtrl's condition rows (vd_rows_eltwise op 8): key_rows holds K = len(idx) key frames
    per video as bf16 NHWC rows (b, k, p) of >= 8 columns, of which the first cc are the condition;
    the result is the [B * F * hw, 8] packed rows of B videos of F frames: frame idx[k] takes key
    frame k (the last k that names a frame wins) with 1.0 in column cc, every other frame is zero.
    One launch writes every element: no zero fill, no indexed copies."""
    frames = sparse_frame_indices(idx, F)
    K = len(frames)
    if not 1 <= K <= SPARSE_MAX or not 1 <= F <= SPARSE_MAX:
        raise ValueError(f"sparse_cond: 1..{SPARSE_MAX} key frames and frames, got {K} and {F}")
    if not 1 <= cc <= 7:
        raise ValueError(f"sparse_cond: 1..7 condition channels, got {cc}")
    _dev(key_rows, out)
    if key_rows.shape[0] != B * K * hw or key_rows.shape[1] != 8:
        raise ValueError(f"sparse_cond: key rows of shape {tuple(key_rows.shape)} are not {B} videos x {K} key frames "
                         f"x {hw} positions of 8 columns")
    if out is None:
        out = torch.empty(B * F * hw, 8, device=key_rows.device, dtype=BF16)
    if tuple(out.shape) != (B * F * hw, 8):
        raise ValueError(f"sparse_cond: out of shape {tuple(out.shape)}, {B} videos of {F} frames need "
                         f"{(B * F * hw, 8)}")
    idx_dev = torch.tensor(frames, dtype=torch.int32, device=key_rows.device)
    check(lib().vd_rows_eltwise(ROWS_SPARSE_COND | (cc << ROWS_SPARSE_CH_SHIFT), _p(key_rows), _rows(key_rows),
                                _p(idx_dev), K, 1, hw, F, out.shape[0], 8, _p(out), _rows(out), _stream()),
          "vd_rows_eltwise(sparse_cond)")
    return out


ROWS_PROMPT_LERP = 9         # VD_ROWS_PROMPT_LERP
PROMPT_MAX = 256             # the longest F and K


def prompt_frame_indices(idx, F):
    """The key frames of a prompt travel: ints, strictly increasing, the first 0, the last F - 1
    (encode_prompt_free_noise appends the last prompt there); refused before any device work."""
    idx = idx.tolist() if torch.is_tensor(idx) else list(idx)
    for i in idx:
        if isinstance(i, bool) or not isinstance(i, int):
            raise TypeError(f"prompt_lerp: frame index {i!r} is not an integer")
    if not 1 <= len(idx) <= PROMPT_MAX or not 1 <= F <= PROMPT_MAX:
        raise ValueError(f"prompt_lerp: 1..{PROMPT_MAX} key prompts and frames, got {len(idx)} and {F}")
    if any(b <= a for a, b in zip(idx, idx[1:])):
        raise ValueError(f"prompt_lerp: frame indices {idx} are not strictly increasing")
    if idx[0] != 0:
        raise ValueError(f"prompt_lerp: the first frame index must be 0, got {idx[0]}")
    if idx[-1] != F - 1:
        raise ValueError(f"prompt_lerp: the last frame index must be {F - 1} (the last of {F} frames), got {idx[-1]}")
    return idx


def prompt_lerp(key_rows, idx, B, F, L, out=None):
    """FreeNoise prompt travel (vd_rows_eltwise op 9): key_rows holds K = len(idx) key prompts per
    video as bf16 rows (b, k, token) of C columns, L tokens each; the result is the [B * F * L, C]
    per-frame rows (b, f, token): frame idx[k] is key k bit for bit, a frame between two keys their
    linear interpolation, w = (f - idx[k]) / (idx[k + 1] - idx[k]), one rounding to bf16.  One
    launch writes every element; out may be a column slice of a wider buffer."""
    frames = prompt_frame_indices(idx, F)
    K = len(frames)
    if L < 1 or B < 1 or key_rows.dim() != 2 or key_rows.shape[0] != B * K * L or key_rows.shape[1] % 8:
        raise ValueError(f"prompt_lerp: key rows of shape {tuple(key_rows.shape)} are not {B} videos x {K} key prompts "
                         f"x {L} tokens of C % 8 == 0 columns")
    _dev(key_rows, out)
    C = key_rows.shape[1]
    if out is None:
        out = torch.empty(B * F * L, C, device=key_rows.device, dtype=BF16)
    if tuple(out.shape) != (B * F * L, C):
        raise ValueError(f"prompt_lerp: out of shape {tuple(out.shape)}, {B} videos of {F} frames need "
                         f"{(B * F * L, C)}")
    idx_dev = torch.tensor(frames, dtype=torch.int32, device=key_rows.device)
    check(lib().vd_rows_eltwise(ROWS_PROMPT_LERP, _p(key_rows), _rows(key_rows), _p(idx_dev), K, 1, L, F,
                                out.shape[0], C, _p(out), _rows(out), _stream()), "vd_rows_eltwise(prompt_lerp)")
    return out


ROWS_SPECTRAL = 6            # VD_ROWS_SPECTRAL
ROWS_SPEC_PASS_SHIFT = 8     # VD_ROWS_SPEC_PASS(p) = p << 8, p in 1..5
SPECTRAL_MAX = 256           # VD_SPECTRAL_MAX: the longest F, H or W
FREE_INIT_METHODS = ("butterworth", "gaussian", "ideal")


def free_init_mask(F, H, W, method, order, spatial_stop_frequency, temporal_stop_frequency):
    """diffusers' FreeInitMixin._get_free_init_freq_filter over (F, H, W) in fp64, indexed in
    fftshift-ed order (centred at N / 2): all zeros when a stop frequency is 0."""
    ds, dt = float(spatial_stop_frequency), float(temporal_stop_frequency)
    if method not in FREE_INIT_METHODS:
        raise NotImplementedError("`filter_type` must be one of gaussian, butterworth or ideal")
    if ds == 0 or dt == 0:
        return torch.zeros(F, H, W, dtype=torch.float64)
    t = torch.arange(F, dtype=torch.float64)[:, None, None]
    h = torch.arange(H, dtype=torch.float64)[None, :, None]
    w = torch.arange(W, dtype=torch.float64)[None, None, :]
    d2 = ((ds / dt) * (2 * t / F - 1)) ** 2 + (2 * h / H - 1) ** 2 + (2 * w / W - 1) ** 2
    if method == "butterworth":
        return 1 / (1 + (d2 / ds ** 2) ** order)
    if method == "gaussian":
        return torch.exp(-1 / (2 * ds ** 2) * d2)
    return (d2 <= ds * 2).to(torch.float64)


def free_init_table(F, H, W, method="butterworth", order=4, spatial_stop_frequency=0.25,
                    temporal_stop_frequency=0.25, device=None, dtype=torch.float32):
    """The operand of free_init_filter: diffusers' mask in fp64, ifftshift-ed to DFT index order,
    made Hermitian-even, M_s(k) = (M(k) + M(-k mod N)) / 2 (what taking the real part of the
    inverse transform amounts to; M is already even when F, H and W are all even), cut to the half
    spectrum [F][H][W // 2 + 1] and rounded once to fp32 (dtype=torch.float64 keeps the unrounded
    table, for checking the identity).  Pure torch: runs on the CPU too."""
    m = free_init_mask(F, H, W, method, order, spatial_stop_frequency, temporal_stop_frequency)
    m = torch.fft.ifftshift(m, dim=(0, 1, 2))
    mirror = m.flip(0, 1, 2).roll((1, 1, 1), (0, 1, 2))  # M(-k mod N)
    m = (m + mirror) / 2
    return m[:, :, :W // 2 + 1].contiguous().to(dtype).to(device or "cpu")


def free_init_filter(z, noise, table, out=None, scratch=None):
    """FreeInit's frequency mix (diffusers' _apply_freq_filter) of fp32 (..., F, H, W) tensors: the
    low spatio-temporal frequencies of z, the high ones of noise, the leading dims being the
    volumes; out = noise + Re(IDFT3(table * DFT3(z - noise))) in five launches of vd_rows_eltwise
    op 6 on the current stream.  table: free_init_table(F, H, W, ...) on the device.  scratch: fp32,
    n_vol * F * H * 2 * (W // 2 + 1) elements, allocated when None; what it holds does not matter."""
    _dev(z, noise, table, out, scratch)
    if z.dim() < 3:
        raise ValueError(f"free_init_filter z: expected (..., F, H, W), got shape {tuple(z.shape)}")
    F, H, W = z.shape[-3:]
    Wh = W // 2 + 1
    for name, t in (("z", z), ("noise", noise), ("table", table)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"free_init_filter {name}: expected a contiguous fp32 tensor, got {t.dtype}, "
                             f"strides {t.stride()}")
    if noise.shape != z.shape:
        raise ValueError(f"free_init_filter noise: shape {tuple(noise.shape)} is not z's {tuple(z.shape)}")
    if tuple(table.shape) != (F, H, Wh):
        raise ValueError(f"free_init_filter table: shape {tuple(table.shape)} is not ({F}, {H}, {Wh}) "
                         "(ops.free_init_table)")
    if max(F, H, W) > SPECTRAL_MAX:
        raise ValueError(f"free_init_filter: F, H, W = {F}, {H}, {W} exceed the kernel's limit of {SPECTRAL_MAX} each")
    rows = z.numel() // W
    if rows == 0:
        raise ValueError("free_init_filter z: empty tensor")
    if out is None:
        out = torch.empty_like(z)
    if out.dtype != torch.float32 or out.shape != z.shape or not out.is_contiguous():
        raise ValueError(f"free_init_filter out: expected a contiguous fp32 tensor of shape {tuple(z.shape)}, got "
                         f"{out.dtype} {tuple(out.shape)}")
    if scratch is None:
        scratch = torch.empty(rows * 2 * Wh, device=z.device, dtype=torch.float32)
    if scratch.dtype != torch.float32 or scratch.numel() < rows * 2 * Wh or not scratch.is_contiguous():
        raise ValueError(f"free_init_filter scratch: expected {rows * 2 * Wh} contiguous fp32 elements, got "
                         f"{scratch.dtype} x {scratch.numel()}")
    for name, t in (("z", z), ("noise", noise), ("table", table), ("out", out), ("scratch", scratch)):
        if t.data_ptr() % 16:
            raise ValueError(f"free_init_filter {name}: the base is not 16-byte aligned (a view into a larger "
                             "tensor? pass a clone)")
    if out.data_ptr() in (z.data_ptr(), noise.data_ptr()):
        raise ValueError("free_init_filter out: must not be z or noise (the last pass reads noise as it writes)")
    fn, st, S = lib().vd_rows_eltwise, _stream(), _p(scratch)

    def op(p):
        return ROWS_SPECTRAL | (p << ROWS_SPEC_PASS_SHIFT)

    check(fn(op(1), _p(z), W, _p(noise), W, 1, H, F, rows, W, S, 2 * Wh, st), "vd_rows_eltwise(spectral 1)")
    check(fn(op(2), S, 2 * Wh, None, 0, 0, H, F, rows, W, S, 2 * Wh, st), "vd_rows_eltwise(spectral 2)")
    check(fn(op(3), S, 2 * Wh, _p(table), Wh, 1, H, F, rows, W, S, 2 * Wh, st), "vd_rows_eltwise(spectral 3)")
    check(fn(op(4), S, 2 * Wh, None, 0, 0, H, F, rows, W, S, 2 * Wh, st), "vd_rows_eltwise(spectral 4)")
    check(fn(op(5), S, 2 * Wh, _p(noise), W, 1, H, F, rows, W, _p(out), W, st), "vd_rows_eltwise(spectral 5)")
    return out


def upsample2x_rows(x, n_img, h, w, out=None):
    _dev(x, out)
    if out is None:
        out = torch.empty(n_img * 4 * h * w, x.shape[1], device=x.device, dtype=BF16)
    check(lib().vd_upsample_nearest2x(_p(x), _rows(x), n_img, h, w, x.shape[1], _p(out), _rows(out), _stream()),
          "vd_upsample_nearest2x")
    return out


# ---------------------------------------------------------------- DiT (§8f rank 3)
def patchify(lat, p, kpad, dup=1, in_div=1.0, out=None):
    """latents fp32 (B,C,F,H,W) -> bf16 token rows [(b,f,hp,wp)][kpad] (x dup for CFG)."""
    _dev(lat, out)
    if lat.dtype != torch.float32 or not lat.is_contiguous():
        raise ValueError("patchify expects contiguous fp32 latents")
    B, Cc, F, H, W = lat.shape
    rows = B * F * (H // p) * (W // p)
    if out is None:
        out = torch.empty(dup * rows, kpad, device=lat.device, dtype=BF16)
    check(lib().vd_patchify(_p(lat), B, Cc, F, H, W, p, dup, in_div, _p(out), kpad, _stream()), "vd_patchify")
    return out


def unpatchify(src, n_img, H, W, p, Cc, out=None):
    """fp32 token rows [(n,hp,wp)][(ph,pw,c)] -> fp32 NHWC pixel rows [(n,h,w)][c]."""
    _dev(src, out)
    if src.dtype != torch.float32:
        raise ValueError("unpatchify expects fp32 rows")
    if out is None:
        out = torch.empty(n_img * H * W, Cc, device=src.device, dtype=torch.float32)
    check(lib().vd_unpatchify(_p(src), _rows(src, torch.float32), n_img, H, W, p, Cc, _p(out), _stream()),
          "vd_unpatchify")
    return out


def rope_qk(x, ncols, d, mode, F, Hp, Wp, theta=10000.0):
    """In-place rotary embedding on columns [0, ncols) of bf16 token rows x."""
    _dev(x)
    check(lib().vd_rope_qk(_p(x), _rows(x), x.shape[0], ncols, d, mode, F, Hp, Wp, theta, _stream()),
          "vd_rope_qk")
    return x


def res_ln_mod(x, *, y=None, gate=None, shift=None, scale=None, rows_per_b=None, x_out=None,
               eps=1e-6, out=None):
    """h = LN(x + gate*y) * (1 + scale) + shift per row group b = row // rows_per_b;
    x_out (may be x) receives x + gate*y.  gate/shift/scale: fp32 [B, >= C] row views."""
    _dev(x, y, gate, shift, scale, x_out, out)
    rows, Cc = x.shape
    mods = [t for t in (gate, shift, scale) if t is not None]
    ld_mod = mods[0].stride(0) if mods else 0
    for t in mods:
        if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) != ld_mod:
            raise ValueError("gate/shift/scale must be fp32 row views sharing one row stride")
    if out is None:
        out = torch.empty(rows, Cc, device=x.device, dtype=BF16)
    check(lib().vd_res_ln_mod(_p(x), _rows(x), _p(y), _rows(y) if y is not None else 0, _p(gate), _p(shift),
                              _p(scale), ld_mod, rows_per_b or rows, _p(x_out),
                              _rows(x_out) if x_out is not None else 0, _p(out), _rows(out), rows, Cc, eps,
                              _stream()), "vd_res_ln_mod")
    return out


def attention_fp8_quant(q, k, v, batch, heads, sq, skv, d=64, rope=None, q_scale=1.0):
    """bf16 q/k/v row views -> the fp8 operands of vd_attention_fp8 (a dict of buffers).
    rope=(Hp, Wp, theta): apply the spatial 2-D RoPE (rope_qk mode 0) to q and k inside the
    quantization pass (vd_attention_fp8_quant_rope); q and k are read un-rotated.
    q_scale: q is multiplied by it before quantization (attention_fp8 folds the softmax scale x
    log2 e there); ws["q_scale"] records it."""
    _dev(q, k, v)
    dev = q.device
    ld8 = (heads * d + 15) // 16 * 16
    u8 = torch.uint8
    ws = {"q8": torch.empty(batch * sq, ld8, device=dev, dtype=u8),
          "k8": torch.empty(batch * skv, ld8, device=dev, dtype=u8),
          "vt8": torch.empty(batch * heads * d, skv, device=dev, dtype=u8),
          "qs": torch.empty(batch * sq, heads, device=dev, dtype=u8),
          "ks": torch.empty(batch * skv, heads, device=dev, dtype=u8),
          "vs": torch.empty(batch * heads, max(1, skv // 64), device=dev, dtype=u8),
          "ld8": ld8, "batch": batch, "heads": heads, "sq": sq, "skv": skv, "d": d, "q_scale": float(q_scale)}
    if rope is not None:
        if sq != skv:
            raise ValueError("fused RoPE quantization needs sq == skv (self-attention)")
        Hp, Wp, theta = rope
        check(lib().vd_attention_fp8_quant_rope(
            _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), batch, heads, sq, d, Hp, Wp, theta,
            _p(ws["q8"]), _p(ws["k8"]), ld8, _p(ws["vt8"]), _p(ws["qs"]), _p(ws["ks"]), _p(ws["vs"]), float(q_scale),
            _stream()), "vd_attention_fp8_quant_rope")
        return ws
    check(lib().vd_attention_fp8_quant(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), batch, heads,
                                       sq, skv, d, _p(ws["q8"]), _p(ws["k8"]), ld8, _p(ws["vt8"]), _p(ws["qs"]),
                                       _p(ws["ks"]), _p(ws["vs"]), float(q_scale), _stream()), "vd_attention_fp8_quant")
    return ws


LOG2E = 1.4426950408889634


def attention_fp8_run(ws, out, scale=None):
    """vd_attention_fp8 on operands from attention_fp8_quant.  `scale` multiplies the scores of
    the dequantized q8 (default d^-1/2 / ws["q_scale"]: the softmax scale q_scale did not fold;
    1 / log2 e after attention_fp8's full fold selects the kernel's folded form)."""
    d = ws["d"]
    if scale is None:
        scale = d ** -0.5 / ws["q_scale"]
    check(lib().vd_attention_fp8(_p(ws["q8"]), _p(ws["k8"]), ws["ld8"], _p(ws["qs"]), _p(ws["ks"]), _p(ws["vt8"]),
                                 _p(ws["vs"]), _p(out), out.stride(0), ws["batch"], ws["heads"], ws["sq"], ws["skv"],
                                 d, scale, _stream()), "vd_attention_fp8")
    return out


def attention_fp8(q, k, v, batch, heads, sq, skv, d=64, scale=None, out=None, rope=None):
    """fp8 (e4m3, block-scaled MFMA) self-attention, d = 64: quantize (optionally with the
    spatial RoPE fused, see attention_fp8_quant) with the softmax scale x log2 e folded into q,
    then attend (the kernel's folded form: no per-score multiply)."""
    scale = d ** -0.5 if scale is None else scale
    ws = attention_fp8_quant(q, k, v, batch, heads, sq, skv, d, rope=rope, q_scale=scale * LOG2E)
    if out is None:
        out = torch.empty(batch * sq, heads * d, device=q.device, dtype=BF16)
    _dev(out)
    return attention_fp8_run(ws, out, scale=1.0 / LOG2E)
