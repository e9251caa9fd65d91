"""The GEMM plan's decision table (vd_gemm_plan / vd_gemm_ws_bytes are host-only: no GPU):

    python tests/golden/make_plan_golden.py            # writes tests/golden/gemm_plan.npz
    python tests/golden/make_plan_golden.py --dump     # one readable line per descriptor, to stdout

grid() enumerates a fixed list of vd_gemm_desc: the dense shapes crossed with the activation,
every forced path and plan_m, each alone and with one optional feature or one alignment case,
then the 2-D and temporal convs.  For each descriptor the table records vd_gemm_plan's return
code, kernel and split and vd_gemm_ws_bytes, in grid order.  tests/test_gemm_plan.py replays the
grid against the built library and compares exactly: the plan fixes the kernel, the N tile and
split-K, and through them the summation order the bit-exact sharded tests rely on.  Regenerate the
table only with a change that means to move a decision; --dump of two trees shows which.
Without a device the library plans for 256 CUs (the MI355X), which is what the table holds.
"""
import ctypes
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "video-diffusion-experiments_amd")]

OUT = HERE / "gemm_plan.npz"
PTR, PTR8 = 256, 264  # dummy operand addresses: 16-byte aligned, and 8- but not 16-byte aligned
GEGLU = 2

DENSE_M = (2, 16, 17, 63, 64, 255, 256, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 147456)
DENSE_N = (4, 32, 48, 64, 320, 640, 960, 1152, 1280, 1920, 2560, 3840, 5120, 10240)
DENSE_K = (320, 328, 352, 640, 1152, 1280, 2560, 2880, 5760, 11520)
PATHS = (0, 1, 2, 3, 5, 6, 8, 9)
PLAN_M = (0, 8192)
# one optional feature, or one alignment case, at a time on every dense shape
FEATURES = ("plain", "res", "rowbias", "ln_out", "ln_fold", "rmap", "rmap_res", "concat", "out_f32",
            "out_al8", "res_al8", "ldc4", "ld_res4")

CONV_IMAGES = (1, 2, 4, 32)
CONV_SIDE = (8, 16, 32, 64)
CONV_CIN = (8, 32, 320, 640, 1280, 2560)
CONV_COUT = (4, 320, 640, 1280)
CONV_FORM = ("s1", "s2", "up")  # stride 1, stride 2, nearest-2x upsample in the loader


def _mult4_not8(n):
    return (n + 7) // 8 * 8 + 4


def _set_feature(d, feat, M, K, nout):
    if feat in ("res", "rmap_res", "res_al8", "ld_res4"):
        d.res, d.ld_res = PTR, nout
    if feat == "rowbias":
        d.rowbias, d.ld_rb, d.rb_div = PTR, nout, 1
    elif feat == "ln_out":
        d.ln_out, d.ld_ln, d.ln_gamma, d.ln_beta, d.ln_eps = PTR, nout, PTR, PTR, 1e-5
    elif feat == "ln_fold":
        d.ln_fold_s, d.ln_fold_eps = PTR, 1e-5
    elif feat in ("rmap", "rmap_res"):
        d.rmap_n1, d.rmap_n2, d.rmap_inner = 2, 1, max(M // 2, 1)
    elif feat == "concat":
        d.a1, d.lda0, d.lda1, d.k0 = PTR, K // 2, K // 2, K // 2
    elif feat == "out_f32":
        d.out_f32 = 1
    elif feat == "out_al8":
        d.out = PTR8
    elif feat == "res_al8":
        d.res = PTR8
    elif feat == "ldc4":
        d.ldc = _mult4_not8(nout)
    elif feat == "ld_res4":
        d.ld_res = _mult4_not8(nout)


def _paths(d):
    for plan_m in PLAN_M:
        d.plan_m = plan_m
        for path in PATHS:
            d.path = path
            yield d


def grid():
    """Yields the descriptors in the table's order.  The same object is mutated and yielded again
    where only path / plan_m change: read it before advancing."""
    from vdiff import _lib as L

    for M in DENSE_M:
        for N in DENSE_N:
            for K in DENSE_K:
                for act in (0, GEGLU):
                    nout = N // 2 if act == GEGLU else N
                    for feat in FEATURES:
                        d = L.GemmDesc(a0=PTR, lda0=K, k0=K, a_mode=0, w=PTR, ldw=K, M=M, N=N, K=K, bias=PTR,
                                       act=act, out=PTR, ldc=nout)
                        _set_feature(d, feat, M, K, nout)
                        yield from _paths(d)
    # 2-D 3x3 convs
    for n_img in CONV_IMAGES:
        for side in CONV_SIDE:
            for cin in CONV_CIN:
                for cout in CONV_COUT:
                    for form in CONV_FORM:
                        for concat in (False, True):
                            ho = side * 2 if form == "up" else (side - 1) // 2 + 1 if form == "s2" else side
                            c0 = cin // 2 if concat else cin
                            d = L.GemmDesc(a0=PTR, lda0=c0, k0=c0, a1=PTR if concat else None, lda1=c0 if concat else 0,
                                           a_mode=1, n_img=n_img, h_in=side, w_in=side, h_out=ho, w_out=ho,
                                           stride=2 if form == "s2" else 1, upsample=int(form == "up"), w=PTR,
                                           ldw=9 * cin, M=n_img * ho * ho, N=cout, K=9 * cin, bias=PTR, out=PTR, ldc=cout)
                            yield from _paths(d)
    # temporal convs: kt = 3 with ks = 3 (full 3-D) and ks = 1 ((2+1)D); the batch's images are the
    # frames of one video (two videos of 16 at 32), unhaloed and with a one-frame halo each side
    for n_img in CONV_IMAGES:
        frames = min(n_img, 16)
        for side in CONV_SIDE:
            for cin in CONV_CIN:
                for cout in CONV_COUT:
                    for ks in (3, 1):
                        for halo in (0, 1):
                            for concat in (False, True):
                                c0 = cin // 2 if concat else cin
                                K = 3 * ks * ks * cin
                                d = L.GemmDesc(a0=PTR, lda0=c0, k0=c0, a1=PTR if concat else None,
                                               lda1=c0 if concat else 0, a_mode=1, n_img=n_img, h_in=side, w_in=side,
                                               h_out=side, w_out=side, stride=1, upsample=0, w=PTR, ldw=K,
                                               M=n_img * side * side, N=cout, K=K, bias=PTR, out=PTR, ldc=cout,
                                               kt=3, ks=ks, frames_in=frames + 2 * halo, frames_out=frames, t_off=halo)
                                yield from _paths(d)


def describe(d):
    """One line that identifies a descriptor of the grid (every field the plan reads)."""
    s = f"M={d.M} N={d.N} K={d.K} act={d.act} path={d.path} plan_m={d.plan_m}"
    if d.a_mode:
        s += (f" conv n_img={d.n_img} in={d.h_in}x{d.w_in} out={d.h_out}x{d.w_out} stride={d.stride} up={d.upsample}"
              f" kt={d.kt} ks={d.ks} frames={d.frames_in}/{d.frames_out} t_off={d.t_off}")
    if d.a1:
        s += f" a1 k0={d.k0}"
    for name in ("res", "rowbias", "ln_out", "ln_fold_s"):
        if getattr(d, name):
            s += f" {name}@{getattr(d, name) % 16}"
    if d.res:
        s += f" ld_res={d.ld_res}"
    if d.rmap_inner:
        s += f" rmap={d.rmap_n1},{d.rmap_n2},{d.rmap_inner}"
    return s + f" out@{d.out % 16} ldc={d.ldc} out_f32={d.out_f32}"


def evaluate(on_row=None):
    """Runs the grid through the library: (rc, kernel, split, ws_bytes) arrays in grid order.
    on_row(i, d, rc, kernel, split, ws) is called per descriptor while d still holds it."""
    from vdiff import _lib as L

    lib = L.lib()
    plan, ws_bytes = lib.vd_gemm_plan, lib.vd_gemm_ws_bytes
    k, sp = ctypes.c_int32(), ctypes.c_int32()
    pk, psp = ctypes.byref(k), ctypes.byref(sp)
    rc_l, k_l, sp_l, ws_l = [], [], [], []
    for i, d in enumerate(grid()):
        k.value = sp.value = -1
        p = ctypes.byref(d)
        rc = plan(p, pk, psp)
        ws = ws_bytes(p)
        rc_l.append(rc)
        k_l.append(k.value)
        sp_l.append(sp.value)
        ws_l.append(ws)
        if on_row:
            on_row(i, d, rc, k.value, sp.value, ws)
    return (np.asarray(rc_l, np.int16), np.asarray(k_l, np.int8), np.asarray(sp_l, np.int8),
            np.asarray(ws_l, np.int64))


def main():
    if "--dump" in sys.argv[1:]:
        evaluate(lambda i, d, rc, k, sp, ws: print(f"{i} {describe(d)} -> rc={rc} kernel={k} split={sp} ws={ws}"))
        return
    rc, k, sp, ws = evaluate()
    np.savez_compressed(OUT, rc=rc, kernel=k, split=sp, ws_bytes=ws)
    print(f"{OUT.name}: {len(k)} descriptors, {OUT.stat().st_size} bytes; kernels "
          f"{sorted(set(k.tolist()))}, splits {sorted(set(sp.tolist()))}")


if __name__ == "__main__":
    main()
