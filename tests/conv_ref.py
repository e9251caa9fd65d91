"""The conv loaders' case matrix (tests/test_conv_matrix_host.py, tests/test_gpu_conv_matrix.py).

Four kernels carry their own copy of the implicit-GEMM loader that turns an output row m into
(image, oh, ow) and walks the taps: gemm_v1.hip, gemm_v2.hip (128-, 160- and 32-column tiles,
and a split-K form), gemm_v5.hip (and its split form) and gemm_v6.hip (unsplit, and with its
in-kernel split reduce).  Every copy owes the same things: a zero halo, the nearest-2x upsample by
>> 1, stride 2, the a0 | a1 channel concat, temporal taps and the halo-frame offset.  This file
holds, for the host test and the GPU test alike:

  CASES            one table: every loader family in every mode it takes, at a geometry where none
                   of its integer arithmetic can hide (below), with the plan control that reaches
                   the family and the (kernel, N tile, K split) the plan must give;
  operands(case)   seeded per case name, CPU: bf16 unit-normal x, bf16 weights of std
                   (taps * Cin)^-0.5, fp32 bias and row bias, bf16 residual;
  reference(...)   fp64 F.conv2d / F.conv3d over those bf16 values, then the epilogue in the order
                   include/vdiff.h documents (+ bias, + rowbias[m / rb_div], act, + res);
  restated(...)    the implicit GEMM said again as an explicit gather (row decode, taps, range
                   check, gather, one matmul per tap) in fp64 plain torch, independent of
                   F.conv*; with fault= it commits exactly one loader mistake (FAULTS);
  tolerance(...)   the existing per-kernel conv bound (test_gpu_memframe.conv_case): rtol 1e-3
                   and atol 1e-4 x max(1, max|ref|) unsplit, 1e-3 x max(1, max|ref|) split;
                   bf16 outputs memframe.close_bf16's two terms.

Geometry.  The base image is 9 x 6: no power of two, h != w, odd height; stride 2 gives 5 x 3,
the upsample 18 x 12.  Image counts put the row count just above the family's minimum and off
every multiple of its tile, so several image seams fall inside every tile and the last tile is
ragged: 5 images (270 rows) for stride 1 on the 256-row kernels, 18 (270 rows) for stride 2,
3 (162 rows) resp. 11 stride-2 images (165 rows) for the unsplit v6 below 256 rows, 2 upsampled
images (432 rows).  "wide" is 2 images of 5 x 96: one image row is longer than v6's 64-row tile.

Channels.  Cin 64 where the family allows; v5 takes Cin 96 (Cin % 64 != 0 is what sends a conv
there); the concat halves are unequal, 128 + 64 (v5: 96 + 32, k0 % 64 != 0), so a split at Cin / 2
or swapped halves cannot pass; "long" is Cin 192 unsplit, three K-tiles per tap; v1 also runs
Cin 8 (its K % 32 != 0 tile).  Cout 128 / 160 / 20 select v2's three N tiles, 72 is v1's and v6's.

Reaching the plans.  split_for() in gemm.hip splits any few-tile shape of 16 or more K-tiles and
none below, so (a) the unsplit long-K plans the full-size product runs are reached with
ops.plan_scaled(mul) (mul the smallest that makes the planned tile count 192, resp. 512 for
forced v6), and (b) a split v2 / v5 needs Cin >= 128 at 3 x 3 taps: the "v2-split" cases use
Cin 128 (18 K-tiles in 2 slices: the slice boundary falls inside a tap), "v5-split" Cin 160.
The kt 3 x ks 1 conv has 3 Cin / 64 K-tiles, so its split form needs Cin 384 — the one case
above Cin 192.  The stride-2 cases carry a row bias beside bias + residual: only where
h_in * w_in != h_out * w_out can a row bias indexed by the input image size be told from a right
one, and v2's 32-column tile runs no other such mode.
"""
from __future__ import annotations

import ctypes
import zlib
from dataclasses import dataclass, replace
from typing import Optional

import torch
import torch.nn.functional as F

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
MAX_ROWS, MAX_CIN = 4000, 192


@dataclass(frozen=True)
class Case:
    name: str
    family: str           # FAMILIES_2D / FAMILIES_3D
    mode: str             # MODES_2D + EXTRA_2D / MODES_3D
    n: int                # 2-D: images; 3-D: videos (B)
    h: int
    w: int
    c0: int
    c1: int
    cout: int
    path: int             # ops.gemm_plan(path=)
    kernel: int           # expected family of vd_gemm_plan
    bn: int               # expected N tile (ntile() below restates the plan's rule)
    split: int            # expected K slices
    mul: int = 1          # ops.plan_scaled(mul)
    stride: int = 1
    up: bool = False
    bias: bool = True
    rowbias: bool = False
    res: bool = False
    out_f32: bool = True
    frames: int = 0       # 3-D: output frames per video (T); 0 = a 2-D conv
    kt: int = 1
    ks: int = 3
    halo: bool = False    # 3-D: frames_in = frames + 2, t_off = 1

    # ---- derived sizes
    @property
    def is3d(self):
        return self.frames > 0

    @property
    def cin(self):
        return self.c0 + self.c1

    @property
    def taps(self):
        return self.kt * self.ks * self.ks

    @property
    def K(self):
        return self.taps * self.cin

    @property
    def frames_in(self):
        return self.frames + 2 if self.halo else self.frames

    @property
    def t_off(self):
        return 1 if self.halo else 0

    @property
    def n_in(self):       # input images
        return self.n * self.frames_in if self.is3d else self.n

    @property
    def n_out(self):      # output images (vd_gemm_desc.n_img)
        return self.n * self.frames if self.is3d else self.n

    @property
    def h_out(self):
        return 2 * self.h if self.up else (self.h - 1) // self.stride + 1

    @property
    def w_out(self):
        return 2 * self.w if self.up else (self.w - 1) // self.stride + 1

    @property
    def M(self):
        return self.n_out * self.h_out * self.w_out

    @property
    def rb_div(self):
        return self.h_out * self.w_out

    @property
    def is_split(self):
        return self.split > 1


FAMILIES_2D = ("v1", "v6", "v6-split", "v2-bn128", "v2-bn160", "v2-bn32", "v2-split", "v5", "v5-split")
MODES_2D = ("s1", "s2", "up", "concat")
FAMILIES_3D = ("v1", "v2-unsplit", "v2-split")
MODES_3D = ("t3s3", "t3s1", "t3s3-halo", "t3s3-s2")
# beside the product: the long-tap walk (Cin 192 unsplit) and the wide image, on these families
EXTRA_2D = {"long": ("v2-bn128", "v6"), "wide": ("v1", "v6", "v6-split", "v2-bn128", "v5")}
# the one case above MAX_CIN (module docstring)
OVER_CIN = ("3d-v2-split-t3s1",)

H, W = 9, 6


def product_2d():
    """The (family, mode) pairs the 2-D table must hold, no more and no fewer."""
    want = {(f, m) for f in FAMILIES_2D for m in MODES_2D if not (f == "v2-bn32" and m in ("up", "concat"))}
    return want | {(f, m) for m, fams in EXTRA_2D.items() for f in fams}


def product_3d():
    return {(f, m) for f in FAMILIES_3D for m in MODES_3D}


def _epi(mode):
    """The epilogue extras of a 2-D mode."""
    if mode in ("s1", "concat", "long", "wide"):   # the resnet's conv1: time_emb_proj broadcast per image
        return dict(rowbias=True)
    if mode == "s2":
        return dict(rowbias=True, res=True)
    return {}


def _cases():
    out = []

    def add2(family, mode, n, c0, c1, cout, path, kernel, bn, split, *, mul=1, h=H, w=W, tag="", **kw):
        geo = dict(stride=2 if mode == "s2" else 1, up=mode == "up")
        out.append(Case(f"{family}-{mode}{tag}", family, mode, n, h, w, c0, c1, cout, path, kernel, bn, split,
                        mul=mul, **geo, **_epi(mode), **kw))

    # ---- v1: forced, any shape; never splits.  128-row tiles: 270 / 432 rows, seams inside each
    add2("v1", "s1", 5, 64, 0, 72, 1, 1, 128, 1)
    add2("v1", "s2", 18, 64, 0, 72, 1, 1, 128, 1)
    add2("v1", "up", 2, 64, 0, 72, 1, 1, 128, 1)
    add2("v1", "concat", 5, 128, 64, 72, 1, 1, 128, 1)
    add2("v1", "wide", 2, 64, 0, 72, 1, 1, 128, 1, h=5, w=96)
    add2("v1", "s1", 5, 8, 0, 72, 1, 1, 128, 1, tag="-cin8")      # K = 72: the K % 32 != 0 tile
    add2("v1", "s2", 18, 8, 0, 72, 1, 1, 128, 1, tag="-cin8")
    # ---- v6 unsplit: the plan's own choice below 256 rows; above, forced and planned as the
    # row count at which its 64 x 64 tiles give 2 workgroups per CU (512 tiles)
    add2("v6", "s1", 3, 64, 0, 72, 0, 6, 64, 1)
    add2("v6", "s2", 11, 64, 0, 72, 0, 6, 64, 1)
    add2("v6", "up", 2, 64, 0, 72, 6, 6, 64, 1, mul=38)
    add2("v6", "concat", 3, 128, 64, 72, 0, 6, 64, 1)
    add2("v6", "long", 3, 192, 0, 72, 0, 6, 64, 1)
    add2("v6", "wide", 2, 64, 0, 72, 6, 6, 64, 1, mul=18, h=5, w=96)
    # ---- v6 forced split: from 256 rows, slices of >= 4 K-tiles (9 K-tiles: 2; 27: 4)
    add2("v6-split", "s1", 5, 64, 0, 72, 6, 6, 64, 2)
    add2("v6-split", "s2", 18, 64, 0, 72, 6, 6, 64, 2)
    add2("v6-split", "up", 2, 64, 0, 72, 6, 6, 64, 2)
    add2("v6-split", "concat", 5, 128, 64, 72, 6, 6, 64, 4)
    add2("v6-split", "wide", 2, 64, 0, 72, 6, 6, 64, 2, h=5, w=96)
    # ---- v2, 128- and 160-column tiles, unsplit: 9 K-tiles never split; 27 do unless planned as 192 tiles
    for fam, cout in (("v2-bn128", 128), ("v2-bn160", 160)):
        bn = cout
        add2(fam, "s1", 5, 64, 0, cout, 2, 2, bn, 1)
        add2(fam, "s2", 18, 64, 0, cout, 2, 2, bn, 1)
        add2(fam, "up", 2, 64, 0, cout, 2, 2, bn, 1)
        add2(fam, "concat", 5, 128, 64, cout, 2, 2, bn, 1, mul=182)
    add2("v2-bn128", "long", 5, 192, 0, 128, 2, 2, 128, 1, mul=182)
    add2("v2-bn128", "wide", 2, 64, 0, 128, 2, 2, 128, 1, h=5, w=96)
    # ---- v2, 32-column tile (N <= 32): the plan's own choice
    add2("v2-bn32", "s1", 5, 64, 0, 20, 0, 2, 32, 1)
    add2("v2-bn32", "s2", 18, 64, 0, 20, 0, 2, 32, 1)
    # ---- v2 split: Cin 128 = 18 K-tiles in 2 slices (4.5 taps each); the concat's 27 in 3
    add2("v2-split", "s1", 5, 128, 0, 128, 2, 2, 128, 2)
    add2("v2-split", "s2", 18, 128, 0, 128, 2, 2, 128, 2)
    add2("v2-split", "up", 2, 128, 0, 128, 2, 2, 128, 2)
    add2("v2-split", "concat", 5, 128, 64, 128, 2, 2, 128, 3)
    # ---- v5 (256 x 320, BK 32): Cin 96 = 13 64-wide K-tiles, unsplit; the 96 + 32 concat has 18
    add2("v5", "s1", 5, 96, 0, 128, 5, 5, 320, 1)
    add2("v5", "s2", 18, 96, 0, 128, 5, 5, 320, 1)
    add2("v5", "up", 2, 96, 0, 128, 5, 5, 320, 1)
    add2("v5", "concat", 5, 96, 32, 128, 5, 5, 320, 1, mul=182)
    add2("v5", "wide", 2, 96, 0, 128, 5, 5, 320, 1, h=5, w=96)
    # ---- v5 split: Cin 160 = 22 K-tiles in 2 slices
    add2("v5-split", "s1", 5, 160, 0, 128, 5, 5, 320, 2)
    add2("v5-split", "s2", 18, 160, 0, 128, 5, 5, 320, 2)
    add2("v5-split", "up", 2, 160, 0, 128, 5, 5, 320, 2)
    add2("v5-split", "concat", 5, 96, 32, 128, 5, 5, 320, 2)
    # ---- every family's s1 once more with a bf16 output
    for c in [c for c in out if c.mode == "s1" and "cin8" not in c.name]:
        out.append(replace(c, name=c.name + "-bf16", out_f32=False))

    # ---- temporal taps: v1 and v2 only.  2 videos of 3 frames of 9 x 6 (324 rows); stride 2:
    # 3 videos of 6 frames (270 rows)
    def add3(family, mode, cin, cout, path, kernel, bn, split, *, mul=1):
        s2, ks = mode == "t3s3-s2", 1 if mode == "t3s1" else 3
        out.append(Case(f"3d-{family}-{mode}", family, mode, 3 if s2 else 2, H, W, cin, 0, cout, path, kernel, bn,
                        split, mul=mul, stride=2 if s2 else 1, rowbias=s2, frames=6 if s2 else 3, kt=3, ks=ks,
                        halo=mode == "t3s3-halo"))

    for mode in MODES_3D:
        s2, s1 = mode == "t3s3-s2", mode == "t3s1"
        add3("v1", mode, 64, 72, 1, 1, 128, 1)
        # 27 K-tiles split 3-fold at this size; unsplit when planned as 192 tiles.  ks 1: 3 K-tiles
        add3("v2-unsplit", mode, 64, 160, 0, 2, 160, 1, mul=1 if s1 else 182 if s2 else 151)
        add3("v2-split", mode, 384 if s1 else 64, 128, 0, 2, 128, 2 if s1 else 3)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------- the plan, restated sizes
def ntile(case):
    """The N tile the plan's rules give the case's kernel (gemm.hip: ntile_128_160, the N <= 32 tile,
    v1's 64-column tile for N <= 64; v5 320, v6 64)."""
    N = case.cout
    if case.kernel == 5:
        return 320
    if case.kernel == 6:
        return 64
    if case.kernel == 2 and N <= 32:
        return 32
    if case.kernel == 1 and N <= 64:
        return 64
    p128, p160 = -(-N // 128) * 128, -(-N // 160) * 160
    return 160 if p160 < p128 or (p160 == p128 and N % 160 == 0) else 128


def ws_bytes(case):
    """vd_gemm_ws_bytes for the case's expected split: one fp32 slab per K slice and, on v6, the
    per-tile arrival counters rounded up to 256 bytes."""
    if case.split <= 1:
        return 0
    n = case.split * case.M * case.cout * 4
    if case.kernel == 6:
        n += (-(-case.M // 64) * -(-case.cout // 64) * 4 + 255) // 256 * 256
    return n


def descriptor(case, ptr=256):
    """The case's vd_gemm_desc with dummy aligned operands and its plan controls (the plan reads
    sizes and alignments only)."""
    import vdiff._lib as L
    from vdiff import ops
    d = L.GemmDesc(a0=ptr, lda0=case.c0, k0=case.c0, a1=ptr if case.c1 else None, lda1=case.c1, a_mode=ops.A_CONV3X3,
                   n_img=case.n_out, h_in=case.h, w_in=case.w, h_out=case.h_out, w_out=case.w_out,
                   stride=case.stride, upsample=int(case.up), w=ptr, ldw=case.K, M=case.M, N=case.cout, K=case.K,
                   bias=ptr if case.bias else None, out=ptr, ldc=case.cout, out_f32=int(case.out_f32), path=case.path)
    if case.rowbias:
        d.rowbias, d.ld_rb, d.rb_div = ptr, case.cout, case.rb_div
    if case.res:
        d.res, d.ld_res = ptr, case.cout
    if case.is3d:
        d.kt, d.ks, d.frames_in, d.frames_out, d.t_off = case.kt, case.ks, case.frames_in, case.frames, case.t_off
    if case.mul > 1:
        d.plan_m = case.M * case.mul
    return d


def planned(case):
    """(kernel, split, workspace bytes) of vd_gemm_plan / vd_gemm_ws_bytes: host only, no launch."""
    import vdiff._lib as L
    d = descriptor(case)
    k, sp = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert L.lib().vd_gemm_plan(ctypes.byref(d), ctypes.byref(k), ctypes.byref(sp)) == 0
    return k.value, sp.value, L.lib().vd_gemm_ws_bytes(ctypes.byref(d))


# ---------------------------------------------------------------- operands
@dataclass
class Operands:
    x0: torch.Tensor                 # [n_in * h * w, c0] bf16
    x1: Optional[torch.Tensor]       # [n_in * h * w, c1] bf16
    wt: torch.Tensor                 # [cout, cin, 3, 3] or [cout, cin, kt, ks, ks] bf16
    bias: Optional[torch.Tensor]     # [cout] fp32
    rowbias: Optional[torch.Tensor]  # [n_out, cout] fp32
    res: Optional[torch.Tensor]      # [M, cout] bf16


def operands(case):
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    rows = case.n_in * case.h * case.w
    x0 = torch.randn((rows, case.c0), generator=g).to(BF)
    x1 = torch.randn((rows, case.c1), generator=g).to(BF) if case.c1 else None
    shape = (case.cout, case.cin, case.kt, case.ks, case.ks) if case.is3d else (case.cout, case.cin, 3, 3)
    wt = (torch.randn(shape, generator=g) * case.K ** -0.5).to(BF)
    bias = torch.randn((case.cout,), generator=g) if case.bias else None
    rowbias = torch.randn((case.n_out, case.cout), generator=g) if case.rowbias else None
    res = torch.randn((case.M, case.cout), generator=g).to(BF) if case.res else None
    return Operands(x0, x1, wt, bias, rowbias, res)


def packed_weight(case, op):
    """The kernels' weight layout [Cout][taps * Cin], K = tap * Cin + ci, taps in (dt, dy, dx) order
    (vdiff.models.layers.pack_conv3x3 / pack_conv3d)."""
    perm = (0, 2, 3, 4, 1) if case.is3d else (0, 2, 3, 1)
    return op.wt.permute(*perm).reshape(case.cout, -1).contiguous()


def _epilogue(case, op, y, rb_div=None):
    if op.bias is not None:
        y = y + op.bias.double()
    if op.rowbias is not None:
        idx = torch.arange(case.M) // (case.rb_div if rb_div is None else rb_div)
        y = y + op.rowbias.double()[idx]
    if op.res is not None:   # act is VD_ACT_NONE in every case: nothing between the row bias and the residual
        y = y + op.res.double()
    return y


def reference(case, op):
    """[M, cout] fp64: torch's own convolution of the same bf16 values, then the epilogue."""
    x = op.x0 if op.x1 is None else torch.cat([op.x0, op.x1], 1)
    x = x.double()
    if case.is3d:
        vid = x.reshape(case.n, case.frames_in, case.h, case.w, case.cin).permute(0, 4, 1, 2, 3)
        # the halo form: every output frame f reads input frames f .. f + 2, no temporal padding
        y = F.conv3d(vid, op.wt.double(), stride=(1, case.stride, case.stride),
                     padding=(0 if case.halo else 1, case.ks // 2, case.ks // 2))
        assert tuple(y.shape) == (case.n, case.cout, case.frames, case.h_out, case.w_out)
        y = y.permute(0, 2, 3, 4, 1).reshape(-1, case.cout)
    else:
        img = x.reshape(case.n, case.h, case.w, case.cin).permute(0, 3, 1, 2)
        if case.up:
            img = F.interpolate(img, scale_factor=2.0, mode="nearest")
        y = F.conv2d(img, op.wt.double(), stride=case.stride, padding=1)
        assert tuple(y.shape) == (case.n, case.cout, case.h_out, case.w_out)
        y = y.permute(0, 2, 3, 1).reshape(-1, case.cout)
    return _epilogue(case, op, y)


# ---------------------------------------------------------------- the restatement and its faults
FAULTS = ("hw_swap", "row_wrap", "seam", "tap_transposed", "up_ceil", "s2_centre", "concat_half", "concat_swapped",
          "t_wrap", "t_reversed", "t_off_ignored", "rb_div_in")


def faults_of(case):
    """The loader mistakes a case's mode is exposed to."""
    f = ["hw_swap"]
    if case.ks == 3:
        f += ["row_wrap", "seam", "tap_transposed"]
    if case.up:
        f.append("up_ceil")
    if case.stride == 2:
        f.append("s2_centre")
    if case.c1:
        f += ["concat_half", "concat_swapped"]
    if case.kt == 3:   # the halo form reads frames f .. f + 2 of frames + 2: no temporal tap leaves the video
        f += ["t_reversed"] if case.halo else ["t_wrap", "t_reversed"]
    if case.halo:
        f.append("t_off_ignored")
    if case.rowbias and case.h * case.w != case.h_out * case.w_out:
        f.append("rb_div_in")
    return f


def _flat_cols(x, pix, ok, cols):
    """x[pix, cols] read as the kernels read memory — element pix * ld + col of the flat buffer, so
    a column past the row's end is the next pixel's — zero where !ok or past the buffer."""
    flat = x.double().reshape(-1)
    idx = pix[:, None] * x.shape[1] + cols[None, :]
    good = ok[:, None] & (idx >= 0) & (idx < flat.numel())
    return torch.where(good, flat[idx.clamp(0, flat.numel() - 1)], torch.zeros((), dtype=F64))


def restated(case, op, fault=None):
    """[M, cout] fp64: the implicit GEMM, explicitly.  Row m is output pixel (image, oh, ow); tap
    (dt, dy, dx) of it reads input pixel (frame + dt - 1, oh * stride + dy - 1, ow * stride + dx - 1)
    of the (upsampled) grid, zero outside; A's K index is tap * Cin + ci with channels [0, k0) from
    x0 and the rest from x1; out = A . W^T per tap, then the epilogue."""
    assert fault is None or fault in FAULTS
    c, ho, wo = case, case.h_out, case.w_out
    m = torch.arange(c.M)
    img, p = m // (ho * wo), m % (ho * wo)
    if fault == "hw_swap":
        oh, ow = p // ho, p % ho
    else:
        oh, ow = p // wo, p % wo
    t_out, t_in = max(c.frames, 1), max(c.frames_in, 1)
    vid, fr = img // t_out, img % t_out
    hg, wg = (2 * c.h, 2 * c.w) if c.up else (c.h, c.w)
    lo = 0 if fault == "s2_centre" else 1
    t_off = 0 if fault == "t_off_ignored" else c.t_off
    rows_in = c.n_in * c.h * c.w
    ci = torch.arange(c.cin)
    y = torch.zeros((c.M, c.cout), dtype=F64)
    wt = op.wt.double()
    for dt in range(c.kt):
        for dy in range(c.ks):
            for dx in range(c.ks):
                gy, gx = (dx, dy) if fault == "tap_transposed" else (dy, dx)
                ih = oh * c.stride + (gy - lo if c.ks == 3 else 0)
                iw = ow * c.stride + (gx - lo if c.ks == 3 else 0)
                fin = fr + t_off + ((c.kt - 1 - dt) if fault == "t_reversed" else dt) - c.kt // 2
                ok = torch.ones(c.M, dtype=torch.bool)
                if fault != "seam":
                    ok &= (ih >= 0) & (ih < hg)
                if fault != "row_wrap":
                    ok &= (iw >= 0) & (iw < wg)
                if fault != "t_wrap":
                    ok &= (fin >= 0) & (fin < t_in)
                if c.up:
                    ih = (ih + 1) // 2 if fault == "up_ceil" else ih // 2
                    iw = (iw + 1) // 2 if fault == "up_ceil" else iw // 2
                pix = ((vid * t_in + fin) * c.h + ih) * c.w + iw
                ok &= (pix >= 0) & (pix < rows_in)
                pix = pix.clamp(0, rows_in - 1)
                if c.c1 == 0:
                    a = _flat_cols(op.x0, pix, ok, ci)
                elif fault == "concat_swapped":
                    a = torch.cat([_flat_cols(op.x1, pix, ok, ci[:c.c1]), _flat_cols(op.x0, pix, ok, ci[:c.c0])], 1)
                else:
                    k0 = c.cin // 2 if fault == "concat_half" else c.c0
                    a = torch.cat([_flat_cols(op.x0, pix, ok, ci[:k0]), _flat_cols(op.x1, pix, ok, ci[:c.cin - k0])], 1)
                w_tap = wt[:, :, dt, dy, dx] if c.is3d else wt[:, :, dy, dx]
                y += a @ w_tap.T
    return _epilogue(c, op, y, rb_div=c.h * c.w if fault == "rb_div_in" else None)


# ---------------------------------------------------------------- the bound
def tolerance(case, ref):
    """(rtol, atol) the GPU test holds the case to: |got - ref| <= atol + rtol |ref|.  fp32 outputs:
    test_gpu_memframe.conv_case's bound; bf16 outputs: memframe.close_bf16's (rel 1/128, 2e-3 of
    the largest |ref|)."""
    top = ref.abs().max().item()
    if not case.out_f32:
        return 1 / 128, 2e-3 * (top + 1e-12)
    return 1e-3, (1e-3 if case.is_split else 1e-4) * max(1.0, top)


def worst_ratio(got, ref, rtol, atol):
    """max over elements of |got - ref| / (atol + rtol |ref|); a NaN anywhere is inf."""
    got, ref = got.double().cpu(), ref.double().cpu()
    r = (got - ref).abs() / (atol + rtol * ref.abs())
    return float("inf") if torch.isnan(r).any() else r.max().item()
