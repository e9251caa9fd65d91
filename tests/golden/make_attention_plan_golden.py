"""The attention plan's decision table, written from a restatement of the rules the library had
BEFORE its attention source was split (commit 1bd7b3e), not from the library under test:

    python tests/golden/make_attention_plan_golden.py          # writes tests/golden/attention_plan.npz
    python tests/golden/make_attention_plan_golden.py --dump   # one readable line per case, to stdout

parent_plan() transcribes csrc/attention.hip of 1bd7b3e — attention_entry, launch_flash,
launch_flash_causal, launch_flash_tail — rule by rule, each with the line it came from
("P:<line>").  It needs no library and no GPU.  tests/test_attention_plan.py sends the same grid
through vd_attention_plan (host-only) and compares entry for entry: which kernel family a call
runs, the 16x16x32 kernel's QBLK, the unit-scale instance, and both launch grids are what that
commit launched.  Regenerate only with a change that means to move a decision.

The grid: every (d, sq, skv, forced kernel, causal, tail) of the edge values below, each plain and
with one variation at a time (fp32 output, an output only 8-byte aligned, a row stride that is a
multiple of 4 only, the two together with fp32, the scale that makes c == 1, a shared K/V batch,
and a batch x heads that takes a workgroup count past 2^31 - 1).
"""
import ctypes
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "video-diffusion-experiments_amd")]

OUT = HERE / "attention_plan.npz"
FIELDS = ("rc", "family", "qblk", "unit_scale", "grid", "exact_grid")
OK, EINVAL, EUNSUPPORTED = 0, 1000, 1001
FLASH, FLASH32, FLASH40, FLASH80, FLASH512 = 1, 2, 3, 4, 5  # VD_ATTN_K_*
CAUSAL, TAIL_SHIFT, TAIL_MASK = 0x100, 16, 0x7F0000         # VD_ATTN_CAUSAL, VD_ATTN_TAIL(n)
KT, F4_QWG, F8K_QWG, F32_FIXW, A5_QWG = 64, 512, 256, 16, 128  # P:34, P:1016, P:1528, P:837, d512:36
LOG2E = np.float32(1.4426950408889634)

PTR, PTR8 = 256, 264  # output addresses: 16-byte aligned, and 8- but not 16-byte aligned
D = (32, 40, 48, 64, 80, 128, 160, 512)
S = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4096)
KERNEL = (0, 1, 2, 3)
TAIL = (0, 1, 64, 65)
UNIT_SCALE = float(np.float32(1.0 / 1.4426950408889634))  # c = scale * log2(e) == 1 in fp32
assert np.float32(UNIT_SCALE) * LOG2E == np.float32(1.0)
VARIANTS = ("plain", "out_f32", "o_al8", "ldo4", "out_f32_ldo4", "unit_scale", "kv_div2", "huge")


def grid():
    """Yields (d, sq, skv, batch, heads, kv_div, o, ldo, out_f32, kernel word, scale) in table order."""
    for d in D:
        for sq in S:
            for skv in S:
                for k in KERNEL:
                    for causal in (0, CAUSAL):
                        for tail in TAIL:
                            word = k | causal | (tail << TAIL_SHIFT)
                            for var in VARIANTS:
                                batch, heads, kv_div = (65535, 65535, 1) if var == "huge" else (2, 8, 1)
                                if var == "kv_div2":
                                    kv_div = 2
                                ldo = heads * d + (4 if var in ("ldo4", "out_f32_ldo4") else 0)
                                yield (d, sq, skv, batch, heads, kv_div, PTR8 if var == "o_al8" else PTR, ldo,
                                       int(var in ("out_f32", "out_f32_ldo4")), word,
                                       UNIT_SCALE if var == "unit_scale" else d ** -0.5)


def describe(c):
    d, sq, skv, batch, heads, kv_div, o, ldo, out_f32, word, scale = c
    return (f"d={d} sq={sq} skv={skv} batch={batch} heads={heads} kv_div={kv_div} o@{o % 16} ldo={ldo} "
            f"out_f32={out_f32} kernel={word & 0xff} causal={int(bool(word & CAUSAL))} "
            f"tail={(word & TAIL_MASK) >> TAIL_SHIFT} scale={scale:.6g}")


def _refuse(rc):
    return (rc, 0, 0, 0, 0, 0)


def _flash(d, sq, heads, batch):
    """The 16x16x32 kernel's launch, the same three times over (P:1929-1944, P:1953-1966, P:1975-1988):
    QBLK 4 for d <= 40 from sq = 1024, grid (ceil(sq / (64 QBLK)), heads, batch), no refusal."""
    qblk = 4 if d <= 40 and sq >= 1024 else 2           # P:1929-1930 / P:1953-1954 / P:1975-1976
    qwg = 256 if qblk == 4 else 128                     # P:1931 / P:1939 (and the causal / tail copies)
    return (OK, FLASH, qblk, 0, (sq + qwg - 1) // qwg * heads * batch, 0)


def parent_plan(d, sq, skv, batch, heads, kv_div, o, ldo, out_f32, word, scale):
    """(rc, family, qblk, unit_scale, grid, exact_grid) of commit 1bd7b3e for one call."""
    # ---- attention_entry's argument checks that read these arguments (P:2451-2457)
    if not (o and o % 8 == 0):                          # P:2451
        return _refuse(EINVAL)
    if ldo % 4:                                         # P:2452
        return _refuse(EINVAL)
    if out_f32 and o % 16:                              # P:2453
        return _refuse(EINVAL)
    if not (batch > 0 and heads > 0 and sq > 0 and skv > 0 and kv_div > 0 and batch % kv_div == 0):  # P:2454
        return _refuse(EINVAL)
    if not (batch <= 65535 and heads <= 65535):         # P:2455
        return _refuse(EINVAL)
    if not (word >= 0 and (word & ~(0xFF | CAUSAL | TAIL_MASK)) == 0 and (word & 0xFF) <= 3):  # P:2457
        return _refuse(EINVAL)
    tail = (word & TAIL_MASK) >> TAIL_SHIFT             # P:2459
    if tail:
        if not (tail <= KT and tail < skv and not (word & CAUSAL) and scale > 0):  # P:2460
            return _refuse(EINVAL)
        if d not in (32, 40, 64, 80, 160):              # P:2461-2468
            return _refuse(EUNSUPPORTED)
        return _flash(d, sq, heads, batch)              # launch_flash_tail, P:1970-1989
    if word & CAUSAL:                                   # P:2470
        if not (sq == skv and kv_div == 1 and scale > 0):  # P:2471
            return _refuse(EINVAL)
        if d not in (32, 64):                           # P:2472-2476
            return _refuse(EUNSUPPORTED)
        return _flash(d, sq, heads, batch)              # launch_flash_causal, P:1948-1967
    kernel = word                                       # no bit above the low byte is left (P:2479-2484)
    if d == 512:                                        # P:2485 -> attention_d512.hip launch_flash512
        if o % 16 or ldo % (4 if out_f32 else 8):       # d512:344
            return _refuse(EINVAL)
        nblk = (sq + A5_QWG - 1) // A5_QWG * heads * batch  # d512:348
        if nblk > 0x7FFFFFFF:                           # d512:349
            return _refuse(EINVAL)
        return (OK, FLASH512, 0, 0, nblk, 0)
    if d not in (32, 40, 64, 80, 128, 160):             # P:2478-2486
        return _refuse(EUNSUPPORTED)
    # ---- launch_flash<D> (P:1868-1945)
    unit = int(np.float32(scale) * LOG2E == np.float32(1.0))  # c (P:1872), c == 1.0f (P:1882 / 1901 / 1918)
    oal = o % 16 == 0 and ldo % (4 if out_f32 else 8) == 0     # P:1874 (d = 40), P:1914 (d = 80)
    if d == 40:                                         # P:1873
        if (kernel == 3 or (kernel == 0 and skv >= 256)) and skv >= 2 * KT and oal:  # P:1876
            nblk = (sq + F4_QWG - 1) // F4_QWG * heads * batch  # P:1877
            if nblk > 0x7FFFFFFF:                       # P:1878
                return _refuse(EINVAL)
            nfix = (sq + 127) // 128 * heads * batch    # P:1880
            return (OK, FLASH40, 0, unit, nblk, (nfix + F32_FIXW - 1) // F32_FIXW)  # P:1881
        if kernel != 1 and oal:                         # P:1897
            nblk = (sq + 255) // 256 * heads * batch    # P:1898
            if nblk > 0x7FFFFFFF:                       # P:1899
                return _refuse(EINVAL)
            return (OK, FLASH32, 0, unit, nblk, 0)
    if d == 80:                                         # P:1912
        if (kernel == 3 or (kernel == 0 and skv >= 4 * KT)) and skv >= 2 * KT and oal:  # P:1915
            nblk = (sq + F8K_QWG - 1) // F8K_QWG * heads * batch  # P:1916
            if nblk > 0x7FFFFFFF:                       # P:1917
                return _refuse(EINVAL)
            return (OK, FLASH80, 0, unit, nblk, 0)
    return _flash(d, sq, heads, batch)                  # P:1929-1944


def _arrays(rows):
    cols = list(zip(*rows))
    types = (np.int16, np.int8, np.int8, np.int8, np.int64, np.int64)
    return tuple(np.asarray(c, t) for c, t in zip(cols, types))


def table():
    """The restatement over the grid: FIELDS arrays in grid order."""
    return _arrays([parent_plan(*c) for c in grid()])


def evaluate():
    """The library (vd_attention_plan) over the grid: FIELDS arrays in grid order."""
    from vdiff import _lib as L

    plan = L.lib().vd_attention_plan
    fam, qb, us = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    g, eg = ctypes.c_int64(), ctypes.c_int64()
    refs = tuple(ctypes.byref(x) for x in (fam, qb, us, g, eg))
    rows = []
    for d, sq, skv, batch, heads, kv_div, o, ldo, out_f32, word, scale in grid():
        fam.value = qb.value = us.value = g.value = eg.value = -1
        rc = plan(o, ldo, batch, heads, sq, skv, d, kv_div, scale, out_f32, word, *refs)
        rows.append((rc, fam.value, qb.value, us.value, g.value, eg.value))
    return _arrays(rows)


def main():
    if "--dump" in sys.argv[1:]:
        for i, c in enumerate(grid()):
            print(i, describe(c), "->", dict(zip(FIELDS, parent_plan(*c))))
        return
    t = table()
    np.savez_compressed(OUT, **dict(zip(FIELDS, t)))
    print(f"{OUT.name}: {len(t[0])} cases, {OUT.stat().st_size} bytes; families {sorted(set(t[1].tolist()))}, "
          f"return codes {sorted(set(t[0].tolist()))}")


if __name__ == "__main__":
    main()
