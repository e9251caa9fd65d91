"""Same-process A/B of the GEMM / implicit-GEMM conv library code (csrc/gemm*.hip) against earlier
forms of its source: each arm is a DIAGNOSTIC library built from a saved copy of a revision's GEMM
sources (gemm.hip alone, or gemm.hip with the per-family gemm_*.hip and gemm_common.h; plus the
product's other objects), loaded RTLD_LOCAL beside the product library.  Every case runs through
the real vdiff.ops API with the arm's library swapped in as vdiff._lib's handle (same plan, same
descriptors), arms interleaved, outputs compared bit for bit against the product's.

Cases: the UNet's 3x3 convs at the 16-frame CFG batch (32 images) — stride 1 at every level,
the channel-concat convs of the up blocks, a stride-2 downsample, a nearest-x2 upsample — and a
(2+1)D temporal conv (kt = 3, ks = 1); GEMM_AB_CASES=geglu: the four GEGLU projections instead;
GEMM_AB_CASES=v1: the small shapes v1's 128 x 160 tiles take (text K/V projection, conv_in);
GEMM_AB_CASES=ff: the level-1 FeedForward as vd_ff_fused's one launch against the two vd_gemm
launches it replaces (product library only; GEMM_AB_FF_M=131072,16384,8192 for other row counts).

    python tools/gemm_ab.py --save NAME [--rev REV]   # here: tools/diag_gemm/src_NAME/ from git REV (default HEAD)
    python tools/gemm_ab.py --build                   # here (CPU): tools/diag_gemm/libvdiff_gemm_NAME.so
    python tools/gemm_ab.py [--rounds 7]              # GPU box
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "video-diffusion-experiments_amd"
OUT = ROOT / "tools" / "diag_gemm"  # git-ignored; not gpurun-ignored (the box loads these libs)
REL = "video-diffusion-experiments_amd/csrc"


def is_gemm_source(name: str) -> bool:
    """The GEMM sources of a revision: gemm.hip alone, or the per-family gemm*.hip / gemm*.h."""
    return name.startswith("gemm") and name.endswith((".hip", ".h"))


def save(name: str, rev: str):
    d = OUT / f"src_{name}"
    d.mkdir(parents=True, exist_ok=True)
    git = ["git", "-C", str(ROOT)]
    ls = subprocess.run([*git, "ls-tree", "--name-only", rev, REL + "/"], check=True, capture_output=True, text=True)
    for f in (Path(p).name for p in ls.stdout.split()):
        if is_gemm_source(f) or f == "common.h":
            src = subprocess.run([*git, "show", f"{rev}:{REL}/{f}"], check=True, capture_output=True, text=True).stdout
            (d / f).write_text(src)
            print("saved", d / f, "from", rev)


def arms():
    return sorted(p.name[4:] for p in OUT.glob("src_*") if (p / "gemm.hip").exists())


def build():
    sys.path.insert(0, str(PKG))
    import build_ext as B
    for name in arms():
        # the arm's own headers first (a quoted include looks beside the including file), then the tree's
        defs = ['-DVD_BUILD_HASH="diag"', f'-DVD_BUILD_ARCH="{B.ARCH}"', f"-I{B.CSRC}", f"-I{ROOT / 'include'}"]
        objs = []
        for src in sorted((OUT / f"src_{name}").glob("*.hip")):
            obj = OUT / f"{src.stem}_{name}.o"
            subprocess.run([B.HIPCC, *B.CFLAGS, *defs, "-c", str(src), "-o", str(obj)], check=True)
            objs.append(str(obj))
        objs += [str(p) for p in sorted(B.BUILD.glob("*.o")) if not is_gemm_source(p.stem + ".hip")]
        lib = OUT / f"libvdiff_gemm_{name}.so"
        subprocess.run([B.HIPCC, f"--offload-arch={B.ARCH}", "-shared", "-fPIC", "-o", str(lib), *objs,
                        "-L/opt/rocm/lib"], check=True)
        print("built", lib)


def run(rounds: int):
    sys.path[:0] = [str(ROOT), str(PKG)]
    import torch
    import vdiff._lib as L
    from vdiff import ops
    libs = {"product": L.lib()}
    for name in arms():
        h = C.CDLL(str(OUT / f"libvdiff_gemm_{name}.so"), mode=os.RTLD_NOW | os.RTLD_LOCAL)
        for fn, (argt, rest) in L.SIGNATURES.items():
            f = getattr(h, fn)
            f.argtypes, f.restype = argt, rest
        libs[name] = h

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*s, scale=1.0):
        return (torch.randn(*s, device=dev, generator=g) * scale).to(torch.bfloat16)

    n = 32
    cases = []

    def conv(name, h, w, c0, cout, c1=0, stride=1, upsample=False):
        x = rnd(n * h * w, c0)
        x1 = rnd(n * h * w, c1) if c1 else None
        wt = rnd(cout, 9 * (c0 + c1), scale=(9 * (c0 + c1)) ** -0.5)
        b = torch.randn(cout, device=dev, generator=g)
        fl = 2.0 * n * (2 * h if upsample else (h - 1) // stride + 1) * (2 * w if upsample else (w - 1) // stride + 1) \
            * cout * 9 * (c0 + c1)
        cases.append((name, lambda: ops.conv3x3(x, n, h, w, wt, x1=x1, stride=stride, upsample=upsample, bias=b)[0],
                      fl))

    def geglu(name, M, N, K):  # GEGLU projection (hidden | gate interleaved, 2N rows of W) with its GELU epilogue
        a = rnd(M, K)
        wt = rnd(2 * N, K, scale=K ** -0.5)
        b = torch.randn(2 * N, device=dev, generator=g)
        cases.append((name, lambda: ops.gemm(a, wt, bias=b, act=ops.ACT_GEGLU), 2.0 * M * 2 * N * K))

    if os.environ.get("GEMM_AB_CASES") == "geglu":
        geglu("L1 GEGLU 320->2x1280", n * 64 * 64, 1280, 320)
        geglu("L2 GEGLU 640->2x2560", n * 32 * 32, 2560, 640)
        geglu("L3 GEGLU 1280->2x5120", n * 16 * 16, 5120, 1280)
        geglu("L4 GEGLU 1280->2x5120", n * 8 * 8, 5120, 1280)
    elif os.environ.get("GEMM_AB_CASES") == "v1":
        # gemm_kernel<128, 160, dense>: the time-embedding MLP (M = the CFG batch, below one 64-row tile);
        # gemm_kernel<128, 160, conv>: conv_in (K = 9 x 8 = 72 is no multiple of 32)
        for kk in (320, 1280):
            a, wt = rnd(2, kk), rnd(1280, kk, scale=kk ** -0.5)
            cases.append((f"temb MLP {kk}->1280", lambda a=a, wt=wt: ops.gemm(a, wt), 2.0 * 2 * 1280 * kk))
        conv("conv_in 8->320", 64, 64, 8, 320)
    else:
        conv("L1 conv 320->320", 64, 64, 320, 320)
        conv("L2 conv 640->640", 32, 32, 640, 640)
        conv("L3 conv 1280->1280", 16, 16, 1280, 1280)
        conv("L4 conv 1280->1280", 8, 8, 1280, 1280)
        conv("L1 up concat 320+320", 64, 64, 320, 320, c1=320)
        conv("L2 up concat 640+320", 32, 32, 640, 640, c1=320)
        conv("L1 down stride 2", 64, 64, 320, 320, stride=2)
        conv("L2 upsample x2", 16, 16, 640, 640, upsample=True)
        # (2+1)D temporal half: kt = 3, ks = 1 over 2 videos x 16 frames at level 2
        xt = rnd(n * 32 * 32, 640)
        wtt = rnd(640, 3 * 640, scale=(3 * 640) ** -0.5)
        cases.append(("L2 temporal kt3", lambda: ops.conv3d(xt, 2, 16, 32, 32, wtt, kt=3, ks=1)[0],
                      2.0 * n * 32 * 32 * 640 * 3 * 640))

    def with_lib(h, fn):
        saved = L._lib
        L._lib = h
        try:
            return fn()
        finally:
            L._lib = saved

    for name, fn, fl in cases:
        ref = with_lib(libs["product"], fn)
        torch.cuda.synchronize()
        ref = ref.clone()
        same = {}
        for a, h in libs.items():
            if a != "product":
                o = with_lib(h, fn)
                torch.cuda.synchronize()
                same[a] = torch.equal(o, ref)
        res = {a: [] for a in libs}
        for r in range(rounds + 1):
            for a, h in libs.items():
                with_lib(h, fn)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    with_lib(h, fn)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    res[a].append(e0.elapsed_time(e1) * 100.0)  # us per call
        med = {a: sorted(v)[len(v) // 2] for a, v in res.items()}
        line = "  ".join(f"{a} {m:7.1f} us ({fl / m / 1e6:5.0f} TF/s{'' if a == 'product' else ', ' + ('bit-identical' if same[a] else 'DIFFERS')})"
                         for a, m in med.items())
        print(f"{name:22s} {line}", flush=True)


def run_ff(rounds: int, Ms=(131072,)):
    """GEMM_AB_CASES=ff: the level-1 FeedForward as the one fused launch (vd_ff_fused) against the
    sum of the two launches it replaces (GEGLU with the folded norm3, then ff2 + bias + residual),
    product library only, same process, arms interleaved per round, outputs compared bit for bit.
    GEMM_AB_FF_M=M1,M2 sets the row counts (default 131072; the rank shapes are 16384 and 8192)."""
    sys.path[:0] = [str(ROOT), str(PKG)]
    import torch
    from vdiff import ops
    from vdiff.models.layers import LnFold, pack_geglu

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    Cc, H = 320, 1280
    norm = torch.nn.LayerNorm(Cc).to(dev)
    w1 = 0.02 * torch.randn(2 * H, Cc, device=dev, generator=g)
    b1 = 0.02 * torch.randn(2 * H, device=dev, generator=g)
    fold = LnFold(norm, w1, b1, pack=pack_geglu)
    w1p, b1p = pack_geglu(w1.to(torch.bfloat16)), pack_geglu(b1.float())
    w2 = (0.02 * torch.randn(Cc, H, device=dev, generator=g)).to(torch.bfloat16)
    b2 = 0.02 * torch.randn(Cc, device=dev, generator=g)
    for M in Ms:
        x = torch.randn(M, Cc, device=dev, generator=g).to(torch.bfloat16)
        out = torch.empty_like(x)
        hid = torch.empty(M, H, device=dev, dtype=torch.bfloat16)
        for label, folded in (("folded", True), ("unfolded", False)):
            if folded and not fold.runs(M, ops.ACT_GEGLU):
                continue

            def pair():
                if folded:
                    ops.gemm(x, fold.w, bias=fold.b, act=ops.ACT_GEGLU, ln_fold=(fold.s, fold.eps), out=hid)
                else:
                    ops.gemm(x, w1p, bias=b1p, act=ops.ACT_GEGLU, out=hid)
                return ops.gemm(hid, w2, bias=b2, res=x, out=out)

            def one():
                if folded:
                    return ops.ff_fused(x, fold.w, w2, b1=fold.b, b2=b2, res=x, ln_fold=(fold.s, fold.eps), out=out)
                return ops.ff_fused(x, w1p, w2, b1=b1p, b2=b2, res=x, out=out)

            want = pair().clone()
            same = torch.equal(one(), want)
            torch.cuda.synchronize()
            arms_ = {"two launches": pair, "fused": one}
            res = {a: [] for a in arms_}
            for r in range(rounds + 1):
                for a, fn in arms_.items():
                    fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(10):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if r:
                        res[a].append(e0.elapsed_time(e1) * 100.0)  # us per call
            fl = 2.0 * M * Cc * 3 * H
            line = "  ".join(f"{a} median {sorted(v)[len(v) // 2]:7.1f} us (min {min(v):7.1f} max {max(v):7.1f}, "
                             f"{fl / sorted(v)[len(v) // 2] / 1e6:5.0f} TF/s)" for a, v in res.items())
            print(f"L1 FeedForward M={M} {label:8s} {line}  fused {'bit-identical' if same else 'DIFFERS'}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--save")
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if a.save:
        save(a.save, a.rev)
    elif a.build:
        build()
    elif os.environ.get("GEMM_AB_CASES") == "ff":
        run_ff(a.rounds, tuple(int(m) for m in os.environ.get("GEMM_AB_FF_M", "131072").split(",")))
    else:
        run(a.rounds)
