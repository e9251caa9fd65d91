"""FreeU benchmark: what enable_freeu adds to a denoising step, bf16, 1x MI355X.

    python tools/freeu_bench.py [--rounds 7] [--inner 20] [--steps 3] [--skip-step] [--out profiles/freeu_bench.json]

1. Per product shape of the full config at 16 frames with CFG (32 images; the skips of
   up_blocks[0] at 8x8x1280 and of up_blocks[1] at 16x16x1280 and 16x16x640), three things:
     (a) vd_rows_eltwise op 2, the one-launch spectral skip filter       — what the model runs
     (b) vd_rows_eltwise op 3 on the first half of 1280 hidden channels  — the backbone scale
     (c) the stock composition on the same rows: NHWC bf16 -> NCHW fp32, torch.fft.fftn,
         fftshift, the 2x2 mask, ifftshift, ifftn, .real, back to NHWC bf16 (diffusers'
         fourier_filter around our layout).  If torch.fft does not run on the device, (c) is
         the closed form in torch ops instead, and "stock_form" says so.
   The forms are interleaved round by round, each timed with device events over `inner`
   back-to-back launches; reported: the median over rounds and the spread (max - min) / median.
2. The whole step: DenoiseLoop (graph replay) at the full config with and without FreeU, in one
   session, interleaved; the added ms per step.
Weights are random; no speed is promised.
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "video-diffusion-experiments_amd")]

import torch  # noqa: E402

import vdiff  # noqa: E402
from vdiff import ops  # noqa: E402

BF16 = torch.bfloat16
IMAGES, FRAMES, L = 32, 16, 77
SHAPES = [(8, 8, 1280), (16, 16, 1280), (16, 16, 640)]  # (H, W, C) of the filtered skips
HIDDEN = 1280  # hidden channels of every resnet input in up_blocks[0] and [1]
FREEU = dict(s1=0.9, s2=0.2, b1=1.2, b2=1.4)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us


def summary(xs):
    med = statistics.median(xs)
    return {"median_us": round(med, 2), "spread": round((max(xs) - min(xs)) / med, 4)}


def stock_fft(x, n, h, w, s):
    xf = x.view(n, h, w, -1).permute(0, 3, 1, 2).float()
    xf = torch.fft.fftshift(torch.fft.fftn(xf, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(xf.shape, device=x.device)
    mask[..., h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1] = s
    y = torch.fft.ifftn(torch.fft.ifftshift(xf * mask, dim=(-2, -1)), dim=(-2, -1)).real
    return y.permute(0, 2, 3, 1).reshape(n * h * w, -1).to(BF16)


def stock_closed_form(x, n, h, w, s):
    xf = x.view(n, h * w, -1).float()
    th = (2 * math.pi * torch.arange(h, device=x.device) / h)[:, None].expand(h, w).reshape(-1)
    tw = (2 * math.pi * torch.arange(w, device=x.device) / w)[None, :].expand(h, w).reshape(-1)
    basis = torch.stack([torch.ones_like(th), th.cos(), th.sin(), tw.cos(), tw.sin(), (th + tw).cos(), (th + tw).sin()])
    corr = torch.einsum("kp,nkc->npc", basis, torch.einsum("kp,npc->nkc", basis, xf))
    return (xf + (s - 1) / (h * w) * corr).reshape(n * h * w, -1).to(BF16)


def filter_forms(h, w, c, rounds, inner):
    g = torch.Generator(device="cuda").manual_seed(h + c)
    rows = IMAGES * h * w
    x = torch.randn(rows, c, device="cuda", generator=g).to(BF16)
    hid = torch.randn(rows, HIDDEN, device="cuda", generator=g).to(BF16)
    out = torch.empty_like(x)
    s_dev, one = torch.tensor([0.2], device="cuda"), torch.ones(1, device="cuda")
    stock, stock_form = stock_fft, "torch.fft"
    try:
        stock(x, IMAGES, h, w, 0.2)
        torch.cuda.synchronize()
    except Exception as e:  # no FFT library behind torch.fft on this device
        stock, stock_form = stock_closed_form, f"closed form in torch ops (torch.fft failed: {type(e).__name__})"
    forms = {"a_filter_op2": lambda: ops.freeu_filter(x, IMAGES, h, w, s_dev, out=out),
             "b_scale_op3_half_of_1280": lambda: ops.scale_rows_(hid[:, :HIDDEN // 2], one),
             "c_stock": lambda: stock(x, IMAGES, h, w, 0.2)}
    got, want = forms["a_filter_op2"]().float(), forms["c_stock"]().float()
    agree = ((got - want).norm() / want.norm()).item()
    for f in forms.values():  # warm-up
        timed(f, 3)
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            t[k].append(timed(f, inner))
    rec = {"H": h, "W": w, "C": c, "images": IMAGES, "stock_form": stock_form,
           "op2_vs_stock_rel_l2": round(agree, 6), **{k: summary(v) for k, v in t.items()}}
    nbytes = 2 * rows * c * 2  # read x once, write out once
    rec["a_filter_op2"]["gb_per_s"] = round(nbytes / rec["a_filter_op2"]["median_us"] / 1e3, 1)
    return rec


def whole_step(rounds, steps):
    pipe = vdiff.AnimateDiffPipeline.from_config("full", device="cuda", vae=None)
    unet = pipe.unet
    s = unet.config["sample_size"]
    lat = torch.randn(1, unet.config["in_channels"], FRAMES, s, s)
    ehs = torch.randn(2, L, unet.config["cross_attention_dim"])
    pipe.scheduler.set_timesteps(50)
    plain = vdiff.DenoiseLoop(unet, pipe.scheduler, lat, ehs, 7.5).prime()
    pipe.enable_freeu(**FREEU)  # stays enabled: the second graph reads the blocks' device scalars
    freeu = vdiff.DenoiseLoop(unet, pipe.scheduler, lat, ehs, 7.5).prime()
    loops = {"without_freeu": plain, "with_freeu": freeu}
    t = {k: [] for k in loops}
    for lp in loops.values():
        lp.run(2)
    for _ in range(rounds):
        for k, lp in loops.items():
            lp.reset(lat.to("cuda", torch.float32))
            t[k].append(timed(lambda lp=lp: lp.run(1), steps) / 1e3)  # ms per step
    rec = {k: {"median_ms": round(statistics.median(v), 3), "spread": round((max(v) - min(v)) / statistics.median(v), 4)}
           for k, v in t.items()}
    rec["added_ms_per_step"] = round(rec["with_freeu"]["median_ms"] - rec["without_freeu"]["median_ms"], 3)
    rec["graph"] = [lp.graph is not None for lp in loops.values()]
    rec["freeu"] = FREEU
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "freeu_bench.json"))
    args = ap.parse_args()
    rec = {"metric": "FreeU: the skip filter and the backbone scale (us per launch) and added ms per step",
           "config": "full, 16 frames, CFG (32 images); 6 filter + 6 scale launches per step", "weights": "random",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inner": args.inner,
           "filter": []}
    for h, w, c in SHAPES:
        rec["filter"].append(filter_forms(h, w, c, args.rounds, args.inner))
        print(f"[freeu_bench] {h}x{w}x{c} done", file=sys.stderr, flush=True)  # the first FFT plan can take a while
    if not args.skip_step:
        rec["step"] = whole_step(args.rounds, args.steps)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
