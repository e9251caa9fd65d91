"""FreeInit benchmark: the spectral low-pass filter and the iterated call, 1x MI355X.

    python tools/free_init_bench.py [--rounds 7] [--inner 20] [--steps 25] [--iters 3] [--skip-call] [--out profiles/free_init_bench.json]

1. The filter at n_vol = 4 and 8 volumes of 16 x 64 x 64 (one and two videos of 4 latent channels),
   two forms interleaved round by round:
     (a) ops.free_init_filter: five launches of vd_rows_eltwise op 6 (direct DFTs out of LDS)
     (b) torch.fft doing what diffusers' _apply_freq_filter does on the same device: fftn of x and of
         the noise, two fftshifts, the mix, ifftshift, ifftn, .real (plain torch: it runs on the
         parent commit as well)
   each timed with device events over `inner` back-to-back calls; reported: the median over rounds
   and the spread (max - min) / median.  When torch.fft is not usable on the device its error is
   recorded instead.
2. The call: the full config at 16 frames, CFG, `steps` steps, output_type "latent": one call with
   enable_free_init(num_iters=iters) beside `iters` plain calls, wall time around a device
   synchronize, median over 3 rounds after one warm-up round.
Weights are random; the numbers are recorded, nothing is gated on them.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "video-diffusion-experiments_amd")]

import torch  # noqa: E402

import vdiff  # noqa: E402
from vdiff import ops  # noqa: E402

FR, H, W = 16, 64, 64
DIMS = (-3, -2, -1)


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


def torch_fft_filter(x, noise, lpf):
    xf = torch.fft.fftshift(torch.fft.fftn(x, dim=DIMS), dim=DIMS)
    nf = torch.fft.fftshift(torch.fft.fftn(noise, dim=DIMS), dim=DIMS)
    mixed = xf * lpf + nf * (1 - lpf)
    return torch.fft.ifftn(torch.fft.ifftshift(mixed, dim=DIMS), dim=DIMS).real


def filter_forms(n_vol, rounds, inner):
    g = torch.Generator(device="cuda").manual_seed(n_vol)
    x = torch.randn(n_vol, FR, H, W, device="cuda", generator=g)
    noise = torch.randn(n_vol, FR, H, W, device="cuda", generator=g)
    table = ops.free_init_table(FR, H, W, device="cuda")
    lpf = ops.free_init_mask(FR, H, W, "butterworth", 4, 0.25, 0.25).float().cuda()
    out = torch.empty_like(x)
    scratch = torch.empty(n_vol * FR * H * 2 * (W // 2 + 1), device="cuda")
    forms = {"a_free_init_filter": lambda: ops.free_init_filter(x, noise, table, out=out, scratch=scratch)}
    rec = {"n_vol": n_vol, "F": FR, "H": H, "W": W}
    try:
        ref = torch_fft_filter(x, noise, lpf)
        torch.cuda.synchronize()
        forms["b_torch_fft"] = lambda: torch_fft_filter(x, noise, lpf)
    except Exception as e:  # no FFT backend for this device in this torch build
        rec["b_torch_fft"] = {"error": repr(e)[:200]}
        ref = None
    for f in forms.values():  # warm-up
        timed(f, 3)
    if ref is not None:
        rec["max_abs_diff_a_vs_b"] = float((out - ref).abs().max())
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            t[k].append(timed(f, inner))
    rec.update({k: summary(v) for k, v in t.items()})
    if "b_torch_fft" in t:
        rec["a_over_b"] = round(rec["a_free_init_filter"]["median_us"] / rec["b_torch_fft"]["median_us"], 3)
    return rec


def whole_call(steps, iters, rounds=3):
    pipe = vdiff.AnimateDiffPipeline.from_config("full", device="cuda", vae=None)
    cross = pipe.unet.config["cross_attention_dim"]
    g = torch.Generator().manual_seed(0)
    kw = dict(prompt_embeds=torch.randn(1, 77, cross, generator=g), negative_prompt_embeds=torch.randn(1, 77, cross, generator=g),
              num_frames=FR, num_inference_steps=steps, guidance_scale=7.5, output_type="latent")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def plain():
        for i in range(iters):
            pipe(generator=torch.Generator().manual_seed(i), **kw)

    def free_init():
        pipe.enable_free_init(num_iters=iters)
        try:
            pipe(generator=torch.Generator().manual_seed(0), **kw)
        finally:
            pipe.disable_free_init()

    t = {"plain_calls": [], "free_init_call": []}
    for r in range(rounds + 1):  # round 0 warms up
        a, b = wall(plain), wall(free_init)
        if r:
            t["plain_calls"].append(a)
            t["free_init_call"].append(b)
    rec = {"config": "full", "frames": FR, "steps": steps, "num_iters": iters, "rounds": rounds}
    for k, v in t.items():
        med = statistics.median(v)
        rec[k] = {"median_ms": round(med, 1), "spread": round((max(v) - min(v)) / med, 4)}
    rec["free_init_over_plain"] = round(rec["free_init_call"]["median_ms"] / rec["plain_calls"]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--skip-call", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "free_init_bench.json"))
    args = ap.parse_args()
    rec = {"metric": "FreeInit: the 3-D spectral low-pass (us per filter of n_vol x 16 x 64 x 64, beside torch.fft's six "
                     "transforms) and one num_iters-iteration call beside num_iters plain calls (ms)",
           "weights": "random", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inner": args.inner,
           "filter": []}
    for n_vol in (4, 8):
        rec["filter"].append(filter_forms(n_vol, args.rounds, args.inner))
        print(f"[free_init_bench] n_vol {n_vol} done", file=sys.stderr, flush=True)
    if not args.skip_call:
        rec["call"] = whole_call(args.steps, args.iters)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
