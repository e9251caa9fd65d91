"""FreeNoise benchmark: the window gather / merge kernels and the windowed step, bf16, 1x MI355X.

    python tools/free_noise_bench.py [--rounds 7] [--inner 20] [--steps 2] [--skip-step] [--out profiles/free_noise_bench.json]

1. Per product shape (B = 2 videos of F = 32 frames, windows of 16 by 4: 5 per video; hw x C of
   the UNet's three levels at 32 x 32 latents), three launches interleaved round by round:
     (a) vd_rows_eltwise op 4, the window gather   reads B*nW*L*hw rows, writes as many
     (b) vd_rows_eltwise op 5, the weighted merge  reads the rows regular windows cover, writes B*F*hw
     (c) vd_rows_eltwise op 0 (out = 0 + y) over B*nW*L*hw rows: the plain streaming copy that
         moves the bytes of (a)
   each timed with device events over `inner` back-to-back launches; reported: the median over
   rounds, the spread (max - min) / median, GB/s over the bytes the launch moves, and the ratio
   of (a) and (b) to (c) per byte moved.
2. The whole step: DenoiseLoop (graph replay) at the full config, CFG: F = 32 with FreeNoise(16, 4)
   off and on, and F = 64 on; ms per step and ms per frame.
Weights are random; no speed is promised.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "video-diffusion-experiments_amd")]

import torch  # noqa: E402

import vdiff  # noqa: E402
from vdiff import ops  # noqa: E402

BF16 = torch.bfloat16
B, F, L, S, TXT = 2, 32, 16, 4, 77
SHAPES = [(1024, 320), (256, 640), (64, 1280)]  # (hw, C)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us


def summary(xs, nbytes):
    med = statistics.median(xs)
    return {"median_us": round(med, 2), "spread": round((max(xs) - min(xs)) / med, 4), "bytes": nbytes,
            "gb_per_s": round(nbytes / med / 1e3, 1)}


def kernel_forms(hw, c, rounds, inner):
    g = torch.Generator(device="cuda").manual_seed(hw + c)
    starts, tail = ops.window_starts(F, L, S)
    nw = len(starts)
    x = torch.randn(B * F * hw, c, device="cuda", generator=g).to(BF16)
    win = torch.empty(B * nw * L * hw, c, device="cuda", dtype=BF16)
    out = torch.empty_like(x)
    cp = torch.empty_like(win)
    wt = torch.tensor([float(min(i + 1, L - i)) for i in range(L)], device="cuda")  # pyramid
    forms = {"a_gather_op4": lambda: ops.window_gather(x, B, F, hw, L, S, out=win),
             "b_merge_op5": lambda: ops.window_merge(win, wt, B, F, hw, L, S, out=out),
             "c_copy_op0": lambda: ops.rows_add(None, win, out=cp)}
    for f in forms.values():  # warm-up
        timed(f, 3)
    assert torch.equal(out, x)  # merge(gather(x)) == x for integer weights
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            t[k].append(timed(f, inner))
    row = c * 2
    # F = 32 has no tail window: the merge reads every window row once
    win_rows, out_rows = B * nw * L * hw, B * F * hw
    nbytes = {"a_gather_op4": 2 * win_rows * row, "b_merge_op5": (win_rows + out_rows) * row,
              "c_copy_op0": 2 * win_rows * row}
    rec = {"hw": hw, "C": c, "B": B, "F": F, "L": L, "s": S, "windows": nw, "tail_len": tail,
           **{k: summary(v, nbytes[k]) for k, v in t.items()}}
    per_byte = {k: rec[k]["median_us"] / nbytes[k] for k in forms}
    rec["gather_vs_copy_per_byte"] = round(per_byte["a_gather_op4"] / per_byte["c_copy_op0"], 3)
    rec["merge_vs_copy_per_byte"] = round(per_byte["b_merge_op5"] / per_byte["c_copy_op0"], 3)
    return rec


def whole_step(rounds, steps):
    pipe = vdiff.AnimateDiffPipeline.from_config("full", device="cuda", vae=None)
    unet = pipe.unet
    s = unet.config["sample_size"]
    ehs = torch.randn(2, TXT, unet.config["cross_attention_dim"])
    pipe.scheduler.set_timesteps(50)
    lat = {f: torch.randn(1, unet.config["in_channels"], f, s, s) for f in (32, 64)}
    loops = {"f32_off": vdiff.DenoiseLoop(unet, pipe.scheduler, lat[32], ehs, 7.5).prime()}
    pipe.enable_free_noise(context_length=L, context_stride=S)  # stays enabled: the graphs read the weight tables
    loops["f32_on"] = vdiff.DenoiseLoop(unet, pipe.scheduler, lat[32], ehs, 7.5).prime()
    loops["f64_on"] = vdiff.DenoiseLoop(unet, pipe.scheduler, lat[64], ehs, 7.5).prime()
    frames = {"f32_off": 32, "f32_on": 32, "f64_on": 64}
    t = {k: [] for k in loops}
    for lp in loops.values():
        lp.run(1)
    for _ in range(rounds):
        for k, lp in loops.items():
            lp.reset(lat[frames[k]].to("cuda", torch.float32))
            t[k].append(timed(lambda lp=lp: lp.run(1), steps) / 1e3)  # ms per step
    rec = {}
    for k, v in t.items():
        med = statistics.median(v)
        rec[k] = {"frames": frames[k], "median_ms_per_step": round(med, 3), "ms_per_frame": round(med / frames[k], 3),
                  "spread": round((max(v) - min(v)) / med, 4), "graph": loops[k].graph is not None}
    rec["added_ms_per_step_f32"] = round(rec["f32_on"]["median_ms_per_step"] - rec["f32_off"]["median_ms_per_step"], 3)
    rec["free_noise"] = {"context_length": L, "context_stride": S, "weighting_scheme": "pyramid"}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "free_noise_bench.json"))
    args = ap.parse_args()
    rec = {"metric": "FreeNoise: window gather / merge (us per launch, GB/s, ratio to a plain copy per byte) and "
                     "ms per step of the windowed full step",
           "weights": "random", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inner": args.inner,
           "kernels": []}
    for hw, c in SHAPES:
        rec["kernels"].append(kernel_forms(hw, c, args.rounds, args.inner))
        print(f"[free_noise_bench] hw {hw} C {c} done", file=sys.stderr, flush=True)
    if not args.skip_step:
        rec["step"] = whole_step(args.rounds, args.steps)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
