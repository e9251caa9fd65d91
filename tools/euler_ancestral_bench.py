"""Euler-ancestral benchmark: the stochastic Euler step kernel beside the plain Euler one, and the
per-step time of a captured denoising loop with each scheduler, bf16, 1x MI355X.  Recorded, not gated.

    python tools/euler_ancestral_bench.py [--rounds 7] [--inner 50] [--videos 5] [--steps 25] [--skip-video]
                                          [--out profiles/euler_ancestral_bench.json]

1. Kernel: vd_euler_cfg_step at the workload's latent shape (1, 4, 16, 64, 64), ncfg = 2, writing
   next_in, as the captured step launches it: without VD_STEP_ANCESTRAL on an Euler table, and with it
   on a middle row of an Euler-ancestral table (sigma_up != 0: one extra fp32 read per latent element,
   from the step's noise slab).  The two forms are interleaved round by round, each timed with device
   events over `inner` back-to-back launches (a launch-to-launch time, not a profiler's kernel time);
   reported: the median over rounds, the spread (max - min) / median, the bytes each must move (from
   the shapes) and the ratios.
2. Loop: on the full synthetic config at 16 frames and guidance 7.5, the primed loop's run() over its
   whole schedule (device events), the arms interleaved in one process after a warm-up run of each:
   Euler (a), Euler ancestral, Euler again (b).  Reported per arm: the median over the repeated
   replays divided by the step count; and the difference ancestral - Euler (the mean of the two
   Euler arms) beside what the two Euler arms differ by, the run-to-run spread.
Weights are random; no speed is promised and no statement about image quality is made.
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

SHAPE = (1, 4, 16, 64, 64)
CPAD, L = 8, 77
GUIDANCE = 7.5


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us


def summary(xs, unit="us"):
    med = statistics.median(xs)
    return {f"median_{unit}": round(med, 3), "spread": round((max(xs) - min(xs)) / med, 4)}


def euler_scheduler():
    return vdiff.EulerDiscreteScheduler.from_config(vdiff.DDIMScheduler().config, timestep_spacing="linspace",
                                                    beta_schedule="linear")


def ancestral_scheduler():
    return vdiff.EulerAncestralDiscreteScheduler.from_config(euler_scheduler().config)


def kernels(rounds, inner, steps):
    g = torch.Generator(device="cuda").manual_seed(0)
    B, C, Fr, H, W = SHAPE
    rows, numel = B * Fr * H * W, B * C * Fr * H * W
    eps = torch.randn(2 * rows, C, device="cuda", generator=g)
    lat = torch.randn(SHAPE, device="cuda", generator=g)
    nxt = torch.empty(2 * rows, CPAD, device="cuda", dtype=torch.bfloat16)
    e, a = euler_scheduler(), ancestral_scheduler()
    e.set_timesteps(steps)
    a.set_timesteps(steps)
    mid = torch.full((1,), steps // 2, device="cuda", dtype=torch.int32)
    e_coef = e.coefficient_table().cuda()
    a_rows = a.coefficient_table()
    assert float(a_rows[steps // 2, 3]) != 0.0  # a row that reads its slab
    a_coef = torch.empty(ops.euler_a_buffer_numel(steps, numel), device="cuda")
    a_coef[:ops.EULER_A_ROW * steps].copy_(a_rows.reshape(-1))
    a_coef[ops.EULER_A_ROW * steps:].normal_(generator=g)
    forms = {"euler": lambda: ops.euler_cfg_step(eps, 2, GUIDANCE, lat, e_coef, step_idx=mid, next_in=nxt),
             "euler_ancestral": lambda: ops.euler_ancestral_cfg_step(eps, 2, GUIDANCE, lat, a_coef, step_idx=mid,
                                                                     next_in=nxt)}
    for f in forms.values():  # warm-up
        timed(f, 10)
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            lat.normal_(generator=g)  # the updates are in place: keep the latents finite
            t[k].append(timed(f, inner))
    rec = {k: summary(v) for k, v in t.items()}
    common = numel * (2 * 4 + 4 + 4) + 2 * rows * CPAD * 2  # eps (both halves), latents r+w, next_in
    rec["euler"]["bytes"] = common
    rec["euler_ancestral"]["bytes"] = common + numel * 4  # the step's noise slab, read
    for k in forms:
        rec[k]["gb_per_s"] = round(rec[k]["bytes"] / rec[k]["median_us"] / 1e3, 1)
    rec["ancestral_over_euler_time"] = round(rec["euler_ancestral"]["median_us"] / rec["euler"]["median_us"], 4)
    rec["ancestral_over_euler_bytes"] = round(rec["euler_ancestral"]["bytes"] / rec["euler"]["bytes"], 4)
    rec["ancestral_minus_euler_us"] = round(rec["euler_ancestral"]["median_us"] - rec["euler"]["median_us"], 3)
    rec["shape"], rec["ncfg"], rec["steps"] = list(SHAPE), 2, steps
    return rec


def loops(unet, n_videos, steps):
    lat = torch.randn(SHAPE)
    ehs = torch.randn(2, L, unet.config["cross_attention_dim"])
    noise = torch.randn((steps,) + SHAPE, generator=torch.Generator().manual_seed(1))
    arms = {"euler_a": (euler_scheduler(), None), "euler_ancestral": (ancestral_scheduler(), noise),
            "euler_b": (euler_scheduler(), None)}
    built = {}
    for k, (s, sn) in arms.items():
        s.set_timesteps(steps)
        x = lat * s.init_noise_sigma
        built[k] = (vdiff.DenoiseLoop(unet, s, x, ehs, GUIDANCE, step_noise=sn).prime(), x.cuda())
        built[k][0].run()  # warm-up: every replay of the schedule once
        print(f"[euler_ancestral_bench] {k} primed", file=sys.stderr, flush=True)
    t = {k: [] for k in arms}
    for _ in range(n_videos):
        for k, (lp, x) in built.items():
            lp.reset(x)
            t[k].append(timed(lp.run, 1) / 1e3)  # ms per schedule
    rec = {k: {"denoise_loop": summary(t[k], "ms"), "ms_per_step": round(statistics.median(t[k]) / steps, 4),
               "steps": steps, "guidance": GUIDANCE, "graph": built[k][0].graph is not None} for k in arms}
    a, b = rec["euler_a"]["ms_per_step"], rec["euler_b"]["ms_per_step"]
    rec["euler_ms_per_step"] = round((a + b) / 2, 4)
    rec["euler_repeat_spread_ms_per_step"] = round(abs(a - b), 4)
    rec["ancestral_ms_per_step"] = rec["euler_ancestral"]["ms_per_step"]
    rec["ancestral_minus_euler_ms_per_step"] = round(rec["ancestral_ms_per_step"] - (a + b) / 2, 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--videos", type=int, default=5)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--skip-video", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "euler_ancestral_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("euler_ancestral_bench: no GPU (there is no CPU path to time)")
    rec = {"metric": "Euler ancestral: step kernel (us per launch) and captured-loop step (ms) beside plain Euler",
           "config": "full, 16 frames, 64x64 latents", "weights": "random", "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "inner": args.inner, "videos": args.videos,
           "kernel": kernels(args.rounds, args.inner, args.steps)}
    print("[euler_ancestral_bench] kernels done", file=sys.stderr, flush=True)
    if not args.skip_video:
        pipe = vdiff.AnimateDiffPipeline.from_config("full", device="cuda", vae=None)
        rec["loop"] = loops(pipe.unet, args.videos, args.steps)
        print("[euler_ancestral_bench] loops done", file=sys.stderr, flush=True)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
