"""FreeNoise prompt-travel benchmark: the per-step time of a captured denoising loop with per-frame
text beside the same loop with per-video text, and the interpolation launch (vd_rows_eltwise op 9),
bf16, 1x MI355X.  Recorded, not gated.

    python tools/prompt_travel_bench.py [--rounds 7] [--inner 50] [--videos 5] [--steps 25] [--skip-video]
                                        [--out profiles/prompt_travel_bench.json]

1. Kernel: ops.prompt_lerp at 2 videos x 64 frames x 77 tokens x 768 columns from 3 key prompts per
   video at frames [0, 20, 63], timed with device events over `inner` back-to-back launches (a
   launch-to-launch time, not a profiler's kernel time; the wrapper's small index upload is in it);
   reported: the median over rounds, the spread (max - min) / median, and the bytes the launch must
   move (from the shapes: every output row written, two key rows read per interpolated row, one per
   key frame) over that time.
2. Loop: on the full synthetic config at 16 frames, 64 x 64 latents, DDIM, guidance 7.5, the primed
   loop's run() over its whole schedule (device events), the arms interleaved in one process after a
   warm-up run of each: per-video text (a), per-frame text (x), per-video text again (b).  The
   per-frame text is 16 distinct [77, dim] entries per video and guidance half, so the spatial
   cross-attentions read 77 K/V rows per frame where the per-video form reads 77 per video.
   Reported per arm: the median over the repeated replays divided by the step count; and the
   difference x - (a + b) / 2 beside |a - b|, the run-to-run spread.
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
L = 77
GUIDANCE = 7.5
LERP = dict(B=2, F=64, idx=[0, 20, 63], C=768)


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


def kernel(rounds, inner):
    B, F, idx, C = LERP["B"], LERP["F"], LERP["idx"], LERP["C"]
    K = len(idx)
    g = torch.Generator(device="cuda").manual_seed(0)
    keys = torch.randn(B * K * L, C, device="cuda", generator=g).to(torch.bfloat16)
    out = torch.empty(B * F * L, C, device="cuda", dtype=torch.bfloat16)
    fn = lambda: ops.prompt_lerp(keys, idx, B, F, L, out=out)  # noqa: E731
    timed(fn, 10)  # warm-up
    rec = summary([timed(fn, inner) for _ in range(rounds)])
    row = L * C * 2
    rec["bytes"] = B * (F * row + (2 * (F - K) + K) * row)  # written; read
    rec["gb_per_s"] = round(rec["bytes"] / rec["median_us"] / 1e3, 1)
    rec.update(videos=B, frames=F, tokens=L, columns=C, key_frames=idx)
    return rec


def loops(unet, n_videos, steps):
    B, _, Fr, _, _ = SHAPE
    D = unet.config["cross_attention_dim"]
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(SHAPE, generator=g)
    per_video = torch.randn(2 * B, L, D, generator=g)
    per_frame = torch.randn(2 * B * Fr, L, D, generator=g)
    arms = {"per_video_a": per_video, "per_frame": per_frame, "per_video_b": per_video}
    built = {}
    for k, ehs in arms.items():
        s = vdiff.DDIMScheduler(beta_schedule="linear", steps_offset=1, clip_sample=False)
        s.set_timesteps(steps)
        built[k] = vdiff.DenoiseLoop(unet, s, lat, ehs, GUIDANCE).prime()
        built[k].run()  # warm-up: every replay of the schedule once
        print(f"[prompt_travel_bench] {k} primed", file=sys.stderr, flush=True)
    x = lat.cuda()
    t = {k: [] for k in arms}
    for _ in range(n_videos):
        for k, lp in built.items():
            lp.reset(x)
            t[k].append(timed(lp.run, 1) / 1e3)  # ms per schedule
    rec = {k: {"denoise_loop": summary(t[k], "ms"), "ms_per_step": round(statistics.median(t[k]) / steps, 4),
               "steps": steps, "guidance": GUIDANCE, "graph": built[k].graph is not None,
               "text_rows": int(built[k].ehs_rows.shape[0]),
               "kv_cache_mb": round(sum(v.numel() * v.element_size() for v in built[k].kv_cache.values()) / 1e6, 2)}
           for k in arms}
    a, b = rec["per_video_a"]["ms_per_step"], rec["per_video_b"]["ms_per_step"]
    rec["per_video_ms_per_step"] = round((a + b) / 2, 4)
    rec["per_video_repeat_spread_ms_per_step"] = round(abs(a - b), 4)
    rec["per_frame_ms_per_step"] = rec["per_frame"]["ms_per_step"]
    rec["per_frame_minus_per_video_ms_per_step"] = round(rec["per_frame_ms_per_step"] - (a + b) / 2, 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--videos", type=int, default=5)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--skip-video", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prompt_travel_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prompt_travel_bench: no GPU (there is no CPU path to time)")
    rec = {"metric": "FreeNoise prompt travel: op 9 (us per launch) and the captured-loop step (ms) with per-frame "
                     "text beside per-video text",
           "config": "full, 16 frames, 64x64 latents, DDIM", "weights": "random",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inner": args.inner, "videos": args.videos,
           "kernel": kernel(args.rounds, args.inner)}
    print("[prompt_travel_bench] kernel done", file=sys.stderr, flush=True)
    if not args.skip_video:
        pipe = vdiff.AnimateDiffPipeline.from_config("full", device="cuda", vae=None)
        rec["loop"] = loops(pipe.unet, args.videos, args.steps)
        print("[prompt_travel_bench] loops done", file=sys.stderr, flush=True)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
