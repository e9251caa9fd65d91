"""UniPC benchmark: the predictor-corrector step kernel beside the DPM-Solver++ one, and UniPC
videos at 10, 15 and 20 steps beside a 25-step DPM++ 2M Karras video and a 50-step DDIM video, bf16,
1x MI355X.  Recorded, not gated.

    python tools/unipc_bench.py [--rounds 7] [--inner 50] [--videos 3] [--skip-video]
                                [--out profiles/unipc_bench.json]

1. Kernel: vd_ddim_cfg_step at the workload's latent shape (1, 4, 16, 64, 64), ncfg = 2, writing
   next_in, as the captured step launches it: the DDIM update, the deterministic DPM-Solver++ update
   on a second-order row (one history slab in and out) and the UniPC update on a row with a
   second-order corrector and predictor (three state slabs in and out).  The forms are interleaved
   round by round, each timed with device events over `inner` back-to-back launches (a
   launch-to-launch time, not a profiler's kernel time); reported: the median over rounds, the
   spread (max - min) / median, the bytes each must move (from the shapes) and the ratios to DPM.
2. Video: on the full synthetic config at 16 frames and guidance 7.5, the primed loop's run() over
   its whole schedule (device events), the arms interleaved in one session: DPM-25 (a), UniPC-10,
   UniPC-15, UniPC-20, DPM-25 again (b) and DDIM-50.  The acceptance is relative: a loop step under
   UniPC may take longer than one under DPM by no more than the two DPM arms differ,
     unipc_ms_per_step - dpm_ms_per_step <= dpm_repeat_spread_ms_per_step
   with dpm_ms_per_step the mean of the two DPM arms' medians; all three figures and the verdict
   are written out.
Weights are random; no speed is promised, and no statement about image quality is made: fewer steps
are faster by construction, what they do to a video is not measured here.
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
UNIPC_STEPS = (10, 15, 20)
DPM_STEPS, DDIM_STEPS = 25, 50


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


def unipc_scheduler():
    return vdiff.UniPCMultistepScheduler.from_config(vdiff.DDIMScheduler().config, use_karras_sigmas=True)


def dpm_scheduler():
    return vdiff.DPMSolverMultistepScheduler.from_config(vdiff.DDIMScheduler().config, use_karras_sigmas=True)


def ddim_scheduler():
    return vdiff.DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)


def kernels(rounds, inner):
    g = torch.Generator(device="cuda").manual_seed(0)
    B, C, Fr, H, W = SHAPE
    rows, numel = B * Fr * H * W, B * C * Fr * H * W
    eps = torch.randn(2 * rows, C, device="cuda", generator=g)
    lat = torch.randn(SHAPE, device="cuda", generator=g)
    hist = torch.randn(SHAPE, device="cuda", generator=g)
    state = torch.randn((3,) + SHAPE, device="cuda", generator=g)
    nxt = torch.empty(2 * rows, CPAD, device="cuda", dtype=torch.bfloat16)
    zero = torch.zeros(1, device="cuda", dtype=torch.int32)
    d, s, u = ddim_scheduler(), dpm_scheduler(), unipc_scheduler()
    d.set_timesteps(DDIM_STEPS)
    s.set_timesteps(DPM_STEPS)
    u.set_timesteps(UNIPC_STEPS[-1])
    mid_s = torch.full((1,), DPM_STEPS // 2, device="cuda", dtype=torch.int32)       # a second-order row
    # a row whose corrector and predictor are both second order
    mid_u = torch.full((1,), UNIPC_STEPS[-1] // 2, device="cuda", dtype=torch.int32)
    d_coef, s_coef, u_coef = (x.coefficient_table().cuda() for x in (d, s, u))
    assert int(s_coef[DPM_STEPS // 2, 7].item()) == 1 and int(u_coef[UNIPC_STEPS[-1] // 2, 12].item()) == 7
    forms = {"ddim": lambda: ops.ddim_cfg_step(eps, 2, GUIDANCE, lat, d_coef, step_idx=zero, next_in=nxt),
             "dpm_2m": lambda: ops.dpm_cfg_step(eps, 2, GUIDANCE, lat, s_coef, step_idx=mid_s, x0_out=hist, next_in=nxt),
             "unipc": lambda: ops.unipc_cfg_step(eps, 2, GUIDANCE, lat, u_coef, step_idx=mid_u, x0_out=state,
                                                 next_in=nxt)}
    for f in forms.values():  # warm-up
        timed(f, 10)
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            lat.normal_(generator=g)  # the updates are in place: keep latents and state finite
            hist.normal_(generator=g)
            state.normal_(generator=g)
            t[k].append(timed(f, inner))
    rec = {k: summary(v) for k, v in t.items()}
    common = numel * (2 * 4 + 4 + 4) + 2 * rows * CPAD * 2  # eps (both halves), latents r+w, next_in
    rec["ddim"]["bytes"] = common
    rec["dpm_2m"]["bytes"] = common + numel * 8       # the history, read and written
    rec["unipc"]["bytes"] = common + numel * 24       # three state slabs, read and written
    for k in forms:
        rec[k]["gb_per_s"] = round(rec[k]["bytes"] / rec[k]["median_us"] / 1e3, 1)
    rec["unipc_over_dpm_time"] = round(rec["unipc"]["median_us"] / rec["dpm_2m"]["median_us"], 4)
    rec["unipc_over_dpm_bytes"] = round(rec["unipc"]["bytes"] / rec["dpm_2m"]["bytes"], 4)
    rec["unipc_over_ddim_time"] = round(rec["unipc"]["median_us"] / rec["ddim"]["median_us"], 4)
    rec["shape"], rec["ncfg"] = list(SHAPE), 2
    return rec


def videos(unet, n_videos):
    lat = torch.randn(SHAPE)
    ehs = torch.randn(2, L, unet.config["cross_attention_dim"])
    arms = {"dpm_2m_karras_25_steps_a": (dpm_scheduler(), DPM_STEPS)}
    for n in UNIPC_STEPS:
        arms[f"unipc_karras_{n}_steps"] = (unipc_scheduler(), n)
    arms["dpm_2m_karras_25_steps_b"] = (dpm_scheduler(), DPM_STEPS)
    arms["ddim_50_steps"] = (ddim_scheduler(), DDIM_STEPS)
    loops = {}
    for k, (s, n) in arms.items():
        s.set_timesteps(n)
        loops[k] = vdiff.DenoiseLoop(unet, s, lat, ehs, GUIDANCE).prime()
        loops[k].run()  # warm-up: every replay of the schedule once
        print(f"[unipc_bench] {k} primed", file=sys.stderr, flush=True)
    t = {k: [] for k in arms}
    for _ in range(n_videos):
        for k, lp in loops.items():
            lp.reset(lat.cuda())
            t[k].append(timed(lp.run, 1) / 1e3)  # ms per video
    rec = {k: {"denoise_loop": summary(t[k], "ms"), "seconds_per_video": round(statistics.median(t[k]) / 1e3, 4),
               "ms_per_step": round(statistics.median(t[k]) / arms[k][1], 4), "steps": arms[k][1],
               "guidance": GUIDANCE, "graph": loops[k].graph is not None} for k in arms}
    a, b = rec["dpm_2m_karras_25_steps_a"]["ms_per_step"], rec["dpm_2m_karras_25_steps_b"]["ms_per_step"]
    u = statistics.median(rec[f"unipc_karras_{n}_steps"]["ms_per_step"] for n in UNIPC_STEPS)
    rec["dpm_ms_per_step"] = round((a + b) / 2, 4)
    rec["dpm_repeat_spread_ms_per_step"] = round(abs(a - b), 4)
    rec["unipc_ms_per_step"] = round(u, 4)
    rec["unipc_step_within_dpm_repeat_spread"] = bool(u - (a + b) / 2 <= abs(a - b))
    dpm_s = sum(rec[f"dpm_2m_karras_25_steps_{x}"]["seconds_per_video"] for x in "ab") / 2
    for n in UNIPC_STEPS:
        sv = rec[f"unipc_karras_{n}_steps"]["seconds_per_video"]
        rec[f"unipc_{n}_over_dpm_25_seconds"] = round(sv / dpm_s, 4)
        rec[f"unipc_{n}_over_ddim_50_seconds"] = round(sv / rec["ddim_50_steps"]["seconds_per_video"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--videos", type=int, default=3)
    ap.add_argument("--skip-video", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "unipc_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unipc_bench: no GPU (there is no CPU path to time)")
    rec = {"metric": "UniPC: step kernel (us per launch); UniPC 10/15/20-step vs 25-step DPM++ 2M Karras vs 50-step "
                     "DDIM video (denoise loop, seconds)",
           "config": "full, 16 frames, 64x64 latents", "weights": "random", "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "inner": args.inner, "kernel": kernels(args.rounds, args.inner)}
    print("[unipc_bench] kernels done", file=sys.stderr, flush=True)
    if not args.skip_video:
        pipe = vdiff.AnimateDiffPipeline.from_config("full", device="cuda", vae=None)
        rec["video"] = videos(pipe.unet, args.videos)
        print("[unipc_bench] videos done", file=sys.stderr, flush=True)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
