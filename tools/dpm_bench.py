"""DPM-Solver++ benchmark: the multistep step kernel beside the DDIM one, and a 25-step DPM++ 2M
Karras video beside the 50-step DDIM video, bf16, 1x MI355X.  Recorded, not gated.

    python tools/dpm_bench.py [--rounds 7] [--inner 50] [--videos 3] [--skip-video]
                              [--out profiles/dpm_bench.json]

1. Kernel: vd_ddim_cfg_step with and without VD_STEP_DPM at the workload's latent shape
   (1, 4, 16, 64, 64), ncfg = 2, writing next_in, as the captured step launches it: the DDIM
   update, the deterministic DPM-Solver++ update on a second-order row (it reads and writes the
   history), and the SDE one (it also reads a noise slab).  The forms are interleaved round by
   round, each timed with device events over `inner` back-to-back launches (a launch-to-launch
   time, not a profiler's kernel time); reported: the median over rounds, the spread
   (max - min) / median, the bytes each must move (from the shapes) and the ratios to DDIM.
2. Video: on the full synthetic config at 16 frames and guidance 7.5, a 25-step DPM++ 2M Karras
   run and a 50-step DDIM run, in one session, interleaved: the primed loop's run() over its whole
   schedule (device events), and the whole pipe(...) call to latents (host clock around a
   synchronise; it builds and captures its loop every call).
Weights are random; no speed is promised, and no statement about image quality is made.
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

SHAPE = (1, 4, 16, 64, 64)
CPAD, L = 8, 77
GUIDANCE = 7.5
DPM = dict(steps=25, guidance=GUIDANCE)
DDIM = dict(steps=50, guidance=GUIDANCE)


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


def dpm_scheduler(algorithm_type="dpmsolver++"):
    return vdiff.DPMSolverMultistepScheduler.from_config(vdiff.DDIMScheduler().config, algorithm_type=algorithm_type,
                                                         use_karras_sigmas=True)


def ddim_scheduler():
    return vdiff.DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)


def kernels(rounds, inner):
    g = torch.Generator(device="cuda").manual_seed(0)
    B, C, Fr, H, W = SHAPE
    rows, numel = B * Fr * H * W, B * C * Fr * H * W
    eps = torch.randn(2 * rows, C, device="cuda", generator=g)
    lat = torch.randn(SHAPE, device="cuda", generator=g)
    hist = torch.randn(SHAPE, device="cuda", generator=g)
    nxt = torch.empty(2 * rows, CPAD, device="cuda", dtype=torch.bfloat16)
    zero = torch.zeros(1, device="cuda", dtype=torch.int32)
    mid = torch.full((1,), DPM["steps"] // 2, device="cuda", dtype=torch.int32)  # a second-order row
    d, s, e = ddim_scheduler(), dpm_scheduler(), dpm_scheduler("sde-dpmsolver++")
    d.set_timesteps(DDIM["steps"])
    n = DPM["steps"]
    s.set_timesteps(n)
    e.set_timesteps(n)
    d_coef = d.coefficient_table().cuda()
    s_coef = s.coefficient_table().cuda()
    assert int(s_coef[n // 2, 7].item()) == 1
    e_coef = torch.randn(ops.dpm_buffer_numel(n, numel, True), device="cuda", generator=g)
    e_coef[:ops.DPM_ROW * n].copy_(e.coefficient_table().reshape(-1))
    forms = {"ddim": lambda: ops.ddim_cfg_step(eps, 2, GUIDANCE, lat, d_coef, step_idx=zero, next_in=nxt),
             "dpm_2m": lambda: ops.dpm_cfg_step(eps, 2, GUIDANCE, lat, s_coef, step_idx=mid, x0_out=hist, next_in=nxt),
             "dpm_2m_sde": lambda: ops.dpm_cfg_step(eps, 2, GUIDANCE, lat, e_coef, step_idx=mid, x0_out=hist,
                                                    next_in=nxt)}
    for f in forms.values():  # warm-up
        timed(f, 10)
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            lat.normal_(generator=g)  # the update is in place: keep the latents finite
            hist.normal_(generator=g)
            t[k].append(timed(f, inner))
    rec = {k: summary(v) for k, v in t.items()}
    common = numel * (2 * 4 + 4 + 4) + 2 * rows * CPAD * 2  # eps (both halves), latents r+w, next_in
    rec["ddim"]["bytes"] = common
    rec["dpm_2m"]["bytes"] = common + numel * 8        # the history, read and written
    rec["dpm_2m_sde"]["bytes"] = common + numel * 12   # and the noise slab
    for k in forms:
        rec[k]["gb_per_s"] = round(rec[k]["bytes"] / rec[k]["median_us"] / 1e3, 1)
    for k in ("dpm_2m", "dpm_2m_sde"):
        rec[f"{k}_over_ddim_time"] = round(rec[k]["median_us"] / rec["ddim"]["median_us"], 4)
        rec[f"{k}_over_ddim_bytes"] = round(rec[k]["bytes"] / rec["ddim"]["bytes"], 4)
    rec["shape"], rec["ncfg"] = list(SHAPE), 2
    return rec


def videos(pipe, n_videos):
    unet = pipe.unet
    lat = torch.randn(SHAPE)
    ehs = torch.randn(2, L, unet.config["cross_attention_dim"])
    neg, pos = ehs.chunk(2)
    arms = {"dpm_2m_karras_25_steps": (dpm_scheduler(), DPM), "ddim_50_steps": (ddim_scheduler(), DDIM)}
    loops = {}
    for k, (s, a) in arms.items():
        s.set_timesteps(a["steps"])
        loops[k] = vdiff.DenoiseLoop(unet, s, lat, ehs, a["guidance"]).prime()
        loops[k].run()  # warm-up: every replay of the schedule once
    t_loop, t_call = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(n_videos):
        for k, lp in loops.items():
            lp.reset(lat.cuda())
            t_loop[k].append(timed(lp.run, 1) / 1e3)  # ms per video
    for i in range(n_videos + 1):  # the first call of each arm is warm-up
        for k, (s, a) in arms.items():
            pipe.scheduler = s
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe(prompt_embeds=pos, negative_prompt_embeds=neg, num_frames=SHAPE[2], num_inference_steps=a["steps"],
                 guidance_scale=a["guidance"], generator=torch.manual_seed(0), output_type="latent")
            torch.cuda.synchronize()
            if i:
                t_call[k].append((time.perf_counter() - t0) * 1e3)
    rec = {k: {"denoise_loop": summary(t_loop[k], "ms"), "pipeline_call_to_latents": summary(t_call[k], "ms"),
               "ms_per_step": round(statistics.median(t_loop[k]) / arms[k][1]["steps"], 3),
               "graph": loops[k].graph is not None, **arms[k][1]} for k in arms}
    a, b = rec["dpm_2m_karras_25_steps"], rec["ddim_50_steps"]
    rec["dpm_over_ddim_denoise_loop"] = round(a["denoise_loop"]["median_ms"] / b["denoise_loop"]["median_ms"], 4)
    rec["dpm_over_ddim_pipeline_call"] = round(a["pipeline_call_to_latents"]["median_ms"]
                                               / b["pipeline_call_to_latents"]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--videos", type=int, default=3)
    ap.add_argument("--skip-video", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dpm_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dpm_bench: no GPU (there is no CPU path to time)")
    rec = {"metric": "DPM-Solver++: step kernel (us per launch), 25-step DPM++ 2M Karras vs 50-step DDIM video (ms)",
           "config": "full, 16 frames, 64x64 latents", "weights": "random", "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "inner": args.inner, "kernel": kernels(args.rounds, args.inner)}
    print("[dpm_bench] kernels done", file=sys.stderr, flush=True)
    if not args.skip_video:
        pipe = vdiff.AnimateDiffPipeline.from_config("full", device="cuda", vae=None)
        rec["video"] = videos(pipe, args.videos)
        print("[dpm_bench] videos done", file=sys.stderr, flush=True)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
