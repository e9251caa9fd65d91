"""LCM benchmark: the LCM step kernel beside the DDIM one, a 6-step LCM video beside the 25-step
DDIM video, and what a LoRA switch costs, bf16, 1x MI355X.

    python tools/lcm_bench.py [--rounds 7] [--inner 50] [--videos 3] [--skip-video] [--skip-lora]
                              [--out profiles/lcm_bench.json]

1. Kernel: vd_ddim_cfg_step with and without VD_STEP_LCM at the workload's latent shape
   (1, 4, 16, 64, 64), ncfg = 2, writing next_in, as the captured step launches it.  The two are
   interleaved round by round, each timed with device events over `inner` back-to-back launches
   (so the figure is a launch-to-launch time, not a profiler's kernel time); reported: the median
   over rounds, the spread (max - min) / median, the bytes each must move (from the shapes) and
   the LCM / DDIM ratio.  The LCM kernel reads one more fp32 per element, the noise.
2. Video: on the full synthetic config at 16 frames, a 6-step guidance 2.0 LCM run and the
   25-step guidance 7.5 DDIM run of the benchmark, in one session, interleaved: the primed loop's
   run() over its whole schedule (device events), and the whole pipe(...) call to latents (host
   clock around a synchronise; it builds and captures its loop every call).
3. LoRA: a rank-8 LoRA on every attention projection of the full config; the time of
   set_adapters (CPU merge of the touched weights + the full prepare() re-pack) and of the
   prepare() re-pack alone.
Weights are random; no speed is promised.
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
LCM = dict(steps=6, guidance=2.0)
DDIM = dict(steps=25, guidance=7.5)


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


def lcm_scheduler():
    return vdiff.LCMScheduler.from_config(None, beta_schedule="linear")


def ddim_scheduler():
    return vdiff.DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)


def kernels(rounds, inner):
    g = torch.Generator(device="cuda").manual_seed(0)
    B, C, Fr, H, W = SHAPE
    rows, numel = B * Fr * H * W, B * C * Fr * H * W
    eps = torch.randn(2 * rows, C, device="cuda", generator=g)
    lat = torch.randn(SHAPE, device="cuda", generator=g)
    nxt = torch.empty(2 * rows, CPAD, device="cuda", dtype=torch.bfloat16)
    step = torch.zeros(1, device="cuda", dtype=torch.int32)
    d, s = ddim_scheduler(), lcm_scheduler()
    d.set_timesteps(DDIM["steps"])
    s.set_timesteps(LCM["steps"])
    d_coef = d.coefficient_table().cuda()
    n = LCM["steps"]
    s_coef = torch.randn(ops.lcm_buffer_numel(n, numel), device="cuda", generator=g)
    s_coef[:ops.LCM_ROW * n].copy_(s.coefficient_table().reshape(-1))
    forms = {"ddim": lambda: ops.ddim_cfg_step(eps, 2, 7.5, lat, d_coef, step_idx=step, next_in=nxt),
             "lcm": lambda: ops.lcm_cfg_step(eps, 2, 2.0, lat, s_coef, step_idx=step, next_in=nxt)}
    for f in forms.values():  # warm-up
        timed(f, 10)
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            lat.normal_(generator=g)  # the update is in place: keep the latents finite
            t[k].append(timed(f, inner))
    rec = {k: summary(v) for k, v in t.items()}
    common = numel * (2 * 4 + 4 + 4) + 2 * rows * CPAD * 2  # eps (both halves), latents r+w, next_in
    rec["ddim"]["bytes"], rec["lcm"]["bytes"] = common, common + numel * 4
    for k in forms:
        rec[k]["gb_per_s"] = round(rec[k]["bytes"] / rec[k]["median_us"] / 1e3, 1)
    rec["lcm_over_ddim_time"] = round(rec["lcm"]["median_us"] / rec["ddim"]["median_us"], 4)
    rec["lcm_over_ddim_bytes"] = round(rec["lcm"]["bytes"] / rec["ddim"]["bytes"], 4)
    rec["shape"], rec["ncfg"] = list(SHAPE), 2
    return rec


def videos(pipe, n_videos):
    unet = pipe.unet
    lat = torch.randn(SHAPE)
    ehs = torch.randn(2, L, unet.config["cross_attention_dim"])
    neg, pos = ehs.chunk(2)
    arms = {"lcm_6_steps_g2": (lcm_scheduler(), LCM), "ddim_25_steps_g7.5": (ddim_scheduler(), DDIM)}
    loops = {}
    for k, (s, a) in arms.items():
        s.set_timesteps(a["steps"])
        noise = torch.randn((a["steps"] - 1,) + SHAPE) if s.kind == "lcm" else None
        loops[k] = vdiff.DenoiseLoop(unet, s, lat, ehs, a["guidance"], step_noise=noise).prime()
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
               "graph": loops[k].graph is not None, **arms[k][1]} for k in arms}
    a, b = rec["lcm_6_steps_g2"], rec["ddim_25_steps_g7.5"]
    rec["lcm_over_ddim_denoise_loop"] = round(a["denoise_loop"]["median_ms"] / b["denoise_loop"]["median_ms"], 4)
    rec["lcm_over_ddim_pipeline_call"] = round(a["pipeline_call_to_latents"]["median_ms"]
                                               / b["pipeline_call_to_latents"]["median_ms"], 4)
    return rec


def lora_switch(pipe, rounds):
    from vdiff import lora
    unet = pipe.unet
    g = torch.Generator().manual_seed(0)
    sd, r = {}, 8
    for name, m in lora.target_modules(unet).items():
        if name.rsplit(".", 1)[-1] in ("to_q", "to_k", "to_v") or name.endswith(".to_out.0"):
            sd[f"unet.{name}.lora_A.weight"] = torch.randn(r, m.weight.shape[1], generator=g) * 0.01
            sd[f"unet.{name}.lora_B.weight"] = torch.randn(m.weight.shape[0], r, generator=g) * 0.01
    t0 = time.perf_counter()
    pipe.load_lora_weights(sd, adapter_name="bench")
    torch.cuda.synchronize()
    t_load = time.perf_counter() - t0
    t_set, t_prep = [], []
    for i in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.set_adapters("bench", 0.5 + 0.1 * i)
        torch.cuda.synchronize()
        t_set.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        unet.prepare()
        torch.cuda.synchronize()
        t_prep.append(time.perf_counter() - t0)
    pipe.unload_lora_weights()
    return {"modules": len(sd) // 2, "rank": r, "parameters_touched": sum(
                lora.target_modules(unet)[k[len("unet."):-len(".lora_A.weight")]].weight.numel()
                for k in sd if k.endswith(".lora_A.weight")),
            "load_lora_weights_s": round(t_load, 3), "set_adapters": summary(t_set, "s"),
            "prepare_repack_alone": summary(t_prep, "s")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--videos", type=int, default=3)
    ap.add_argument("--skip-video", action="store_true")
    ap.add_argument("--skip-lora", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lcm_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lcm_bench: no GPU (there is no CPU path to time)")
    rec = {"metric": "LCM: step kernel (us per launch), 6-step LCM vs 25-step DDIM video (ms), LoRA switch (s)",
           "config": "full, 16 frames, 64x64 latents", "weights": "random", "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "inner": args.inner, "kernel": kernels(args.rounds, args.inner)}
    print("[lcm_bench] kernels done", file=sys.stderr, flush=True)
    if not (args.skip_video and args.skip_lora):
        pipe = vdiff.AnimateDiffPipeline.from_config("full", device="cuda", vae=None)
        if not args.skip_video:
            rec["video"] = videos(pipe, args.videos)
            print("[lcm_bench] videos done", file=sys.stderr, flush=True)
        if not args.skip_lora:
            rec["lora"] = lora_switch(pipe, min(args.rounds, 3))
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
