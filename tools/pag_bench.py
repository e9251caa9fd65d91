"""Perturbed-attention guidance benchmark: denoising steps/s of the PAG loops beside the plain
ones at bench.py's own shape (full config, 16 frames, 64 x 64 latents, DDIM, one hipGraph replay
per step), bf16, 1x MI355X.  Recorded, not gated.

    python tools/pag_bench.py [--rounds 5] [--steps 20] [--warmup 3] [--out profiles/pag_bench.json]

Four captured DenoiseLoops on one model, interleaved round by round, each round `steps` replays
timed with device events (after `warmup` untimed replays per loop):
  cfg        guidance 7.5, no PAG: the UNet on 2 branches (bench.py's headline loop)
  cfg_pag    guidance 7.5 + PAG:   3 branches [uncond; cond; perturbed]
  nocfg      guidance 1, no PAG:   1 branch
  nocfg_pag  guidance 1 + PAG:     2 branches [cond; perturbed]
PAG uses the default layers ("mid_block.*attn1") and a constant scale 3.0.  Reported per loop: the
median steps/s and ms per step over the rounds and the spread (max - min) / median; and the
ratios of step time, cfg_pag / cfg (the untested guess is 1.5) and nocfg_pag / nocfg (2.0), and
nocfg_pag / cfg (both run two branches: what the identity layers and the lost CFG dedup cost).
Weights are random; no statement about image quality is made.
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
from vdiff.weights import materialize_synthetic  # noqa: E402

FRAMES, L = 16, 77
LAYERS = "mid_block.*attn1"
ARMS = {"cfg": (7.5, False), "cfg_pag": (7.5, True), "nocfg": (1.0, False), "nocfg_pag": (1.0, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="full", choices=["full", "tiny"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pag_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pag_bench: no GPU (there is no CPU path to time)")
    unet = materialize_synthetic(args.config, device="cuda", seed=0)
    unet.prepare()
    marked = unet.set_pag_applied_layers(LAYERS)
    # bench.py's inputs
    lat = torch.randn((1, 4, FRAMES, 64, 64), generator=torch.Generator().manual_seed(42))
    ehs = torch.randn((2, L, unet.config["cross_attention_dim"]), generator=torch.Generator().manual_seed(1))
    sched = vdiff.DDIMScheduler.from_config(vdiff.DDIMScheduler().config, beta_schedule="linear", steps_offset=1,
                                            clip_sample=False)
    sched.set_timesteps(50)
    per_loop = args.warmup + args.rounds * args.steps
    ts = sched.timesteps.repeat((per_loop + 49) // 50)[:max(per_loop, 50)]
    loops = {}
    for name, (g, pag) in ARMS.items():
        e = ehs if g > 1 else ehs[1:]
        if pag:
            e = torch.cat([e, ehs[1:]])
        loops[name] = vdiff.DenoiseLoop(unet, sched, lat.cuda(), e.cuda(), g, timesteps=ts,
                                        pag=vdiff.PerturbedAttentionGuidance(3.0) if pag else None).prime()
        loops[name].run(args.warmup)
        print(f"[pag_bench] {name}: graph={loops[name].graph is not None} branches={loops[name].ncfg}",
              file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    ms = {k: [] for k in ARMS}
    for _ in range(args.rounds):
        for name, lp in loops.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            lp.run(args.steps)
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / args.steps)
    for name, lp in loops.items():
        assert torch.isfinite(lp.lat).all(), f"{name}: non-finite latents"
    rec = {"metric": "PAG: denoising steps/s of the captured loop with and without perturbed-attention guidance",
           "config": f"{args.config}, {FRAMES} frames, 64x64 latents, DDIM, one hipGraph replay per step",
           "weights": "random", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "steps_per_round": args.steps, "warmup": args.warmup, "pag_applied_layers": LAYERS, "marked": marked,
           "pag_scale": 3.0, "loops": {}}
    for name, xs in ms.items():
        med = statistics.median(xs)
        rec["loops"][name] = {"branches": loops[name].ncfg, "graph": loops[name].graph is not None,
                              "ms_per_step": round(med, 3), "steps_per_s": round(1e3 / med, 4),
                              "spread": round((max(xs) - min(xs)) / med, 4)}
    m = {k: v["ms_per_step"] for k, v in rec["loops"].items()}
    rec["cfg_pag_over_cfg_step_time"] = round(m["cfg_pag"] / m["cfg"], 4)
    rec["nocfg_pag_over_nocfg_step_time"] = round(m["nocfg_pag"] / m["nocfg"], 4)
    rec["nocfg_pag_over_cfg_step_time"] = round(m["nocfg_pag"] / m["cfg"], 4)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
