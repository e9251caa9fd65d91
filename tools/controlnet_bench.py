"""ControlNet benchmark: what a ControlNet adds to a denoising step, bf16, 1x MI355X.

    python tools/controlnet_bench.py [--rounds 7] [--inner 20] [--steps 3] [--skip-step] [--out profiles/controlnet_bench.json]

1. The whole step: DenoiseLoop (graph replay) at the full config, 16 frames, CFG, with and
   without a full-size ControlNet (361 M parameters, run on both guidance halves: 32 images), in
   one session, interleaved; the added ms per step.  Also guess mode, where the ControlNet sees
   the conditional half only (16 images).
2. The injection: the 13 vd_rows_eltwise op 7 launches of one step (ops.ctrl_add_: scale read on
   the device, one fused multiply-add, the skip updated in place) against the two-pass form on
   the same rows — op 3 (scale the residual in place) then op 0 (add it to the skip).
3. The one-off conditioning embedding: ControlNetModel.embed_condition on 16 frames of 512 x 512.
Each form is timed with device events over `inner` back-to-back runs, the forms interleaved
round by round; reported: the median over rounds and the spread (max - min) / median.
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
FRAMES, L = 16, 77


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us


def summary(xs, unit="us", scale=1.0):
    med = statistics.median(xs)
    return {f"median_{unit}": round(med * scale, 3), "spread": round((max(xs) - min(xs)) / med, 4)}


def build():
    unet = vdiff.weights.materialize_synthetic("full", device="cuda", seed=0).prepare()
    with torch.device("meta"):
        cn = vdiff.ControlNetModel("full")
    cn = cn.to_empty(device="cuda").to(dtype=BF16)
    vdiff.init_synthetic_(cn, seed=1, device="cuda")
    return unet, cn.prepare()


def whole_step(unet, cn, rounds, steps):
    s = unet.config["sample_size"]
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(1, unet.config["in_channels"], FRAMES, s, s, generator=g)
    ehs = torch.randn(2, L, unet.config["cross_attention_dim"], generator=g)
    cond = torch.rand(1, 3, FRAMES, 8 * s, 8 * s, generator=g)
    sched = vdiff.DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)
    sched.set_timesteps(50)
    loops = {"plain": vdiff.DenoiseLoop(unet, sched, lat, ehs, 7.5).prime(),
             "controlnet": vdiff.DenoiseLoop(unet, sched, lat, ehs, 7.5,
                                             control=vdiff.ControlNetConditioning(cn, cond)).prime(),
             "controlnet_guess_mode": vdiff.DenoiseLoop(
                 unet, sched, lat, ehs, 7.5, control=vdiff.ControlNetConditioning(cn, cond, guess_mode=True)).prime()}
    t = {k: [] for k in loops}
    for lp in loops.values():
        lp.run(2)
    for _ in range(rounds):
        for k, lp in loops.items():
            lp.reset(lat.to("cuda", torch.float32))
            t[k].append(timed(lambda lp=lp: lp.run(1), steps))
    rec = {k: summary(v, "ms", 1e-3) for k, v in t.items()}
    for k in ("controlnet", "controlnet_guess_mode"):
        rec[k]["added_ms_per_step"] = round(rec[k]["median_ms"] - rec["plain"]["median_ms"], 3)
    rec["graph"] = {k: lp.graph is not None for k, lp in loops.items()}
    return rec


def injection(unet, rounds, inner):
    """The 13 skips of the full config at 32 images of 64 x 64 latents."""
    shapes = unet.control_residual_shapes(2 * FRAMES, unet.config["sample_size"], unet.config["sample_size"])
    g = torch.Generator(device="cuda").manual_seed(3)
    acc = [torch.randn(r, c, device="cuda", generator=g).to(BF16) for r, c in shapes]
    res = [torch.randn(r, c, device="cuda", generator=g).to(BF16) for r, c in shapes]
    n = len(shapes)
    block, _ = ops.ctrl_block(torch.full((1, n), 0.5), "cuda")
    half = torch.tensor([0.5], device="cuda")

    def fused():
        for i in range(n):
            ops.ctrl_add_(acc[i], res[i], block, i, cols=n)

    def two_pass():
        for i in range(n):
            ops.scale_rows_(res[i], half)
            ops.rows_add(acc[i], res[i], out=acc[i])

    forms = {"op7_13_launches": fused, "op3_then_op0_26_launches": two_pass}
    for f in forms.values():
        timed(f, 3)
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            t[k].append(timed(f, inner))
    rec = {k: summary(v) for k, v in t.items()}
    elems = sum(r * c for r, c in shapes)
    rec["elements"] = elems
    rec["op7_13_launches"]["gb_per_s"] = round(3 * 2 * elems / rec["op7_13_launches"]["median_us"] / 1e3, 1)  # 2 reads + 1 write
    return rec


def embedding(cn, rounds):
    cond = torch.rand(1, 3, FRAMES, 512, 512, device="cuda")
    cn.embed_condition(cond)
    t = [timed(lambda: cn.embed_condition(cond), 2) for _ in range(rounds)]
    return {"frames": FRAMES, "height": 512, "width": 512, **summary(t, "ms", 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "controlnet_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("controlnet_bench needs the GPU: nothing is measured without one")
    unet, cn = build()
    rec = {"metric": "ControlNet: added ms per step, the 13 injections (us), the one-off embedding (ms)",
           "config": "full, 16 frames, 64 x 64 latents, CFG (32 images)", "weights": "random",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inner": args.inner,
           "controlnet_parameters": sum(p.numel() for p in cn.parameters())}
    rec["injection"] = injection(unet, args.rounds, args.inner)
    rec["embedding"] = embedding(cn, args.rounds)
    if not args.skip_step:
        rec["step"] = whole_step(unet, cn, args.rounds, args.steps)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
