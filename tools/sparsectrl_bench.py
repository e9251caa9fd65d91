"""SparseCtrl benchmark: what a SparseControlNetModel adds to a denoising step, bf16, 1x MI355X.

    python tools/sparsectrl_bench.py [--rounds 7] [--inner 20] [--steps 3] [--skip-step] [--out profiles/sparsectrl_bench.json]

1. The whole step: DenoiseLoop (graph replay) at the full config, 16 frames x 64 x 64 latents,
   CFG — plain, with a full-size SparseControlNetModel (its motion modules included, no conv_in)
   and with a full-size ControlNetModel, in one session, interleaved; the added ms per step.  Also
   guess mode, where the sparse ControlNet sees the conditional half only.
2. vd_rows_eltwise op 8 (ops.sparse_cond), once per video, at the two product shapes with F = 16
   and key frames at [0, 8, 15]: cc = 4, hw = 4096 (a 64 x 64 latent condition) and cc = 3,
   hw = 262144 (a 512 x 512 pixel condition); bytes moved = 16 per output row + 16 per row of a
   conditioned frame.
The method is tools/controlnet_bench.py's: device events over `inner` back-to-back runs, the forms
interleaved round by round; reported: the median over rounds and the spread (max - min) / median.
Weights are random; no speed is promised.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "video-diffusion-experiments_amd"), str(ROOT / "tools")]

import torch  # noqa: E402

import vdiff  # noqa: E402
from controlnet_bench import FRAMES, L, summary, timed  # noqa: E402
from vdiff import ops  # noqa: E402

BF16 = torch.bfloat16
IDX = [0, 8, 15]


def synthetic(cls, seed):
    with torch.device("meta"):
        m = cls("full")
    m = m.to_empty(device="cuda")
    for mod in m.modules():
        if hasattr(mod, "reset_buffers"):  # the motion modules' positional tables
            mod.reset_buffers()
    m = m.to(dtype=BF16)
    vdiff.init_synthetic_(m, seed=seed, device="cuda")
    return m.prepare()


def whole_step(unet, sparse, cn, rounds, steps):
    s = unet.config["sample_size"]
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(1, unet.config["in_channels"], FRAMES, s, s, generator=g)
    ehs = torch.randn(2, L, unet.config["cross_attention_dim"], generator=g)
    keys = ops.pack_latents(torch.randn(1, 4, len(IDX), s, s, generator=g).cuda(), dup=1, cpad=8)
    rows = ops.sparse_cond(keys, IDX, 1, FRAMES, s * s, 4)
    cond = torch.rand(1, 3, FRAMES, 8 * s, 8 * s, generator=g)
    sched = vdiff.DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)
    sched.set_timesteps(50)

    def sparse_ctl(guess):
        return vdiff.SparseControlConditioning(sparse, rows, 1, FRAMES, s, s, 1.0, guess)

    loops = {"plain": vdiff.DenoiseLoop(unet, sched, lat, ehs, 7.5).prime(),
             "sparsectrl": vdiff.DenoiseLoop(unet, sched, lat, ehs, 7.5, control=sparse_ctl(False)).prime(),
             "sparsectrl_guess_mode": vdiff.DenoiseLoop(unet, sched, lat, ehs, 7.5, control=sparse_ctl(True)).prime(),
             "controlnet": vdiff.DenoiseLoop(unet, sched, lat, ehs, 7.5,
                                             control=vdiff.ControlNetConditioning(cn, cond)).prime()}
    t = {k: [] for k in loops}
    for lp in loops.values():
        lp.run(2)
    for _ in range(rounds):
        for k, lp in loops.items():
            lp.reset(lat.to("cuda", torch.float32))
            t[k].append(timed(lambda lp=lp: lp.run(1), steps))
    rec = {k: summary(v, "ms", 1e-3) for k, v in t.items()}
    for k in loops:
        if k != "plain":
            rec[k]["added_ms_per_step"] = round(rec[k]["median_ms"] - rec["plain"]["median_ms"], 3)
    rec["graph"] = {k: lp.graph is not None for k, lp in loops.items()}
    return rec


def op8(rounds, inner):
    rec = {}
    for name, cc, hw in (("latent_cc4_hw4096", 4, 4096), ("pixel_cc3_hw262144", 3, 262144)):
        keys = torch.randn(len(IDX) * hw, 8, device="cuda").to(BF16)
        out = torch.empty(FRAMES * hw, 8, device="cuda", dtype=BF16)
        idx = torch.tensor(IDX, dtype=torch.int32, device="cuda")
        op = ops.ROWS_SPARSE_COND | (cc << ops.ROWS_SPARSE_CH_SHIFT)
        h, stream = vdiff._lib.lib(), torch.cuda.current_stream().cuda_stream

        def launch():  # the launch alone: the wrapper's index upload is host work of its own
            vdiff._lib.check(h.vd_rows_eltwise(op, keys.data_ptr(), 8, idx.data_ptr(), len(IDX), 1, hw, FRAMES,
                                               FRAMES * hw, 8, out.data_ptr(), 8, stream), "vd_rows_eltwise(sparse_cond)")

        timed(launch, 3)
        timed(lambda: ops.sparse_cond(keys, IDX, 1, FRAMES, hw, cc, out=out), 3)
        tl, tw = [], []
        for _ in range(rounds):
            tl.append(timed(launch, inner))
            tw.append(timed(lambda: ops.sparse_cond(keys, IDX, 1, FRAMES, hw, cc, out=out), inner))
        moved = 16 * (FRAMES + len(IDX)) * hw
        rec[name] = {"frames": FRAMES, "key_frames": len(IDX), "hw": hw, "cc": cc, "bytes": moved,
                     "launch": summary(tl), "wrapper": summary(tw)}
        rec[name]["launch"]["gb_per_s"] = round(moved / rec[name]["launch"]["median_us"] / 1e3, 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sparsectrl_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparsectrl_bench needs the GPU: nothing is measured without one")
    rec = {"metric": "SparseCtrl: added ms per step against the plain and the ControlNet pipeline; op 8 (us)",
           "config": "full, 16 frames, 64 x 64 latents, CFG; key frames at [0, 8, 15]", "weights": "random",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inner": args.inner}
    rec["op8"] = op8(args.rounds, args.inner)
    if not args.skip_step:
        unet = vdiff.weights.materialize_synthetic("full", device="cuda", seed=0).prepare()
        sparse = synthetic(vdiff.SparseControlNetModel, 1)
        cn = synthetic(vdiff.ControlNetModel, 1)
        rec["sparse_controlnet_parameters"] = sum(p.numel() for p in sparse.parameters())
        rec["step"] = whole_step(unet, sparse, cn, args.rounds, args.steps)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
