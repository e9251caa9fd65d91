#!/usr/bin/env python3
"""bench.py — denoising steps/s of the AnimateDiff UNetMotionModel step on MI355X.

Metric (BASELINE.json): denoising steps/sec (whole node) at 16-frame 512x512
bf16.  One step = UNet forward on the CFG batch (B=2: uncond + cond) of a
16-frame 64x64-latent video + CFG combine + DDIM update, run as
one replay of the captured hipGraph.  Workload: BASELINE config 3 (SD-1.5 +
motion-adapter-v1-5-2 shapes, 1.31B params, synthetic N(0, 0.02^2) weights,
synthetic latents/text embeddings).  With N ranks the 16 frames are sharded
F/N per GPU (frame-parallel, all-to-all around each motion module): all ranks
together run ONE video's denoising, so value = steps/s of the node (strong
scaling).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    torchrun --nproc-per-node N bench.py --gpus N ...

A plain run does only what the headline needs: set up, W warm-up steps, the K timed steps, one
JSON line (`value`, `ms_per_step`, `step_mfma`, which is arithmetic on the step time).  Every
measurement that takes a run of its own is behind `--full`: the `roofline` timings, the
`cpu_baseline`, the `no_cfg` variant and (N > 1) the `replicas_control`; without `--full` those
keys are null.  `--dump-outputs DIR` writes what the timed loop returned after its last step
(DenoiseLoop.run's latents, float32) as DIR/latents.npy (DIR/latents_rank<r>.npy per rank when
N > 1: each rank's frame shard); inputs and weights are seeded, so two builds run with the same
arguments can be compared output for output.

`--gpus N > 1` without a torch.distributed environment (no WORLD_SIZE) starts the N ranks
itself — `python -m torch.distributed.run --nproc-per-node N` as a CHILD process, before this
process touches the GPU — forwards rank 0's JSON line and exits with the children's status.
Under a launcher, WORLD_SIZE must equal --gpus (else exit 2).  `--layout replicas` is the
SURVEY §8e upper-bound control: N independent 16-frame videos, one per GPU, no collective in
the step; value = all ranks' steps / the slowest rank's time, labelled, never the headline.
`--dry-run` goes through the same launch / rendezvous / max-over-ranks path on the CPU (gloo)
without a model, for the CPU tests of this contract.

With `--full`, also reported: `roofline` for the spatial self-attention kernel at level 1
(S=4096, d=40: the north-star kernel), timed with HIP events on its launch
stream; `step_mfma` = the whole step's algorithmic FLOPs / step time vs the
bf16 dense MFMA peak; `cpu_baseline` = the oracle (PyTorch-CPU fp32
restatement) on a bounded sample (rank 0, N=1 only).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
for p in (str(ROOT), str(ROOT / "video-diffusion-experiments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = "denoising steps/sec (whole node) at 16-frame 512×512 bf16; 1/2/4/8-GPU scaling"
PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0
STEP_TFLOP = {"full": 35.496, "tiny": 0.234}   # BASELINE.md §2 / SURVEY App. B, CFG batch, F=16 / F=4
# FLOPs of the CFG batch that the CFG dedup (DenoiseLoop.cfg_dedup, round 5) does not execute — the
# two guidance halves are the same latents and timestep until the first cross-attention, so these
# run on one half (per 16 frames, full model): conv_in 1.510 + down_blocks[0].resnets[0]'s two 3x3
# convs 241.592 + proj_in 13.422 + QKV 40.265 + the L1 self-attention 343.597 + to_out 13.422 +
# attn2.to_q 13.422 GFLOP (+ time_emb_proj 0.001) = 667.23 GFLOP.  step_mfma's `achieved` keeps the
# algorithmic CFG-batch count (the outputs are bit-identical to the undeduplicated step); the
# executed-FLOP rate is reported beside it.
CFG_DEDUP_TFLOP = {"full": 0.66723}
WARM_ATTN = 10                 # untimed launches before each roofline timing (tools/prof_summary.py skips them)


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print(*a, file=sys.stderr, flush=True)


def capture_l1_attention(unet, frames, ehs_dim):
    """The step's own level-1 self-attention operands: one eager UNet forward of the bench
    workload (both CFG halves of `frames` frames, t = 981) with an ops.ATTN_TAP that keeps the
    first d = 40, S = 4096 self-attention call's q | k | v (in the model's fused [rows][3C]
    layout, softmax scale folded into q by Attention.prepare)."""
    from vdiff import ops
    got = {}

    def tap(q, k, v, batch, heads, sq, skv, d, scale):
        if "qkv" not in got and d == 40 and sq == 4096 and skv == 4096:
            got["qkv"] = torch.cat([q, k, v], 1)
            got["scale"] = scale
    g = torch.Generator().manual_seed(42)
    x = torch.randn((1, 4, frames, 64, 64), generator=g).cuda()
    ehs = torch.randn((2, 77, ehs_dim), generator=torch.Generator().manual_seed(1)).cuda()
    ops.ATTN_TAP = tap
    try:
        with torch.no_grad():
            unet(torch.cat([x, x]), 981, encoder_hidden_states=ehs)
    finally:
        ops.ATTN_TAP = None
    torch.cuda.synchronize()
    return got["qkv"], got["scale"]


def time_attention(n_img, reps, stream, stress=False, model_qkv=None):
    """The L1 spatial self-attention kernel alone: 4*S^2*d*heads*n_img FLOPs per launch.

    model_qkv: the step's own q | k | v of that call (capture_l1_attention) — the roofline
    line.  Without it the synthetic inputs of rounds 1-3: q, k, v ~ N(0, 1.5^2) with the softmax
    scale d^-1/2 * log2(e) folded into q (exp2-argument std about 3.2 log2 units); stress=True
    drops the folded scale (std about 14: the deferred-max fast pass rescales often)."""
    from vdiff import ops
    S, heads, d = 4096, 8, 40
    C = heads * d
    if model_qkv is not None:
        qkv = model_qkv
        assert qkv.shape == (n_img * S, 3 * C)
    else:
        g = torch.Generator(device="cuda").manual_seed(7)
        qkv = torch.randn(n_img * S, 3 * C, device="cuda", generator=g) * 1.5
        if not stress:
            qkv[:, :C] *= d ** -0.5 * math.log2(math.e)
        qkv = qkv.to(torch.bfloat16)
    out = torch.empty(n_img * S, C, device="cuda", dtype=torch.bfloat16)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    scale = 1.0 / math.log2(math.e)   # the model's call: softmax scale folded into to_q (Attention.prepare)
    for _ in range(WARM_ATTN):  # ~10 ms of launches: the clock settles after the step loops
        ops.attention(q, k, v, n_img, heads, S, S, d, out=out, scale=scale)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        ops.attention(q, k, v, n_img, heads, S, S, d, out=out, scale=scale)
    e1.record(stream)
    e1.synchronize()
    ms = e0.elapsed_time(e1) / reps
    flop = 4.0 * S * S * d * heads * n_img
    byts = 4.0 * n_img * S * C * 2            # Q, K, V read once + O written once (bf16)
    tf = flop / (ms * 1e-3) / 1e12
    return {"kernel": "flash40_kernel<unit-c> + its flash32 exact fix-up launch (spatial self-attn, L1: "
                      f"S=4096, d=40, 8 heads, {n_img} images)",
            "bound": "mfma", "achieved": round(tf, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(tf / PEAK_BF16_TFLOPS, 4), "traffic": None,
            "avg_launch_ms": round(ms, 4), "algorithmic_flop_per_launch": flop,
            "algorithmic_bytes_per_launch": byts}


ROOF_SOURCES = ("video-diffusion-experiments_amd/csrc/attention.hip", "video-diffusion-experiments_amd/csrc/common.h")


def roof_src_hash() -> str:
    """sha256[:16] of the roofline kernel's sources: the PMC summaries under profiles/ record the
    hash of the tree they were measured on, and bench.py uses only a summary whose hash equals
    the current tree's (tools/roofline_prof.sh writes them)."""
    import hashlib
    h = hashlib.sha256()
    for f in ROOF_SOURCES:
        h.update(f.encode() + b"\0" + (ROOT / f).read_bytes() + b"\0")
    return h.hexdigest()[:16]


def _pmc_file(pattern):
    """The committed PMC summary (profiles/<pattern>) measured on THIS tree's roofline kernel
    sources (its kernel_src_hash), newest round first; (None, None) when there is none."""
    want = roof_src_hash()
    for f in sorted((ROOT / "profiles").glob(pattern), reverse=True):
        try:
            t = json.loads(f.read_text())
        except (OSError, ValueError):
            continue
        if t.get("kernel_src_hash") == want:
            return t, f.name
    return None, None


def pmc_traffic(n_img):
    """HBM bytes per launch of the roofline kernel from the committed PMC summary measured on
    this tree (profiles/rNN_traffic.json: separate FETCH_SIZE / WRITE_SIZE rocprofv3 passes over
    `bench.py --roofline-only` at 32 images, corrected as MI355X_MICROARCH.md §HBM prescribes;
    scaled linearly to this rank's image count).  None when no summary matches the sources."""
    t, name = _pmc_file("r*_traffic.json")
    if t is None or "flash40_kernel" not in (t.get("kernel") or ""):
        return None, None
    return t["traffic_bytes_per_launch"] * n_img / 32.0, name


def pmc_mfma_busy():
    """MFMA-busy share of the roofline kernel (SQ_VALU_MFMA_BUSY_CYCLES over 1024 SIMDs x
    GRBM_GUI_ACTIVE/8) from the committed profiles/rNN_mfma_busy.json measured on this tree.
    Counts padded MFMA work, unlike `frac`."""
    t, name = _pmc_file("r*_mfma_busy.json")
    return (t.get("mfma_busy_frac"), name) if t else (None, None)


def cpu_baseline(unet_gpu, cfg_name, frames_sample, frames_full):
    """Oracle (oracle/unet_ref.py, fp32 PyTorch-CPU) on `frames_sample` frames of the
    same CFG-batch step; scaled to steps/s of the full `frames_full`-frame video."""
    from oracle import ddim_ref, unet_ref
    from vdiff.config import get_config
    cfg = get_config(cfg_name)
    sd = {k: v.detach().float().cpu() for k, v in unet_gpu.state_dict().items()}
    g = torch.Generator().manual_seed(42)
    lat = torch.randn((1, 4, frames_sample, 64, 64), generator=g)
    ehs = torch.randn((2, 77, cfg["cross_attention_dim"]), generator=torch.Generator().manual_seed(1))
    acp = ddim_ref.alphas_cumprod()
    times = []
    with torch.no_grad():
        for _ in range(4):  # 1 warm-up + 3 timed
            t0 = time.perf_counter()
            eps = unet_ref.unet_forward(sd, cfg, torch.cat([lat, lat]), 981, ehs)
            ddim_ref.ddim_step(ddim_ref.cfg_combine(eps, 7.5), 981, lat, 50, acp)
            times.append(time.perf_counter() - t0)
    t = sorted(times[1:])[1]
    return {"value": round(1.0 / (t * frames_full / frames_sample), 5), "unit": "denoising steps/s",
            "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"1 CFG step (UNet fwd B=2 + CFG + DDIM) of the {cfg_name} model on {frames_sample} "
                      f"of {frames_full} frames, fp32, 1 warm-up then median of 3 = {t:.2f} s, scaled "
                      f"x{frames_full // frames_sample} to the full video (every op but the motion "
                      f"attention core, 0.1 % of the FLOPs, is linear in frames; BASELINE.md §3)"}


def dump_outputs(dirname, lat, world, rank):
    """The latents the timed loop returned after its last step, as float32 .npy: latents.npy on
    one GPU, latents_rank<r>.npy (this rank's frame shard) on several.  1 MiB for the full
    workload's [1, 4, 16, 64, 64], far below the 64 MB a dump may take."""
    import numpy as np
    d = Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    arr = lat.detach().float().cpu().numpy()
    assert arr.nbytes <= 64 << 20, f"output dump of {arr.nbytes} bytes"
    np.save(d / ("latents.npy" if world == 1 else f"latents_rank{rank}.npy"), arr)


def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def visible_gpus():
    """GPUs this process could use, counted WITHOUT touching the HIP runtime (the launcher parent
    must not initialise it: torch.cuda.device_count() falls back to hipGetDeviceCount when amdsmi
    is absent — ADVICE r05): the *_VISIBLE_DEVICES lists if set, else the KFD topology nodes with
    SIMDs.  None when neither is readable (the ranks then find out themselves)."""
    counts = []
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v:  # an empty list is left to the ranks (its meaning differs between runtimes)
            counts.append(len([t for t in v.split(",") if t.strip()]))
    if counts:
        return min(counts)
    nodes = Path("/sys/class/kfd/kfd/topology/nodes")
    try:
        n = 0
        for props in nodes.glob("*/properties"):
            for line in props.read_text().splitlines():
                if line.startswith("simd_count") and int(line.split()[1]) > 0:
                    n += 1
        return n or None
    except (OSError, ValueError):
        return None


def launch_ranks(n: int, argv) -> int:
    """Start n ranks of this script under torch.distributed.run as a child process (never an
    exec: nothing here has touched the GPU, and the children initialise it themselves);
    their stdout is this process's, so rank 0's JSON line comes through unchanged."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", str(Path(__file__).resolve())] + list(argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.setdefault("OMP_NUM_THREADS", "4")
    log(f"[bench] --gpus {n}: launching {n} ranks: {' '.join(cmd[1:])}")
    return subprocess.run(cmd, env=env).returncode


def check_world(args):
    """The rank environment against --gpus: (world, rank, local_rank) or SystemExit."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" in os.environ and world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a "
              f"{world}-rank run as {args.gpus} GPUs", file=sys.stderr)
        raise SystemExit(2)
    return world, int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))


def dry_run(args, world, rank):
    """The multi-rank contract without a GPU or a model: gloo rendezvous, the timed region's
    barriers, max-over-ranks, one JSON line from rank 0 (tests/test_bench_launch.py)."""
    if world > 1:
        dist.init_process_group("gloo")
    t0 = time.perf_counter()
    if world > 1:
        dist.barrier()
    el = torch.tensor([time.perf_counter() - t0 + 1e-6 * (rank + 1)], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        ranks = [None] * world
        dist.all_gather_object(ranks, {"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "0"))})
    else:
        ranks = [{"rank": 0, "local_rank": 0}]
    if rank == 0:
        print(json.dumps({"metric": METRIC, "value": None, "unit": "denoising steps/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "dry_run": True,
                          "layout": args.layout, "max_elapsed_s": el.item(), "ranks": ranks}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="full", choices=["full", "tiny"])
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beside the headline: roofline kernel timings, CPU oracle "
                         "baseline, the no-CFG variant, the replicas control (N>1); each has its own --no-* switch")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the latents the timed loop returned to DIR/latents.npy "
                         "(float32; DIR/latents_rank<r>.npy per rank when N>1)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=2)
    ap.add_argument("--attn-reps", type=int, default=20)
    ap.add_argument("--no-nocfg", action="store_true", help="skip the B=1 (no-CFG) variant")
    ap.add_argument("--roofline-only", action="store_true",
                    help="only the roofline kernel's timing (the same time_attention call as the bench line; "
                         "tools/roofline_prof.sh runs its PMC passes over this)")
    ap.add_argument("--overlap", type=int, default=1,
                    help="N>1: chunk each motion module's all-to-alls over positions and overlap them with "
                         "the transformer block on a second stream (vdiff.dist.FrameShard overlap_chunks)")
    ap.add_argument("--window", default="a2a", choices=["a2a", "kv-gather"],
                    help="N>1: motion-module temporal window — all-to-all re-shard (default) or the north "
                         "star's K/V all-gather over the frame shards (vdiff.dist.FrameShard window)")
    ap.add_argument("--layout", default="auto", choices=["auto", "frame", "cfg-frame", "replicas"],
                    help="N>1 placement (vdiff.dist.layout): auto = cfg-frame at 2 GPUs, frame otherwise; "
                         "replicas = one independent video per GPU (SURVEY §8e upper-bound control, weak scaling)")
    ap.add_argument("--no-replicas", action="store_true",
                    help="N>1: skip the replicas control measured after the sharded run")
    ap.add_argument("--dry-run", action="store_true",
                    help="CPU only: the launch / rendezvous / max-over-ranks path with gloo and no model")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        n_vis = None if args.dry_run else visible_gpus()
        if n_vis is not None and n_vis < args.gpus:
            print(f"bench.py: --gpus {args.gpus} but {n_vis} GPUs visible", file=sys.stderr)
            raise SystemExit(2)
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    world, rank, local = check_world(args)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dry_run:
        dry_run(args, world, rank)
        return
    torch.cuda.set_device(local)
    if args.roofline_only:
        from vdiff.weights import materialize_synthetic
        frames = args.frames or 16
        unet = materialize_synthetic(args.config, device="cuda", seed=0)
        unet.prepare()
        mqkv, _ = capture_l1_attention(unet, frames, unet.config["cross_attention_dim"])
        del unet
        roof = time_attention(2 * frames, args.attn_reps, torch.cuda.current_stream(), model_qkv=mqkv)
        roof["kernel_src_hash"] = roof_src_hash()
        print(json.dumps({"roofline": roof}), flush=True)
        return
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))

    import vdiff
    from vdiff import DDIMScheduler, DenoiseLoop
    from vdiff.weights import materialize_synthetic

    cfg_name = args.config
    frames = args.frames or (16 if cfg_name == "full" else 4)
    replicas = args.layout == "replicas"
    t0 = time.time()
    from vdiff.dist import NodeLayout
    # replicas: every rank is a whole single-GPU job on its own video (no shard, no collective)
    lay = NodeLayout("frame" if replicas else args.layout, frames, cfg=True, world=1 if replicas else world,
                     rank=0 if replicas else rank, overlap_chunks=args.overlap, window=args.window)
    unet = materialize_synthetic(cfg_name, device="cuda", seed=0)
    unet.dist = lay.frame_shard
    unet.prepare()
    log(f"[bench] model ready in {time.time() - t0:.1f}s; world={world} layout="
        f"{'replicas x%d' % world if replicas else lay.describe()}")
    cfg = unet.config
    fl = lay.frames_local
    g = torch.Generator().manual_seed(42)
    lat_all = torch.randn((1, 4, frames, 64, 64), generator=g)
    ehs = torch.randn((2, 77, cfg["cross_attention_dim"]), generator=torch.Generator().manual_seed(1))
    sched = DDIMScheduler.from_config(DDIMScheduler().config, beta_schedule="linear", steps_offset=1,
                                      clip_sample=False)
    sched.set_timesteps(50)
    total = args.warmup + args.steps
    ts = sched.timesteps.repeat((total + 49) // 50)[:max(total, 50)]

    def timed(lay_, ehs_, guidance, cfg_shard=None):
        """W untimed + K timed replays of a captured loop on this layout; the timed region is
        bracketed by barrier + synchronize on both sides; returns (max-over-ranks seconds, loop,
        what the last timed step returned)."""
        lp = DenoiseLoop(unet, sched, lat_all[:, :, lay_.frame_slice()].cuda(), ehs_.cuda(), guidance,
                         timesteps=ts, use_graph=not args.no_graph, cfg_shard=cfg_shard)
        lp.prime()
        lp.run(args.warmup)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t_start = time.perf_counter()
        out = lp.run(args.steps)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        el = time.perf_counter() - t_start
        if world > 1:
            tt = torch.tensor([el], device="cuda", dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el = tt.item()
        assert torch.isfinite(lp.lat).all(), "non-finite latents"
        return el, lp, out

    elapsed, loop, out = timed(lay, ehs, 7.5, lay.cfg_shard)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out, world, rank)
    del out
    log(f"[bench] graph={'yes' if loop.graph is not None else 'no'} {loop.graph_error or ''}")
    videos = world if replicas else 1           # independent videos the node denoised per step
    sps = videos * args.steps / elapsed
    graph_ok = loop.graph is not None
    cfg_dedup = bool(getattr(loop, "cfg_dedup", False))  # the loop's CFG dedup (step_mfma labels it)
    ms = 1e3 * elapsed / args.steps
    del loop

    # the B=1 (no-CFG, guidance 1) variant, labelled — same graph-captured
    # loop on the conditional half only
    nocfg = None
    if args.full and not args.no_nocfg:
        # no CFG pair to split: frame-shard over all ranks
        lay1 = lay if lay.layout == "frame" else NodeLayout("frame", frames, cfg=False, world=world, rank=rank,
                                                             overlap_chunks=args.overlap, window=args.window)
        unet.dist = lay1.frame_shard
        e1, lp1, _ = timed(lay1, ehs[1:], 1.0)
        del lp1
        nocfg = {"value": round(videos * args.steps / e1, 4), "unit": "denoising steps/s",
                 "ms_per_step": round(1e3 * e1 / args.steps, 3),
                 "config": "guidance_scale 1 (no CFG): UNet batch 1 per step, same frames/latents"}

    # the "replicas only" upper-bound control beside a sharded run — every rank
    # denoises its own whole 16-frame video, no collective; labelled, never the headline
    rep = None
    if args.full and world > 1 and not replicas and not args.no_replicas:
        lay_r = NodeLayout("frame", frames, cfg=True, world=1, rank=0)
        unet.dist = None
        er, lpr, _ = timed(lay_r, ehs, 7.5)
        del lpr
        rep = {"value": round(world * args.steps / er, 4), "unit": "denoising steps/s (node, N videos)",
               "ms_per_step": round(1e3 * er / args.steps, 3), "scaling": "weak",
               "config": f"replicas x{world}: one independent {frames}-frame CFG video per GPU, no collective "
                         "(SURVEY §8e upper-bound control, not the headline)"}
    unet.dist = lay.frame_shard

    roof = None
    if args.full:
        imgs = (2 // lay.cfg_ranks) * fl  # images per rank in the CFG run
        mqkv = None
        if lay.frame_shard is None and lay.cfg_shard is None:  # one GPU: the step's own operands
            mqkv, _ = capture_l1_attention(unet, fl, cfg["cross_attention_dim"])
        roof = time_attention(imgs, args.attn_reps, torch.cuda.current_stream(), model_qkv=mqkv)
        syn = time_attention(imgs, args.attn_reps, torch.cuda.current_stream())
        st = time_attention(imgs, args.attn_reps, torch.cuda.current_stream(), stress=True)
        roof["synthetic"] = {k: syn[k] for k in ("achieved", "frac", "avg_launch_ms")}
        roof["stress"] = {k: st[k] for k in ("achieved", "frac", "avg_launch_ms")}
        roof["inputs"] = (("q | k | v of the step's level-1 self-attention in the synthetic-weight model (one eager "
                           "forward of the workload with its N(0, 0.02^2) random-init weights, t = 981; softmax scale "
                           "folded into q by to_q) -- not a trained network's logit statistics") if mqkv is not None else
                          "synthetic (multi-rank run)") + (
                          "; `synthetic`: q, k, v ~ N(0, 1.5^2) with the scale folded (exp2 argument std ~3.2), "
                          "rounds 1-3's roofline input; `stress`: the scale not folded (std ~14)")
        roof["traffic"], roof["traffic_source"] = pmc_traffic(imgs)
        roof["mfma_busy"], roof["mfma_busy_source"] = pmc_mfma_busy()
        roof["kernel_src_hash"] = roof_src_hash()
    gpu_tflop = STEP_TFLOP[cfg_name] * frames / (16 if cfg_name == "full" else 4) / (1 if replicas else world)
    step_tf = gpu_tflop / (ms * 1e-3)
    step_mfma = {"algorithmic_tflop_per_step_per_gpu": round(gpu_tflop, 3),
                 "achieved": round(step_tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                 "frac": round(step_tf / PEAK_BF16_TFLOPS, 4)}
    dedup = cfg_dedup and lay.cfg_shard is None and cfg_name in CFG_DEDUP_TFLOP
    if dedup:  # the duplicated CFG-half work the step skips (bit-identical outputs): labelled, not hidden
        saved = CFG_DEDUP_TFLOP[cfg_name] * frames / 16 / (1 if replicas else world)
        step_mfma["cfg_dedup_tflop_saved"] = round(saved, 3)
        step_mfma["executed_tflop_per_step_per_gpu"] = round(gpu_tflop - saved, 3)
        step_mfma["executed_achieved"] = round((gpu_tflop - saved) / (ms * 1e-3), 1)
        step_mfma["executed_frac"] = round((gpu_tflop - saved) / (ms * 1e-3) / PEAK_BF16_TFLOPS, 4)
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        log("[bench] timing the CPU oracle baseline ...")
        cpu = cpu_baseline(unet, cfg_name, min(args.cpu_frames, frames), frames)

    if rank == 0:
        line = {
            "metric": METRIC,
            "value": round(sps, 4),
            "unit": "denoising steps/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms, 3),
            "higher_is_better": True,
            "scaling": "weak" if replicas else "strong",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic (latents randn seed 42, text embeddings randn seed 1, weights N(0,0.02^2))",
            "config": {
                "workload": ("BASELINE config 3: AnimateDiff UNetMotionModel (SD-1.5 + motion-adapter-"
                             "v1-5-2 shapes, 1.31B params), 16 frames x 64x64 latents (512x512), CFG "
                             "batch 2, guidance 7.5, DDIM 50-step schedule, one hipGraph replay per step")
                if cfg_name == "full" else "BASELINE config 2: tiny UNetMotionModel, 4 frames x 64x64",
                "model": f"UNetMotionModel[{cfg_name}]",
                "frames": frames, "latent_hw": 64, "global_batch": 2, "seq_len": 4096,
                "parallelism": (f"replicas x{world} (one independent video per GPU: SURVEY §8e upper-bound "
                                "control, not the headline)") if replicas else lay.describe(),
                "hipgraph": graph_ok,
            },
            "roofline": roof,
            "step_mfma": step_mfma,
            "cpu_baseline": cpu,
            "no_cfg": nocfg,
            "replicas_control": rep,
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
