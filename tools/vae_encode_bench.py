"""VAE encode benchmark: AutoencoderKL.encode of one 16-frame 512x512 video (the first stage of
AnimateDiffVideoToVideoPipeline.prepare_latents) through the SD-1.5 encoder shapes (synthetic
N(0, 0.02^2) weights), bf16, 1x MI355X, with the decode of the same frames' latents
(tools/vae_bench.py's workload) beside it for scale.

    python tools/vae_encode_bench.py [--frames 16] [--runs 7] [--chunk 8] [--out profiles/vae_encode_bench.json]

Each run is one whole encode (or decode) ended by a device synchronise; the figure is the median
over --runs runs after one warm-up of the same shapes, with min and max beside it.  Prints one JSON
line and writes it to --out.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "video-diffusion-experiments_amd")]

import torch  # noqa: E402

from vdiff import AnimateDiffPipeline, AutoencoderKL, init_synthetic_  # noqa: E402
from vdiff.models.vae import VAE_FULL  # noqa: E402

PEAK = 2500.0


def encode_flop(cfg, frames, H, W):
    """2*M*N*K over every conv / linear / attention product of the encoder."""
    ch, lpb, lc = list(cfg["block_out_channels"]), cfg["layers_per_block"], cfg["latent_channels"]
    pix = H * W

    def conv(cin, cout, p, k=9):
        return 2.0 * frames * p * cout * cin * k

    def res(cin, cout, p):
        return conv(cin, cout, p) + conv(cout, cout, p) + (conv(cin, cout, p, 1) if cin != cout else 0)

    f, prev = conv(cfg["in_channels"], ch[0], pix), ch[0]
    for i, c in enumerate(ch):
        f += sum(res(prev if j == 0 else c, c, pix) for j in range(lpb))
        prev = c
        if i < len(ch) - 1:
            pix //= 4
            f += conv(c, c, pix)
    f += 2 * res(prev, prev, pix)
    f += frames * (2.0 * pix * prev * prev * 4 + 4.0 * pix * pix * prev)  # q,k,v,out + QK^T, PV
    return f + conv(prev, 2 * lc, pix) + conv(2 * lc, 2 * lc, pix, 1)


def timed(fn, runs):
    fn()  # warm-up: kernel loads, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return {"median": round(ms[len(ms) // 2], 2), "min": round(ms[0], 2), "max": round(ms[-1], 2), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vae_encode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vae_encode_bench needs the GPU: no timing is taken without one")
    vae = init_synthetic_(AutoencoderKL("full", encoder=True), seed=0).to("cuda", torch.bfloat16).prepare()
    vae.frames_per_chunk = args.chunk
    x = (torch.rand((args.frames, 3, args.size, args.size), generator=torch.Generator().manual_seed(42)) * 2 - 1).cuda()
    dist = vae.encode(x).latent_dist
    assert torch.isfinite(dist.parameters).all()
    pipe = AnimateDiffPipeline.__new__(AnimateDiffPipeline)
    pipe.vae = vae
    lat = (dist.mode() * VAE_FULL["scaling_factor"]).permute(1, 0, 2, 3)[None].contiguous()
    enc = timed(lambda: vae.encode(x), args.runs)
    dec = timed(lambda: pipe.decode_latents(lat), args.runs)
    flop = encode_flop(VAE_FULL, args.frames, args.size, args.size)
    dt = enc["median"] / 1e3
    line = {
        "metric": f"VAE encode frames/s ({args.frames}-frame {args.size}x{args.size} video, SD-1.5 AutoencoderKL encoder)",
        "value": round(args.frames / dt, 2), "unit": "frames/s", "ms_per_video": enc,
        "dtype": "bf16", "data": "synthetic (frames uniform seed 42, weights N(0,0.02^2))",
        "config": {"workload": f"encode ({args.frames}, 3, {args.size}, {args.size}) -> moments "
                               f"({args.frames}, 8, {args.size // 8}, {args.size // 8})", "frames_per_chunk": args.chunk},
        "algorithmic_tflop": round(flop / 1e12, 3),
        "mfma": {"achieved": round(flop / dt / 1e12, 1), "peak": PEAK, "unit": "TFLOP/s",
                 "frac": round(flop / dt / 1e12 / PEAK, 4)},
        "decode_same_frames_ms_per_video": dec,
        "encode_over_decode": round(enc["median"] / dec["median"], 3)}
    print(json.dumps(line))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
