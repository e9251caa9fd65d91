"""CLIP text-encoder benchmark: AnimateDiffPipeline.encode_prompt at the SD-1.5 encoder shapes
(vdiff.CLIPTextModel("sd15"): 12 layers, 768 wide, 12 heads, 77 positions; random weights), for
one prompt pair (2 prompts: a video's positive + negative) and for the grid search's 78 x 2 = 156
prompts in one batched forward, bf16, 1x MI355X.

    python tools/clip_bench.py [--reps 10] [--out profiles/clip_bench.json]

No real vocabulary exists offline, so the tokenizer runs on a synthetic one (the byte alphabet,
its `</w>` forms and the two specials: every prompt becomes one id per byte, truncated at 77),
which exercises the same host code and gives full 77-token rows.  Reported per batch size:
milliseconds per encode_prompt (tokenizer included, and the tokenizer's share), the number of
library calls (vd_* entry points; a split-K GEMM or an unfused GEMM + LayerNorm is one call with
two launches) and the algorithmic GFLOP.  There is no speed bar: the encoder runs once per video
against about 2.4 s of denoising.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "video-diffusion-experiments_amd")]

import torch  # noqa: E402

from vdiff import AnimateDiffPipeline, CLIPTextModel, CLIPTokenizer, ops  # noqa: E402
from vdiff.tokenizer import BOS, EOS, EOW, bytes_to_unicode  # noqa: E402

PROMPT = "a photo of an astronaut riding a horse on the moon, highly detailed, cinematic lighting, 4k"


def byte_tokenizer():
    syms = list(bytes_to_unicode().values())
    vocab = {t: i for i, t in enumerate(syms + [s + EOW for s in syms] + [BOS, EOS])}
    return CLIPTokenizer(vocab, [])


def encoder_flop(cfg, rows, seq):
    H, I, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
    return L * (2.0 * rows * H * (4 * H + 2 * I) + 4.0 * rows * seq * H / 2)  # causal: half the scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clip_bench.json"))
    args = ap.parse_args()
    torch.manual_seed(0)
    enc = CLIPTextModel("sd15").to("cuda", torch.bfloat16).prepare()
    tok = byte_tokenizer()
    pipe = AnimateDiffPipeline.__new__(AnimateDiffPipeline)
    pipe.text_encoder, pipe.tokenizer = enc, tok
    results = []
    for n in (2, 156):
        prompts = [f"{PROMPT} {i}" for i in range(n)]
        out = pipe.encode_prompt(prompts, n)  # warm-up (kernel loads, allocator)
        torch.cuda.synchronize()
        assert out.shape == (n, 77, 768) and torch.isfinite(out.float()).all()
        calls = [0]
        real = ops.check

        def counting(rc, what="", _c=calls, _r=real):
            _c[0] += 1
            return _r(rc, what)
        ops.check = counting
        try:
            pipe.encode_prompt(prompts, n)
        finally:
            ops.check = real
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            tok(prompts)
        t_tok = (time.perf_counter() - t0) / args.reps
        t0 = time.perf_counter()
        for _ in range(args.reps):
            pipe.encode_prompt(prompts, n)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.reps
        flop = encoder_flop(enc.config, n * 77, 77)
        results.append({"prompts": n, "ms_per_encode_prompt": round(1e3 * dt, 3), "tokenizer_ms": round(1e3 * t_tok, 3),
                        "vd_calls": calls[0], "algorithmic_gflop": round(flop / 1e9, 2),
                        "tflops_end_to_end": round(flop / dt / 1e12, 2)})  # host tokenizing overlaps the device
    rec = {"metric": "CLIP text encoder: ms per encode_prompt (SD-1.5 shapes, 77 tokens, bf16)", "config": "sd15",
           "weights": "random", "reps": args.reps, "device": torch.cuda.get_device_name(0), "results": results}
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
