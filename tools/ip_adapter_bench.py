"""IP-Adapter benchmark: what the image prompt adds to a denoising step, bf16, 1x MI355X.

    python tools/ip_adapter_bench.py [--rounds 7] [--steps 3] [--skip-step] [--out profiles/ip_adapter_bench.json]

1. Per cross-attention shape of the full config at 16 frames with CFG (32 images, 77 text
   tokens, 4 image tokens; hw 4096 / d 40, hw 1024 / d 80, hw 256 / d 160, hw 64 / d 160), three
   forms of the spatial cross-attention:
     (a) text only, the product kernel choice                      — the baseline
     (b) VD_ATTN_TAIL(4): one launch, two softmax segments          — what the model runs
     (c) the composition: (a), a second call on the 4 image keys, and a row add
   The forms are interleaved round by round (a, b, c, a, b, c, ...), each timed with device events
   over `inner` back-to-back launches; reported: the median over rounds and the spread
   (max - min) / median of each form.
2. The whole step: DenoiseLoop (graph replay) at the full config with and without the adapter, in
   one session, interleaved; the added ms per step.
3. The once-per-video cost: the ViT-H/14 forward, the image projection and the 16 K/V GEMM pairs.
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
IMAGES, FRAMES, L, N_IP = 32, 16, 77, 4
SHAPES = [(4096, 8, 40), (1024, 8, 80), (256, 8, 160), (64, 8, 160)]  # (hw, heads, d)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us


def summary(xs):
    med = statistics.median(xs)
    return {"median_us": round(med, 2), "spread": round((max(xs) - min(xs)) / med, 4)}


def attention_forms(hw, heads, d, rounds, inner):
    C = heads * d
    bkv = IMAGES // FRAMES
    g = torch.Generator(device="cuda").manual_seed(hw + d)
    q = torch.randn(IMAGES * hw, C, device="cuda", generator=g).to(BF16)
    kv_text = torch.randn(bkv * L, 2 * C, device="cuda", generator=g).to(BF16)
    kv_ip = torch.randn(bkv * N_IP, 2 * C, device="cuda", generator=g).to(BF16)
    kv_both = torch.cat([torch.cat([kv_text[b * L:(b + 1) * L], kv_ip[b * N_IP:(b + 1) * N_IP]]) for b in range(bkv)])
    out, out2 = torch.empty(IMAGES * hw, C, device="cuda", dtype=BF16), torch.empty(IMAGES * hw, C, device="cuda", dtype=BF16)
    scale = 1.0 / 1.4426950408889634  # the model path: c == 1 (the scale is folded into to_q)
    kw = dict(kv_div=FRAMES, scale=scale)

    def form_a():
        ops.attention(q, kv_text[:, :C], kv_text[:, C:], IMAGES, heads, hw, L, d, out=out, **kw)

    def form_b():
        ops.attention(q, kv_both[:, :C], kv_both[:, C:], IMAGES, heads, hw, L + N_IP, d, out=out, tail=N_IP, **kw)

    def form_c():
        ops.attention(q, kv_text[:, :C], kv_text[:, C:], IMAGES, heads, hw, L, d, out=out, **kw)
        ops.attention(q, kv_ip[:, :C], kv_ip[:, C:], IMAGES, heads, hw, N_IP, d, out=out2, **kw)
        ops.rows_add(out, out2, out=out)

    forms = {"a_text_only": form_a, "b_tail": form_b, "c_composition": form_c}
    for f in forms.values():  # warm-up
        timed(f, 3)
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, f in forms.items():
            t[k].append(timed(f, inner))
    rec = {"hw": hw, "heads": heads, "d": d, **{k: summary(v) for k, v in t.items()}}
    noise = max(rec[k]["spread"] for k in forms) * rec["b_tail"]["median_us"]
    rec["added_us_b_minus_a"] = round(rec["b_tail"]["median_us"] - rec["a_text_only"]["median_us"], 2)
    rec["c_beats_b_beyond_spread"] = bool(rec["b_tail"]["median_us"] - rec["c_composition"]["median_us"] > noise)
    rec["product_uses"] = "c_composition" if rec["c_beats_b_beyond_spread"] else "b_tail"
    return rec


def synthetic_adapter(unet, clip_dim, n=N_IP):
    g = torch.Generator().manual_seed(0)
    cross = unet.config["cross_attention_dim"]
    sd = {"image_proj.proj.weight": torch.randn(n * cross, clip_dim, generator=g) * clip_dim ** -0.5,
          "image_proj.proj.bias": torch.zeros(n * cross), "image_proj.norm.weight": torch.ones(cross),
          "image_proj.norm.bias": torch.zeros(cross)}
    for i, a in enumerate(unet.spatial_cross_attentions()):
        for kv in "kv":
            sd[f"ip_adapter.{2 * i + 1}.to_{kv}_ip.weight"] = torch.randn(a.heads * a.dim_head, cross, generator=g) * cross ** -0.5
    return sd


def whole_step(rounds, steps):
    pipe = vdiff.AnimateDiffPipeline.from_config("full", device="cuda", vae=None)
    unet = pipe.unet
    s = unet.config["sample_size"]
    lat = torch.randn(1, unet.config["in_channels"], FRAMES, s, s)
    ehs = torch.randn(2, L, unet.config["cross_attention_dim"])
    pipe.scheduler.set_timesteps(50)
    plain = vdiff.DenoiseLoop(unet, pipe.scheduler, lat, ehs, 7.5).prime()
    enc = vdiff.CLIPVisionModelWithProjection("vit_h14").to("cuda", BF16).prepare()
    pipe.load_ip_adapter(synthetic_adapter(unet, enc.config["projection_dim"]))
    px = torch.randn(1, 3, 224, 224, device="cuda")

    def once(fn, reps=5):
        fn()
        return round(statistics.median(timed(fn, 1) for _ in range(reps)) / 1e3, 3)  # ms

    e = enc(px).image_embeds
    both = torch.cat([torch.zeros_like(e), e])
    ip = pipe.image_projection(both)
    ehs_rows = ehs.to("cuda", BF16).reshape(2 * L, -1)
    ip_rows = ip.reshape(2 * N_IP, -1)
    attns = unet.spatial_cross_attentions()
    per_video = {"vit_h14_forward_ms": once(lambda: enc(px)), "image_projection_ms": once(lambda: pipe.image_projection(both)),
                 "kv_gemms_16_attentions_ms": once(lambda: [a.project_kv(ehs_rows, ip_rows, 2) for a in attns]),
                 "kv_gemms_text_only_ms": once(lambda: [a.project_kv(ehs_rows) for a in attns])}
    adapted = vdiff.DenoiseLoop(unet, pipe.scheduler, lat, ehs, 7.5, ip_embeds=ip).prime()
    loops = {"without_adapter": plain, "with_adapter": adapted}
    t = {k: [] for k in loops}
    for k, lp in loops.items():
        lp.run(2)
    for _ in range(rounds):
        for k, lp in loops.items():
            lp.reset(lat.to("cuda", torch.float32))
            t[k].append(timed(lambda lp=lp: lp.run(1), steps) / 1e3)  # ms per step
    rec = {k: {"median_ms": round(statistics.median(v), 3), "spread": round((max(v) - min(v)) / statistics.median(v), 4)}
           for k, v in t.items()}
    rec["added_ms_per_step"] = round(rec["with_adapter"]["median_ms"] - rec["without_adapter"]["median_ms"], 3)
    rec["graph"] = [lp.graph is not None for lp in loops.values()]
    return rec, per_video


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ip_adapter_bench.json"))
    args = ap.parse_args()
    rec = {"metric": "IP-Adapter: cross-attention forms (us per launch set) and added ms per step",
           "config": "full, 16 frames, CFG (32 images), 77 text + 4 image tokens", "weights": "random",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "inner": args.inner,
           "attention": [attention_forms(hw, h, d, args.rounds, args.inner) for hw, h, d in SHAPES]}
    if not args.skip_step:
        rec["step"], rec["once_per_video"] = whole_step(args.rounds, args.steps)
    print(json.dumps(rec))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
