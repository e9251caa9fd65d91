"""Temporal-consistency metrics of generated videos on the GPU.

Mirrors the reference's measurement (experiments/06_measure_grid_search.py): frames are
read like its load_frames (:97-113: sorted frame_*.png, PIL RGB), and per video the
consecutive-pair MSE / PSNR (:209-218), their mean / population std, and the flicker
index (:221-235) are reported under the reference's JSON keys.  The pixel work — every
byte of every frame, for a whole batch of videos — is one pass of the HIP kernel
vd_frame_metrics (exact integer sums); the host only forms the scalars.  The optical-flow
fields (06:163-199 Farneback flow magnitude, :259-284 warp error) come from the HIP
Farneback pipeline vd_farneback_flow + vd_flow_warp_stats over every pair of the batch.
LPIPS (06:122-154, lpips.LPIPS(net='alex', version='0.1')) is the class LPIPS below: AlexNet's
five ReLU taps in exact fp32 on the f32-input MFMA (vd_lpips_pairs), features once per frame.
Its weights are not part of this repository: LPIPS.from_files takes the torchvision AlexNet
checkpoint (alexnet-owt-*.pth) and the lpips package's weights/v0.1/alex.pth, or one saved
lpips.LPIPS.state_dict(), from local files; LPIPS.synthetic gives seeded weights for tests.
measure_videos(x, lpips=LPIPS...) then fills mean_lpips / std_lpips / the per-pair lpips and
temporal_consistency_score; with lpips=None those fields stay None.  Parity with the LPIPS
values in the reference's records is not pinned: no AlexNet weights exist offline, and the
reference ran cuDNN with TF32 allowed, so its records are themselves good to about 1e-3.
"""
from __future__ import annotations

from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import check, lib


def load_frames(frame_dir) -> np.ndarray:
    """[F, H, W, 3] uint8 — experiments/06:97-113 without its /255."""
    from PIL import Image
    d = Path(frame_dir)
    files = sorted(d.glob("*.png")) or sorted(d.glob("*.jpg"))
    if not files:
        raise ValueError(f"No frames found in {d}")
    return np.stack([np.array(Image.open(f).convert("RGB")) for f in files])


def frame_sums(videos_u8: torch.Tensor):
    """uint8 [V, F, H, W, 3] on the GPU -> (sse [V, F-1], sad [V, F-2]) int64 on the GPU."""
    if not videos_u8.is_cuda or videos_u8.dtype != torch.uint8:
        raise ValueError("frame_sums takes a uint8 CUDA tensor (no CPU fallback)")
    x = videos_u8.contiguous()
    V, Fr = x.shape[:2]
    nb = x[0, 0].numel()
    sse = torch.empty(V, Fr - 1, device=x.device, dtype=torch.int64)
    sad = torch.empty(V, max(Fr - 2, 0), device=x.device, dtype=torch.int64)
    stream = torch.cuda.current_stream().cuda_stream
    check(lib().vd_frame_metrics(x.data_ptr(), V, Fr, nb, sse.data_ptr(), sad.data_ptr() if Fr > 2 else None,
                                 stream), "vd_frame_metrics")
    return sse, sad


# OpticalFlowEstimator.compute_flow's cv2 arguments (06:176-186)
FARNEBACK = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2)


def _u8_videos(videos_u8: torch.Tensor) -> torch.Tensor:
    if not videos_u8.is_cuda or videos_u8.dtype != torch.uint8 or videos_u8.dim() != 5 or videos_u8.shape[-1] != 3:
        raise ValueError("takes a uint8 CUDA tensor [videos, frames, H, W, 3] (no CPU fallback)")
    return videos_u8.contiguous()


def farneback_flow(videos_u8: torch.Tensor, **params) -> torch.Tensor:
    """uint8 [V, F, H, W, 3] on the GPU -> flow fp32 [V, F-1, H, W, 2]: cv2.calcOpticalFlowFarneback
    of every consecutive grey pair (06:163-188), parameters as 06 passes them unless overridden."""
    x = _u8_videos(videos_u8)
    V, Fr, H, W = x.shape[:4]
    p = {**FARNEBACK, **params}
    ws_bytes = lib().vd_farneback_workspace(V, Fr, H, W)
    if ws_bytes < 0:
        raise ValueError(f"bad video shape {tuple(x.shape)}")
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    flow = torch.empty(V, Fr - 1, H, W, 2, device=x.device, dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    check(lib().vd_farneback_flow(x.data_ptr(), V, Fr, H, W, p["pyr_scale"], p["levels"], p["winsize"],
                                  p["iterations"], p["poly_n"], p["poly_sigma"], flow.data_ptr(), ws.data_ptr(),
                                  ws_bytes, stream), "vd_farneback_flow")
    return flow


def flow_sums(videos_u8: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """-> fp64 [V, F-1, 3] = {sum |flow|, sum |flow|^2, sum (warp_frame(f, flow) - f')^2}."""
    x = _u8_videos(videos_u8)
    V, Fr, H, W = x.shape[:4]
    if tuple(flow.shape) != (V, Fr - 1, H, W, 2) or flow.dtype != torch.float32 or not flow.is_cuda:
        raise ValueError("flow must be fp32 CUDA [V, F-1, H, W, 2]")
    flow = flow.contiguous()
    ws_bytes = lib().vd_flow_warp_workspace(V, Fr)
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8)
    stats = torch.empty(V, Fr - 1, 3, device=x.device, dtype=torch.float64)
    stream = torch.cuda.current_stream().cuda_stream
    check(lib().vd_flow_warp_stats(x.data_ptr(), flow.data_ptr(), V, Fr, H, W, stats.data_ptr(), ws.data_ptr(),
                                   ws_bytes, stream), "vd_flow_warp_stats")
    return stats


def flow_fields(stats, hw: int) -> dict:
    """One video's [F-1, 3] flow sums -> the per-pair and aggregate flow / warp fields of the
    reference's record (06:190-199 magnitude mean / population std, :336-338, :379-383)."""
    mag_mean = [s[0] / hw for s in stats]
    mag_std = [float(np.sqrt(max(s[1] / hw - (s[0] / hw) ** 2, 0.0))) for s in stats]
    warp = [s[2] / (3 * hw) for s in stats]
    return {"mean_flow_magnitude": float(np.mean(mag_mean)), "flow_magnitude_variance": float(np.var(mag_mean)),
            "mean_warp_error": float(np.mean(warp)), "warp_error_variance": float(np.var(warp)),
            "pairs": [{"flow_magnitude_mean": m, "flow_magnitude_std": sd, "warp_error": w}
                      for m, sd, w in zip(mag_mean, mag_std, warp)]}


def _psnr(mse: float) -> float:
    return 100.0 if mse < 1e-10 else float(10 * np.log10(1.0 / mse))


def video_metrics(sse, sad, n_values: int, lpips: Optional[Sequence[float]] = None) -> dict:
    """One video's record, keys as the reference's <experiment>_metrics.json."""
    mse = [float(s) / (255.0 ** 2 * n_values) for s in sse]
    psnr = [_psnr(m) for m in mse]
    rec = {
        "num_frames": len(mse) + 1,
        "mean_mse": float(np.mean(mse)), "std_mse": float(np.std(mse)),
        "mean_psnr": float(np.mean(psnr)),
        "mean_lpips": float(np.mean(lpips)) if lpips is not None else None,
        "std_lpips": float(np.std(lpips)) if lpips is not None else None,
        "mean_flow_magnitude": None, "flow_magnitude_variance": None,
        "mean_warp_error": None, "warp_error_variance": None,
        "temporal_consistency_score": None,
        "flicker_index": float(np.mean([float(s) / (255.0 * n_values) for s in sad])) if len(sad) else 0.0,
        "frame_metrics": [{"frame_idx": i, "mse": m, "psnr": p,
                           "lpips": float(lpips[i]) if lpips is not None else None}
                          for i, (m, p) in enumerate(zip(mse, psnr))],
    }
    if lpips is not None:  # experiments/06:238-256
        rec["temporal_consistency_score"] = (float(np.var(mse)) * 1000 + float(np.mean(mse)) * 100
                                             + float(np.mean(lpips)) * 50 + float(np.var(lpips)) * 500)
    return rec


FLOW_WORKSPACE_CAP = 2 << 30   # bytes of Farneback workspace per group of videos
LPIPS_WORKSPACE_CAP = 2 << 30  # bytes of AlexNet features per group of videos (~15.5 MB per 512x512 frame)

# AlexNet `features` as lpips slices it: (index in torchvision's Sequential, lpips slice, Cin, Cout, k)
LPIPS_CONVS = ((0, 1, 3, 64, 11), (3, 2, 64, 192, 5), (6, 3, 192, 384, 3), (8, 4, 384, 256, 3), (10, 5, 256, 256, 3))
LPIPS_SHIFT = (-.030, -.088, -.188)  # lpips ScalingLayer
LPIPS_SCALE = (.458, .448, .450)


def lpips_param_offsets() -> dict:
    """Float offsets of the vd_lpips_pairs parameter blob (include/vdiff.h): conv weights 1..5
    (OHWI), conv biases 1..5, lin vectors 1..5, shift, scale; "size" is the blob's length."""
    off, o = {}, 0
    for l, (_, _, cin, cout, k) in enumerate(LPIPS_CONVS):
        off[f"w{l}"] = o
        o += cout * k * k * cin
    for name in ("b", "lin"):
        for l, (_, _, _, cout, _) in enumerate(LPIPS_CONVS):
            off[f"{name}{l}"] = o
            o += cout
    off["shift"], off["scale"], off["size"] = o, o + 3, o + 6
    return off


def _sd_get(sd, keys, shape, what):
    for k in keys:
        if k in sd:
            t = sd[k]
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"LPIPS {what}: {k} has shape {tuple(t.shape)}, expected {tuple(shape)}")
            return t.detach().to("cpu", torch.float32)
    raise ValueError(f"LPIPS {what}: missing key {keys[0]}" + (f" (or {', '.join(keys[1:])})" if keys[1:] else ""))


def lpips_pack_params(alexnet_sd: dict, lin_sd: Optional[dict] = None) -> torch.Tensor:
    """State dicts -> the fp32 parameter blob of vd_lpips_pairs (CPU, 1-D).  Either the torchvision
    AlexNet state dict (features.{0,3,6,8,10}.{weight,bias}; classifier keys ignored) with the lpips
    package's alex.pth (lin{0..4}.model.1.weight, [1, C, 1, 1]) as lin_sd, or, with lin_sd None, one
    full lpips.LPIPS.state_dict() (net.slice{1..5}.{0,3,6,8,10}.*, lin{l} / lins.{l}, optionally
    scaling_layer.shift / .scale).  Conv weights are repacked OIHW -> OHWI."""
    full = lin_sd is None
    lin_sd = alexnet_sd if full else lin_sd
    off = lpips_param_offsets()
    blob = torch.zeros(off["size"], dtype=torch.float32)
    for l, (idx, sl, cin, cout, k) in enumerate(LPIPS_CONVS):
        stem = f"net.slice{sl}.{idx}" if full else f"features.{idx}"
        w = _sd_get(alexnet_sd, [f"{stem}.weight"], (cout, cin, k, k), "AlexNet weights")
        b = _sd_get(alexnet_sd, [f"{stem}.bias"], (cout,), "AlexNet weights")
        lin = _sd_get(lin_sd, [f"lin{l}.model.1.weight", f"lins.{l}.model.1.weight"], (1, cout, 1, 1), "lin weights")
        blob[off[f"w{l}"]:off[f"w{l}"] + w.numel()] = w.permute(0, 2, 3, 1).reshape(-1)
        blob[off[f"b{l}"]:off[f"b{l}"] + cout] = b
        blob[off[f"lin{l}"]:off[f"lin{l}"] + cout] = lin.reshape(-1)
    shift, scale = torch.tensor(LPIPS_SHIFT), torch.tensor(LPIPS_SCALE)
    if full and "scaling_layer.shift" in alexnet_sd:
        shift = _sd_get(alexnet_sd, ["scaling_layer.shift"], (1, 3, 1, 1), "scaling layer").reshape(3)
        scale = _sd_get(alexnet_sd, ["scaling_layer.scale"], (1, 3, 1, 1), "scaling layer").reshape(3)
    blob[off["shift"]:off["shift"] + 3] = shift
    blob[off["scale"]:off["scale"] + 3] = scale
    return blob


def lpips_synthetic_state_dicts(seed: int):
    """Seeded stand-ins for the two checkpoints (torchvision AlexNet layout, lpips alex.pth layout):
    conv weights randn * sqrt(2 / (Cin k^2)), biases 0.1 randn, lin |randn| / sqrt(C), all fp32."""
    g = torch.Generator().manual_seed(seed)
    alex, lin = {}, {}
    for l, (idx, _, cin, cout, k) in enumerate(LPIPS_CONVS):
        alex[f"features.{idx}.weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        alex[f"features.{idx}.bias"] = 0.1 * torch.randn(cout, generator=g)
        lin[f"lin{l}.model.1.weight"] = (torch.randn(cout, generator=g).abs() / cout ** 0.5).reshape(1, cout, 1, 1)
    return alex, lin


class LPIPS:
    """lpips.LPIPS(net='alex', version='0.1') in eval mode over consecutive frames, on the GPU in
    exact fp32 (vd_lpips_pairs).  Holds the packed parameter blob on `device`."""

    def __init__(self, params: torch.Tensor, device="cuda"):
        n = lpips_param_offsets()["size"]
        if params.dim() != 1 or params.numel() != n or params.dtype != torch.float32:
            raise ValueError(f"LPIPS parameter blob must be fp32 [{n}], got {params.dtype} {tuple(params.shape)}")
        self.params = params.to(device).contiguous()

    @classmethod
    def from_state_dicts(cls, alexnet_sd: dict, lin_sd: Optional[dict] = None, device="cuda") -> "LPIPS":
        return cls(lpips_pack_params(alexnet_sd, lin_sd), device)

    @classmethod
    def from_files(cls, alexnet_path, lin_path=None, device="cuda") -> "LPIPS":
        """Local checkpoint files only (nothing is ever downloaded): the torchvision AlexNet
        checkpoint plus the lpips package's alex.pth, or one saved lpips.LPIPS.state_dict()."""
        def load(path):
            f = Path(path)
            if not f.is_file():
                raise FileNotFoundError(f"LPIPS.from_files: {str(path)!r} is not a local file")
            return torch.load(f, map_location="cpu", weights_only=True)
        return cls.from_state_dicts(load(alexnet_path), None if lin_path is None else load(lin_path), device)

    @classmethod
    def synthetic(cls, seed: int = 0, device="cuda") -> "LPIPS":
        return cls.from_state_dicts(*lpips_synthetic_state_dicts(seed), device=device)

    def __call__(self, videos_u8: torch.Tensor, workspace_cap: int = LPIPS_WORKSPACE_CAP) -> torch.Tensor:
        """uint8 [V, F, H, W, 3] on the GPU -> fp64 [V, F-1] = LPIPS(frame f, frame f+1).  Runs over
        groups of whole videos whose feature workspace stays under `workspace_cap`."""
        if not self.params.is_cuda:
            raise ValueError("LPIPS runs on the GPU only (its parameters are on the CPU); no CPU fallback")
        x = _u8_videos(videos_u8)
        V, Fr, H, W = x.shape[:4]
        per_video = int(lib().vd_lpips_workspace(Fr, H, W))
        if Fr < 2 or per_video < 0:
            raise ValueError(f"LPIPS needs at least 2 frames of at least 31x31, got {tuple(x.shape)}")
        group = max(1, min(V, min(int(workspace_cap), 4 << 30) // per_video))
        ws = torch.empty(int(lib().vd_lpips_workspace(group * Fr, H, W)), device=x.device, dtype=torch.uint8)
        out = torch.empty(V, Fr - 1, device=x.device, dtype=torch.float64)
        stream = torch.cuda.current_stream().cuda_stream
        for v0 in range(0, V, group):
            n = min(group, V - v0)
            check(lib().vd_lpips_pairs(x[v0:v0 + n].data_ptr(), n, Fr, H, W, self.params.data_ptr(),
                                       out[v0:v0 + n].data_ptr(), ws.data_ptr(), ws.numel(), stream),
                  "vd_lpips_pairs")
        return out


def measure_videos(videos_u8: torch.Tensor, lpips=None, flow: bool = True,
                   workspace_cap: int = FLOW_WORKSPACE_CAP) -> list:
    """uint8 [V, F, H, W, 3] (GPU) -> one record per video (flow fields from the HIP Farneback
    pipeline unless flow=False).  The flow pass runs over groups of videos whose workspace
    (~112 B per pixel-frame) stays under `workspace_cap`, so the reference's 78-video grid does
    not need ~37 GB at once; videos too short or small for Farneback (fewer than 2 frames,
    H or W < 8) keep their flow fields None, as 06 leaves them when it has no pair.
    `lpips`: None (the LPIPS fields stay None), per-video lists of per-pair values, or an LPIPS
    instance, which computes them here."""
    if isinstance(lpips, LPIPS):
        lpips = lpips(videos_u8).cpu().tolist()
    sse, sad = frame_sums(videos_u8)
    sse, sad = sse.cpu().tolist(), sad.cpu().tolist()
    n = int(np.prod(videos_u8.shape[2:]))
    recs = [video_metrics(sse[v], sad[v], n, None if lpips is None else lpips[v]) for v in range(len(sse))]
    V, Fr, H, W = videos_u8.shape[:4]
    if flow and Fr >= 2 and H >= 8 and W >= 8:
        hw = int(H * W)
        per_video = max(int(lib().vd_farneback_workspace(1, Fr, H, W)), 1)
        group = max(1, min(V, workspace_cap // per_video))
        st = []
        for v0 in range(0, V, group):
            part = videos_u8[v0:v0 + group]
            st += flow_sums(part, farneback_flow(part)).cpu().tolist()
        for rec, s in zip(recs, st):
            ff = flow_fields(s, hw)
            for fm, pm in zip(rec["frame_metrics"], ff.pop("pairs")):
                fm.update(pm)
            rec.update(ff)
    return recs


def frames_from_video(video: torch.Tensor) -> torch.Tensor:
    """Pipeline output (B, F, 3, H, W) in [0, 1] -> uint8 [B, F, H, W, 3] as the reference saves
    its PNG frames (numpy_to_pil: (x * 255).round())."""
    return (video.permute(0, 1, 3, 4, 2) * 255).round().to(torch.uint8)
