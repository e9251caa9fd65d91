"""Writes tests/golden/ip_adapter_vision.npz: transformers' OWN CLIPVisionModelWithProjection
outputs for the two tiny vision configs of tests/ip_adapter_ref.py (d = 32 with 17 tokens and
quick_gelu; d = 80 with 5 tokens and gelu), loaded with vision_synthetic_state_dict(cfg, 0) and
run on vision_fixture_pixels(cfg) in fp32 on the CPU: image_embeds, last_hidden_state, the
pixel values and a checksum of the weights.  The transformers version is stored in the file.

Run from the repository root:
    python tests/golden/make_ip_adapter_golden.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))

import ip_adapter_ref as ref  # noqa: E402


def main():
    import transformers
    out = {"transformers_version": np.array(transformers.__version__)}
    for name, cfg in ref.VISION_TINY.items():
        m = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**cfg)).eval()
        sd = ref.vision_synthetic_state_dict(cfg, 0)
        m.load_state_dict(sd, strict=True)
        px = ref.vision_fixture_pixels(cfg)
        with torch.no_grad():
            o = m(pixel_values=px)
        out[f"{name}.pixel_values"] = px.numpy()
        out[f"{name}.image_embeds"] = o.image_embeds.numpy()
        out[f"{name}.last_hidden_state"] = o.last_hidden_state.numpy()
        out[f"{name}.weight_checksum"] = np.array(sum(v.double().abs().sum().item() for v in sd.values()))
    path = ROOT / "tests" / "golden" / "ip_adapter_vision.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
