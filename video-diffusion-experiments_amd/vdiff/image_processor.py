"""transformers.CLIPImageProcessor with CLIP's defaults, on the host with PIL (once per video):
RGB conversion, bicubic resize of the shortest edge to 224, centre crop to 224, / 255, and
normalisation by CLIP's mean and std -> pixel_values (B, 3, 224, 224) fp32.

Accepted inputs: a PIL image, an ndarray (H, W, 3) uint8 or float in [0, 1], a tensor (3, H, W)
or (H, W, 3) of either kind, or a list of those.  Everything goes through PIL in uint8, as
transformers' slow processor does, so the resize is PIL's own bicubic filter.
"""
from __future__ import annotations

import numpy as np
import torch

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


class ImageBatch(dict):
    """transformers' BatchFeature as the pipelines read it: ["pixel_values"] and .pixel_values."""

    @property
    def pixel_values(self):
        return self["pixel_values"]


class CLIPImageProcessor:
    def __init__(self, size: int = 224, crop_size: int = 224, image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD):
        self.size, self.crop_size = int(size), int(crop_size)
        self.image_mean, self.image_std = tuple(image_mean), tuple(image_std)

    @staticmethod
    def to_pil(image):
        from PIL import Image
        if isinstance(image, Image.Image):
            return image.convert("RGB")
        a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
        if a.ndim != 3 or 3 not in (a.shape[0], a.shape[-1]):
            raise ValueError(f"an image must be (H, W, 3) or (3, H, W), got {a.shape}")
        if a.shape[-1] != 3:
            a = a.transpose(1, 2, 0)
        if a.dtype != np.uint8:
            a = (np.clip(a.astype(np.float64), 0.0, 1.0) * 255.0).round().astype(np.uint8)
        return Image.fromarray(a, "RGB")

    def resize_crop(self, img):
        """Shortest edge to `size` (bicubic; the long edge int(size * long / short), as transformers'
        get_resize_output_image_size), then the centre crop transformers takes."""
        from PIL import Image
        w, h = img.size
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = self.size, int(self.size * long / short)
        nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
        img = img.resize((nw, nh), Image.BICUBIC)
        c = self.crop_size
        top, left = (nh - c) // 2, (nw - c) // 2
        return img.crop((left, top, left + c, top + c))

    def __call__(self, images, return_tensors="pt", **unused):
        if return_tensors != "pt":
            raise NotImplementedError("return_tensors: 'pt' only")
        if not isinstance(images, (list, tuple)):
            images = [images]
        out = []
        mean = np.asarray(self.image_mean, np.float32)
        std = np.asarray(self.image_std, np.float32)
        for im in images:
            a = np.asarray(self.resize_crop(self.to_pil(im)), np.float32) * np.float32(1 / 255)
            out.append(torch.from_numpy(((a - mean) / std).transpose(2, 0, 1).copy()))
        return ImageBatch(pixel_values=torch.stack(out))
