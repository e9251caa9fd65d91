"""FreeNoise prompt travel reference (test infrastructure, CPU): diffusers'
`AnimateDiffFreeNoiseMixin._encode_prompt_free_noise` (the {frame: text} dict's normalisation and
the default linear `prompt_interpolation_callback`) and the UNet forward in which every frame's
spatial cross-attention reads its own text, restated on top of oracle/unet_ref.py and
tests/free_noise_ref.py.

PARITY STATUS: diffusers is not installed here, so this is a restatement from its published
source, unpinned like the rest of oracle/.  One known difference: diffusers interpolates with
torch.linspace weights in the embeddings' dtype; here the weight of frame f between the key frames
i0 < i1 is the fp32 quotient float(f - i0) / float(i1 - i0) (what the device computes) and the
interpolation itself runs in fp64.
"""
from __future__ import annotations

import contextlib

import torch

import free_noise_ref
from oracle import unet_ref


def normalise_prompt(prompt, num_frames, name="prompt"):
    """One side of _encode_prompt_free_noise: a str is {0: str}; int keys and str values; sorted
    by frame; the first key 0; the last key <= num_frames - 1, where the last prompt is repeated
    when no key names that frame -> (frame indices, texts).  The rule is a dozen lines of host
    Python, so this is the same text as AnimateDiffPipeline._prompt_travel_keys, not an independent
    derivation: tests/test_prompt_travel_host.py holds BOTH to literal expectations."""
    if isinstance(prompt, str):
        prompt = {0: prompt}
    if not isinstance(prompt, dict):
        raise ValueError(f"Expected `{name}` to be either `str` or `dict`, got {type(prompt).__name__}.")
    if not prompt or not all(isinstance(k, int) and not isinstance(k, bool) for k in prompt) or \
            not all(isinstance(v, str) for v in prompt.values()):
        raise ValueError(f"Expected integer keys and string values for `{name}` dict.")
    frames = sorted(prompt)
    if frames[0] != 0:
        raise ValueError(f"The minimum frame index in `{name}` dict must be 0 or missing.")
    if frames[-1] >= num_frames:
        raise ValueError(f"The maximum frame index in `{name}` dict must be lesser than `num_frames` and follow "
                         "0-based indexing.")
    texts = [prompt[f] for f in frames]
    if frames[-1] != num_frames - 1:
        frames, texts = frames + [num_frames - 1], texts + [texts[-1]]
    return frames, texts


def check_indices(idx, F):
    idx = [int(i) for i in idx]
    if any(b <= a for a, b in zip(idx, idx[1:])):
        raise ValueError(f"frame indices {idx} are not strictly increasing")
    if idx[0] != 0:
        raise ValueError(f"the first frame index must be 0, got {idx[0]}")
    if idx[-1] != F - 1:
        raise ValueError(f"the last frame index must be {F - 1}, got {idx[-1]}")
    return idx


def lerp_ref(keys, idx, F):
    """keys [..., K, L, C] (any float dtype), idx the K key frames -> fp64 [..., F, L, C]: frame
    idx[k] is key k exactly; a frame between idx[k] and idx[k + 1] is (1 - w) * a + w * b in fp64,
    with w the fp32 quotient float(f - idx[k]) / float(idx[k + 1] - idx[k])."""
    idx = check_indices(idx, F)
    keys = keys.double()
    out = torch.empty(keys.shape[:-3] + (F,) + keys.shape[-2:], dtype=torch.float64)
    for k, i0 in enumerate(idx):
        out[..., i0, :, :] = keys[..., k, :, :]
        if k + 1 < len(idx):
            i1 = idx[k + 1]
            for f in range(i0 + 1, i1):
                w = (torch.tensor(float(f - i0), dtype=torch.float32) /
                     torch.tensor(float(i1 - i0), dtype=torch.float32)).double()
                out[..., f, :, :] = (1.0 - w) * keys[..., k, :, :] + w * keys[..., k + 1, :, :]
    return out


def lerp_operands(keys, idx, F):
    """max(|a|, |b|) per output element, fp64 [..., F, L, C]: the two keys a frame is mixed from
    (the key itself on a key frame).  The absolute slack of the device bound scales with it."""
    idx = check_indices(idx, F)
    keys = keys.double().abs()
    out = torch.empty(keys.shape[:-3] + (F,) + keys.shape[-2:], dtype=torch.float64)
    for k, i0 in enumerate(idx):
        out[..., i0, :, :] = keys[..., k, :, :]
        if k + 1 < len(idx):
            for f in range(i0 + 1, idx[k + 1]):
                out[..., f, :, :] = torch.maximum(keys[..., k, :, :], keys[..., k + 1, :, :])
    return out


@contextlib.contextmanager
def _text(ehs_frames):
    """Inside the block every spatial transformer of oracle/unet_ref reads ehs_frames, whatever
    text the forward hands it (unet_forward_free_noise looks transformer2d up on the module at each
    call).  Restored on exit."""
    plain = unet_ref.transformer2d

    def transformer2d(sd, p, x, ehs, *args, **kwargs):
        return plain(sd, p, x, ehs_frames, *args, **kwargs)

    unet_ref.transformer2d = transformer2d
    try:
        yield
    finally:
        unet_ref.transformer2d = plain


def unet_forward_per_frame(sd, cfg, sample, timestep, ehs, free_noise=None, act="fp32"):
    """tests/free_noise_ref.unet_forward_free_noise with the text's repeat_interleave(F) skipped
    when `ehs` already has B * F rows (video-major, then frame): every frame's spatial
    cross-attention reads its own [L, D] text.  With B rows it IS unet_forward_free_noise.  The
    per-frame text passes through the same rounder as the per-video text does."""
    b, nf = sample.shape[0], sample.shape[2]
    if ehs.shape[0] == b:
        return free_noise_ref.unet_forward_free_noise(sd, cfg, sample, timestep, ehs, free_noise, act)
    if ehs.shape[0] != b * nf:
        raise ValueError(f"{ehs.shape[0]} text rows for {b} videos of {nf} frames: expected {b} or {b * nf}")
    frames = unet_ref.ROUNDERS[act](ehs.float())
    with _text(frames):
        # the per-video text handed down is never read: each video's frame 0, for the shapes alone
        return free_noise_ref.unet_forward_free_noise(sd, cfg, sample, timestep, ehs[::nf], free_noise, act)
