"""The tiny-UNet case the prompt-travel tests share (test infrastructure, CPU): the model, its
inputs and the CPU references, each computed once per process."""
from __future__ import annotations

import functools

import torch

import prompt_travel_ref as P
from vdiff import UNetMotionModel, init_synthetic_
from vdiff.config import TINY

BF = torch.bfloat16
FN = (4, 2, "pyramid")  # context_length, context_stride, weighting_scheme
IDX = {7: [0, 2, 6], 6: [0, 2, 5]}  # the key frames of the three key prompts

# BAR = 1.3 x the larger of two measurements on this model and these inputs, as
# tests/test_gpu_free_noise.py sets its bar (1.3 x is the headroom test_tiny_unet_matches_oracle keeps):
#   the bf16-emulating CPU reference against the fp32 one, per-frame text, FreeNoise on / off:
#     0.01535 / 0.01593 (F = 6), 0.01578 / 0.01603 (F = 7); 0.01568 / 0.01584 and 0.01575 / 0.01605 on
#     another host's CPU (another BLAS blocking)
#   the device on the parent's path, the same sharpened model with per-video text on the fast path,
#     against its fp32 reference, FreeNoise on / off: 0.01579 / 0.01564 (F = 6), 0.01606 / 0.01608 (F = 7)
# so BAR = 1.3 x 0.01608.  What the device measures against it with per-frame text is written above
# the tests in tests/test_gpu_prompt_travel.py.
BAR = 1.3 * 0.01608


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).norm() / want.norm()).item()


def sharpened_(model):
    """tests/test_gpu_free_noise.py's sharpened_ (every motion module's to_q / to_k x 8, its
    proj_out x 4), and the text made to matter: every spatial attn2.to_q / to_k x 8 and attn2.to_v
    x 32.  With the stock synthetic weights the text moves the UNet output by 0.0024 rel-L2, far
    below the bf16 path's own distance from the fp32 reference, and nothing about which frame
    reads which text could be seen.  Powers of two: the values stay bf16."""
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "motion_modules." in n:
                if n.endswith(("to_q.weight", "to_k.weight")):
                    p.mul_(8)
                elif n.endswith("proj_out.weight") and "transformer_blocks" not in n:
                    p.mul_(4)
            elif ".attn2." in n:
                if n.endswith(("to_q.weight", "to_k.weight")):
                    p.mul_(8)
                elif n.endswith("to_v.weight"):
                    p.mul_(32)
    return model


def latents(F, seed):
    return torch.randn(1, 4, F, 16, 16, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def model():
    """(the sharpened tiny model on the CPU, its fp32 state dict)."""
    m = sharpened_(init_synthetic_(UNetMotionModel("tiny"), seed=0))
    return m, {k: v.float() for k, v in m.state_dict().items()}


@functools.lru_cache(maxsize=None)
def keys():
    """Three key prompts for either CFG half: [2, 3, 77, 64], bf16 values in fp32."""
    return torch.randn(2, 3, 77, 64, generator=torch.Generator().manual_seed(1234)).to(BF).float()


@functools.lru_cache(maxsize=None)
def case(F):
    """F frames of 16 x 16 latents duplicated to CFG batch 2, the per-frame text [2 * F, 77, 64]
    (the key prompts interpolated in fp64 and rounded to bf16 once, what the device rows hold) and
    the per-video text of the parent's path (the first key prompt of either half)."""
    lat = latents(F, 100 + F)
    pf = P.lerp_ref(keys(), IDX[F], F).to(BF).float().reshape(2 * F, 77, 64)
    return dict(lat=lat, x2=torch.cat([lat, lat]), pf=pf, pv=keys()[:, 0].contiguous())


@functools.lru_cache(maxsize=None)
def reference(F, free_noise, act="fp32", text="pf"):
    """The CPU reference of the case: text "pf" per frame, "pv" per video, or a planted fault of the
    per-frame text: "frame0" (every frame reads frame 0's text: a kv_div that stays `frames`),
    "rolled" (an off-by-one frame index), "swapped" (the CFG halves exchanged)."""
    _, sd = model()
    c = case(F)
    pf = c["pf"].view(2, F, 77, 64)
    ehs = {"pf": pf, "pv": None, "frame0": pf[:, :1].expand(-1, F, -1, -1), "rolled": pf.roll(1, 1),
           "swapped": pf.flip(0)}[text]
    ehs = c["pv"] if ehs is None else ehs.reshape(2 * F, 77, 64)
    with torch.no_grad():
        return P.unet_forward_per_frame(sd, TINY, c["x2"], 961, ehs, FN if free_noise else None, act)
