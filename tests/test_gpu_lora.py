"""LoRA loading on the MI355X (tiny UNet): a loaded LoRA against a second UNet whose state dict
was merged offline, against the CPU oracle on the merged weights, unloading, and switching
adapters between two pipeline calls."""
from pathlib import Path

import numpy as np
import pytest
import torch

import lora_ref as R
from oracle import unet_ref
from vdiff import AnimateDiffPipeline, DDIMScheduler, UNetMotionModel, init_synthetic_
from vdiff.config import TINY

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
BF = torch.bfloat16
# the bound tests/test_gpu_unet.py::test_tiny_unet_matches_oracle holds the tiny UNet to (rel-L2
# against the fp32 oracle; measured 0.0137-0.0138 there)
BAR = 0.018


def rel_l2(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).norm() / want.norm()).item()


def fresh_unet():
    return init_synthetic_(UNetMotionModel("tiny"), seed=0).to("cuda", BF)


@pytest.fixture(scope="module")
def tiny(cuda):
    """The tiny UNet on the golden inputs cut to 2 frames x 32^2, its output before any LoRA, one
    LoRA touching every kind of target (std 0.1: on the CPU oracle it moves the output by 0.78
    rel-L2, and the device-emulating oracle stays 0.0141 from the fp32 one on the merged weights),
    and the state dict merged offline."""
    unet = fresh_unet().prepare()
    g = np.load(GOLD / "tiny_unet.npz")
    lat = torch.from_numpy(g["latents"])[:, :, :2, :32, :32].contiguous()
    ehs = torch.from_numpy(g["ehs"])
    x2 = torch.cat([lat, lat])
    base_sd = {k: v.clone() for k, v in unet.state_dict().items()}
    lo = R.make_lora(unet, alpha=2.0, std=0.1)
    merged = R.merged_state_dict(base_sd, [(lo, 1.0)])
    run = lambda u: u(x2.cuda(), 961, encoder_hidden_states=ehs.cuda()).sample.clone()  # noqa: E731
    return dict(unet=unet, lat=lat, ehs=ehs, x2=x2, base_sd=base_sd, lora=lo, merged=merged, run=run,
                base_out=run(unet))


@pytest.fixture
def loaded(tiny):
    tiny["unet"].load_lora_state_dict(R.write_peft(tiny["lora"]), adapter_name="a")
    yield tiny["unet"]
    tiny["unet"].unload_lora()


def test_loaded_lora_equals_an_offline_merge_bit_for_bit(tiny, loaded):
    for need in ("attn1.to_q", "attn2.to_k", "ff.net.0.proj", "ff.net.2", ".motion_modules.", "resnets.0.conv1"):
        assert any(need in m for m in tiny["lora"]), need
    got = tiny["run"](loaded)
    other = fresh_unet()
    other.load_state_dict(tiny["merged"])
    want = tiny["run"](other.prepare())
    assert all(torch.equal(loaded.state_dict()[k], tiny["merged"][k]) for k in tiny["merged"])
    assert torch.equal(got, want)
    d = rel_l2(got, tiny["base_out"])
    print(f"LoRA on vs off rel-L2 {d:.4f}")
    assert d > 5 * BAR, d  # a LoRA that is not applied cannot pass the parity test below


def test_loaded_lora_matches_the_oracle_on_the_merged_weights(tiny, loaded):
    sd = {k: v.float().cpu() for k, v in tiny["merged"].items()}
    with torch.no_grad():
        want = unet_ref.unet_forward(sd, TINY, tiny["x2"], 961, tiny["ehs"])
    err = rel_l2(tiny["run"](loaded), want)
    print(f"tiny UNet + LoRA rel-L2 vs fp32 oracle {err:.5f}; base output vs that oracle "
          f"{rel_l2(tiny['base_out'], want):.5f}")
    assert err < BAR, err


def test_unload_restores_the_base_output_bit_for_bit(tiny):
    u = tiny["unet"]
    u.load_lora_state_dict(R.write_kohya(tiny["lora"]))
    assert not torch.equal(tiny["run"](u), tiny["base_out"])
    u.unload_lora()
    assert all(torch.equal(u.state_dict()[k], tiny["base_sd"][k]) for k in tiny["base_sd"])
    assert torch.equal(tiny["run"](u), tiny["base_out"])


def test_set_adapters_between_two_pipeline_calls_takes_effect(tiny):
    """No stale loop, graph or cross-attention K/V cache: the second call runs the new weights."""
    u = tiny["unet"]
    pipe = AnimateDiffPipeline(u, DDIMScheduler(beta_schedule="linear", steps_offset=1, clip_sample=False))
    neg, pos = tiny["ehs"].chunk(2)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=tiny["lat"], num_frames=2, height=256, width=256,
              num_inference_steps=2, guidance_scale=7.5, output_type="latent")
    try:
        base = pipe(**kw).frames.clone()
        pipe.load_lora_weights(R.write_peft(tiny["lora"]), adapter_name="a")
        on = pipe(**kw).frames.clone()
        pipe.set_adapters("a", 0.0)
        off = pipe(**kw).frames.clone()
        pipe.set_adapters("a", 1.0)
        again = pipe(**kw).frames.clone()
    finally:
        pipe.unload_lora_weights()
    assert not torch.equal(on, base)
    assert torch.equal(off, base)
    assert torch.equal(again, on)
    assert torch.equal(pipe(**kw).frames, base)
