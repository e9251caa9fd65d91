"""LoRA loading on the CPU (tiny UNet, bf16 parameters as on the device, nothing prepared): the
four key layouts, the merge formula, adapter weights, restoring the base, and the refusals."""
import pytest
import torch

import lora_ref as R
from vdiff import AnimateDiffPipeline, UNetMotionModel, init_synthetic_, lora
from vdiff import pretrained as P


@pytest.fixture()
def unet():
    return init_synthetic_(UNetMotionModel("tiny"), seed=0).to(torch.bfloat16)


def weights(unet, modules):
    sd = unet.state_dict()
    return {m: sd[m + ".weight"].clone() for m in modules}


def same(a, b):
    return all(torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)) for k in a) and set(a) == set(b)


def test_the_four_layouts_merge_to_identical_weights(unet):
    lo = R.make_lora(unet, alpha=2.0)
    base = weights(unet, R.MODULES)
    got = {}
    for name, sd in (("peft", R.write_peft(lo)), ("legacy", R.write_legacy(lo)), ("kohya", R.write_kohya(lo))):
        assert unet.load_lora_state_dict(sd) == "default_0"
        got[name] = weights(unet, R.MODULES)
        assert not any(torch.equal(got[name][m], base[m]) for m in R.MODULES), name  # every target moved
        unet.unload_lora()
        assert same(weights(unet, R.MODULES), base)
    assert same(got["peft"], got["legacy"]) and same(got["peft"], got["kohya"])
    # (d) has no alpha key: alpha = r, motion-module attention only
    lm = R.make_lora(unet, modules=R.MOTION_ATTN, alpha=4.0)
    unet.load_lora_state_dict(R.write_motion(lm))
    d = weights(unet, R.MOTION_ATTN)
    unet.unload_lora()
    unet.load_lora_state_dict(R.write_peft(lm, alpha=False))  # alpha defaults to r
    assert same(weights(unet, R.MOTION_ATTN), d)
    assert not any(torch.equal(d[m], base[m]) for m in R.MOTION_ATTN)


def test_merged_linear_is_the_fp64_formula_rounded_once(unet):
    m = R.SPATIAL + "attn1.to_q"
    w0 = unet.state_dict()[m + ".weight"].clone()
    lo = R.make_lora(unet, modules=(m,), r=4, alpha=2.0)
    unet.load_lora_state_dict(R.write_peft(lo), adapter_name="a")
    unet.set_adapters("a", 0.75)
    A, B, al = lo[m]
    want = (w0.double() + 0.75 * (al / 4) * (B.double() @ A.double())).to(torch.bfloat16)
    got = unet.state_dict()[m + ".weight"]
    assert got.dtype == torch.bfloat16 and torch.equal(got, want) and not torch.equal(got, w0)


def test_conv3x3_lora_is_the_composition_of_its_two_convs(unet):
    m = "down_blocks.0.resnets.0.conv1"
    lo = R.make_lora(unet, modules=(m,), r=4)
    A, B, _ = lo[m]
    shape = unet.state_dict()[m + ".weight"].shape
    delta = lora.lora_delta(A, B, shape, dtype=torch.float64)  # before any rounding
    assert delta.dtype == torch.float64 and delta.shape == shape
    x = torch.randn(2, shape[1], 9, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    conv = torch.nn.functional.conv2d
    want = conv(conv(x, A.double(), padding=1), B.double())
    got = conv(x, delta, padding=1)
    assert ((got - want).norm() / want.norm()).item() < 1e-12


def test_two_adapters_sum_with_their_weights(unet):
    a = R.make_lora(unet, seed=1)
    b = R.make_lora(unet, modules=R.MODULES[:6] + R.MODULES[10:12], seed=2, r=2, alpha=2.0)
    base = {k: v.clone() for k, v in unet.state_dict().items()}
    unet.load_lora_state_dict(R.write_peft(a), adapter_name="a")
    unet.load_lora_state_dict(R.write_kohya(b), adapter_name="b")
    assert unet.get_active_adapters() == ["a", "b"]
    unet.set_adapters(["a", "b"], [1.0, 0.5])
    want = R.merged_state_dict(base, [(a, 1.0), (b, 0.5)])
    got = unet.state_dict()
    assert all(torch.equal(got[k], want[k]) for k in want)
    # only "a": b's share is gone, not merely scaled
    unet.set_adapters("a")
    want = R.merged_state_dict(base, [(a, 1.0)])
    assert all(torch.equal(unet.state_dict()[k], want[k]) for k in want)
    unet.delete_adapters("a")
    assert unet.get_active_adapters() == []
    assert all(torch.equal(unet.state_dict()[k], base[k]) for k in base)


def test_weight_zero_and_unload_restore_the_base_bit_for_bit(unet):
    base = {k: v.clone() for k, v in unet.state_dict().items()}
    lo = R.make_lora(unet)
    unet.load_lora_state_dict(R.write_peft(lo), adapter_name="x")
    assert not all(torch.equal(unet.state_dict()[k], base[k]) for k in base)
    unet.set_adapters(["x"], [0.0])
    assert same(dict(unet.state_dict()), base)
    unet.set_adapters(["x"], [1.0])
    assert not all(torch.equal(unet.state_dict()[k], base[k]) for k in base)
    unet.unload_lora()
    assert same(dict(unet.state_dict()), base)
    assert unet.get_active_adapters() == [] and unet._lora.base == {}


def test_pipeline_surface_and_files(unet, tmp_path):
    from safetensors.torch import save_file
    pipe = AnimateDiffPipeline(unet, vae=None)
    lo = R.make_lora(unet)
    base = {k: v.clone() for k, v in unet.state_dict().items()}
    want = R.merged_state_dict(base, [(lo, 1.0)])
    save_file({k: v.contiguous() for k, v in R.write_peft(lo).items()}, str(tmp_path / "lcm.safetensors"))
    torch.save(R.write_kohya(lo), str(tmp_path / "pytorch_lora_weights.bin"))
    for src, kw in ((tmp_path / "lcm.safetensors", {}), (tmp_path, {}), (str(tmp_path), dict(weight_name="pytorch_lora_weights.bin"))):
        assert pipe.load_lora_weights(src, adapter_name="lcm", **kw) == "lcm"
        assert pipe.get_active_adapters() == ["lcm"]
        assert all(torch.equal(unet.state_dict()[k], want[k]) for k in want)
        pipe.unload_lora_weights()
        assert same(dict(unet.state_dict()), base)
    pipe.load_lora_weights(R.write_peft(lo), adapter_name="lcm")
    pipe.fuse_lora(lora_scale=0.5)
    half = R.merged_state_dict(base, [(lo, 0.5)])
    assert all(torch.equal(unet.state_dict()[k], half[k]) for k in half)
    pipe.unfuse_lora()
    assert all(torch.equal(unet.state_dict()[k], want[k]) for k in want)
    pipe.delete_adapters("lcm")
    assert same(dict(unet.state_dict()), base)
    with pytest.raises(FileNotFoundError, match="local"):
        pipe.load_lora_weights("wangfuyun/AnimateLCM")


def test_errors(unet):
    lo = R.make_lora(unet, modules=R.MODULES[:2])
    sd = R.write_peft(lo)
    bad = dict(sd)
    bad["unet.down_blocks.9.attentions.0.proj_in.lora_A.weight"] = torch.zeros(4, 64)
    bad["unet.down_blocks.9.attentions.0.proj_in.lora_B.weight"] = torch.zeros(64, 4)
    with pytest.raises(KeyError, match="down_blocks.9"):
        unet.load_lora_state_dict(bad)
    with pytest.raises(KeyError, match="map to no module"):
        unet.load_lora_state_dict({"unet.conv_in.lora_A.weight": torch.zeros(4, 4, 3, 3),
                                   "unet.conv_in.lora_B.weight": torch.zeros(64, 4, 1, 1)})  # not a target
    for k in ("text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight",
              "lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight"):
        with pytest.raises(NotImplementedError, match="text-encoder"):
            unet.load_lora_state_dict({**sd, k: torch.zeros(4, 4)})
    m = R.MODULES[0]
    with pytest.raises(ValueError, match="do not fit"):
        unet.load_lora_state_dict({f"unet.{m}.lora_A.weight": torch.zeros(4, 63), f"unet.{m}.lora_B.weight": torch.zeros(64, 4)})
    with pytest.raises(KeyError, match="only one"):
        unet.load_lora_state_dict({f"unet.{m}.lora_A.weight": torch.zeros(4, 64)})
    assert unet.get_active_adapters() == [] and unet._lora.base == {} and unet._lora.adapters == {}  # nothing half-loaded
    unet.load_lora_state_dict(sd, adapter_name="a")
    with pytest.raises(ValueError, match="already loaded"):
        unet.load_lora_state_dict(sd, adapter_name="a")
    with pytest.raises(ValueError, match="not loaded"):
        unet.set_adapters("b")
    with pytest.raises(ValueError, match="adapter weights"):
        unet.set_adapters(["a"], [1.0, 2.0])


def test_ambiguous_kohya_name_is_refused():
    names = {"blk.attentions.0.to_q", "blk.attentions_0.to_q"}
    sd = {"lora_unet_blk_attentions_0_to_q.lora_down.weight": torch.zeros(2, 4),
          "lora_unet_blk_attentions_0_to_q.lora_up.weight": torch.zeros(4, 2)}
    with pytest.raises(ValueError, match="more than one module"):
        lora.parse_lora_state_dict(sd, names)


def test_time_cond_proj_dim_is_refused_by_name():
    cfg = dict(block_out_channels=(320, 640, 1280, 1280), down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",),
               up_block_types=("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3, attention_head_dim=8)
    P.motion_unet_config(cfg, {})
    with pytest.raises(NotImplementedError, match="time_cond_proj_dim"):
        P.motion_unet_config({**cfg, "time_cond_proj_dim": 256}, {})
