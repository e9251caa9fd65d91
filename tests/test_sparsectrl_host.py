"""SparseCtrl on the host: the config translation and its refusals, the module tree's key set
against diffusers' names written out here, the restatement's conditioning against hand-written
expectations, ops.sparse_cond's index validation (before any library call), the pipeline's
refusals, and what the restatement itself must show for the GPU tests to mean anything: the
residuals ignore the latents, the motion modules carry a key frame to the last frame, and only the
conditioning embedding reads the condition (tests/sparsectrl_ref.py)."""
import json

import pytest
import torch

import sparsectrl_ref as S
import vdiff
from vdiff import (AnimateDiffSparseControlNetPipeline, SparseControlConditioning, SparseControlNetModel,
                   UNetMotionModel, ops)
from vdiff.models.sparse_controlnet import sparse_controlnet_config, sparse_controlnet_config_from_diffusers


# ---------------------------------------------------------------- config
def test_config_translation_and_refusals():
    cfg = sparse_controlnet_config_from_diffusers({})
    assert cfg == dict(in_channels=4, sample_size=64, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
                       down_block_types=("CrossAttnDownBlockMotion",) * 3 + ("DownBlockMotion",), norm_num_groups=32,
                       norm_eps=1e-5, cross_attention_dim=768, num_attention_heads=8, motion_num_attention_heads=8,
                       motion_max_seq_length=32, conditioning_channels=4,
                       conditioning_embedding_out_channels=(16, 32, 96, 256), concat_conditioning_mask=True,
                       use_simplified_condition_embedding=True)
    assert sparse_controlnet_config_from_diffusers(dict(attention_head_dim=4))["num_attention_heads"] == 4
    assert sparse_controlnet_config_from_diffusers(dict(attention_head_dim=[4, 4]))["num_attention_heads"] == 4
    assert sparse_controlnet_config_from_diffusers(dict(num_attention_heads=2, attention_head_dim=4))[
        "num_attention_heads"] == 2
    assert not sparse_controlnet_config_from_diffusers(dict(use_simplified_condition_embedding=False))[
        "use_simplified_condition_embedding"]
    for extra, match in ((dict(use_linear_projection=True), "use_linear_projection"),
                         (dict(global_pool_conditions=True), "global_pool_conditions"),
                         (dict(controlnet_conditioning_channel_order="bgr"), "channel_order"),
                         (dict(transformer_layers_per_block=2), "transformer_layers_per_block"),
                         (dict(temporal_transformer_layers_per_block=2), "temporal_transformer_layers_per_block"),
                         (dict(only_cross_attention=True), "only_cross_attention"),
                         (dict(layers_per_block=[2, 2, 2, 2]), "per-block layers_per_block"),
                         (dict(attention_head_dim=[5, 10, 20, 20]), "per-block attention heads"),
                         (dict(concat_conditioning_mask=False), "concat_conditioning_mask"),
                         (dict(down_block_types=["CrossAttnDownBlock2D", "DownBlock2D"]), "down_block_types")):
        with pytest.raises(NotImplementedError, match=match):
            sparse_controlnet_config_from_diffusers(extra)
    with pytest.raises(NotImplementedError, match="concat_conditioning_mask"):
        SparseControlNetModel("tiny", concat_conditioning_mask=False)
    tiny = sparse_controlnet_config("tiny")
    assert tiny["block_out_channels"] == vdiff.TINY["block_out_channels"]
    assert tiny["down_block_types"] == ("CrossAttnDownBlockMotion", "DownBlockMotion")
    assert tiny["motion_max_seq_length"] == 32 and tiny["conditioning_embedding_out_channels"] == (16, 32, 32, 64)
    assert "up_block_types" not in tiny and "out_channels" not in tiny


# ---------------------------------------------------------------- the tree, under diffusers' names
def wb(p):
    return [f"{p}.weight", f"{p}.bias"]


def resnet_keys(p, shortcut):
    names = ["norm1", "conv1", "time_emb_proj", "norm2", "conv2"] + (["conv_shortcut"] if shortcut else [])
    return [k for n in names for k in wb(f"{p}.{n}")]


def transformer_keys(p):
    """Transformer2DModel and AnimateDiffTransformer3D share the layout: norm, proj_in, one
    BasicTransformerBlock (to_q / to_k / to_v without bias), proj_out."""
    t = f"{p}.transformer_blocks.0"
    keys = wb(f"{p}.norm") + wb(f"{p}.proj_in") + wb(f"{p}.proj_out")
    for a, n in (("attn1", "norm1"), ("attn2", "norm2")):
        keys += wb(f"{t}.{n}") + [f"{t}.{a}.to_q.weight", f"{t}.{a}.to_k.weight", f"{t}.{a}.to_v.weight"]
        keys += wb(f"{t}.{a}.to_out.0")
    return keys + wb(f"{t}.norm3") + wb(f"{t}.ff.net.0.proj") + wb(f"{t}.ff.net.2")


def expected_keys(channels, layers, simplified):
    keys = wb("conv_in") + wb("time_embedding.linear_1") + wb("time_embedding.linear_2")
    if simplified:
        keys += wb("controlnet_cond_embedding")
    else:
        keys += wb("controlnet_cond_embedding.conv_in") + wb("controlnet_cond_embedding.conv_out")
        keys += [k for i in range(6) for k in wb(f"controlnet_cond_embedding.blocks.{i}")]
    n_zero, prev = 1, channels[0]
    for i, ch in enumerate(channels):
        last = i == len(channels) - 1
        for j in range(layers):
            keys += resnet_keys(f"down_blocks.{i}.resnets.{j}", shortcut=j == 0 and prev != ch)
            if not last:
                keys += transformer_keys(f"down_blocks.{i}.attentions.{j}")
            keys += transformer_keys(f"down_blocks.{i}.motion_modules.{j}")
        if not last:
            keys += wb(f"down_blocks.{i}.downsamplers.0.conv")
        n_zero += layers + (0 if last else 1)
        prev = ch
    keys += [k for i in range(n_zero) for k in wb(f"controlnet_down_blocks.{i}")]
    keys += resnet_keys("mid_block.resnets.0", False) + resnet_keys("mid_block.resnets.1", False)
    keys += transformer_keys("mid_block.attentions.0") + wb("controlnet_mid_block")
    return keys


@pytest.mark.parametrize("simplified", [True, False])
@pytest.mark.parametrize("name,channels,layers,n_res", [("tiny", (64, 128), 1, 5),
                                                        ("full", (320, 640, 1280, 1280), 2, 13)])
def test_state_dict_keys_are_diffusers(name, channels, layers, n_res, simplified):
    extra = {} if simplified else dict(use_simplified_condition_embedding=False, conditioning_channels=3)
    with torch.device("meta"):
        m = SparseControlNetModel(name, **extra)
    got = [k for k in m.state_dict() if not k.endswith(".pos_embed.pe")]  # the PE table is a buffer here
    want = expected_keys(channels, layers, simplified)
    assert len(set(want)) == len(want)
    assert set(got) == set(want), (sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5])
    assert m.num_residuals == n_res
    assert not any("motion_modules" in k for k in got if k.startswith("mid_block"))
    sd = m.state_dict()
    cin = 5 if simplified else 4
    first = "controlnet_cond_embedding.weight" if simplified else "controlnet_cond_embedding.conv_in.weight"
    assert tuple(sd[first].shape) == (channels[0] if simplified else 16, cin, 3, 3)
    if name == "full":
        assert m.residual_channels() == [320] * 4 + [640] * 3 + [1280] * 6
        assert tuple(sd["down_blocks.3.motion_modules.1.proj_in.weight"].shape) == (1280, 1280)
    else:
        assert m.residual_channels() == [c for _, c in UNetMotionModel("tiny").control_residual_shapes(1, 8, 8)]


def test_from_pretrained_local_folder_round_trip(tmp_path):
    from safetensors.torch import save_file
    src = S.random_sparse_controlnet("tiny", seed=3)
    cfg = dict(_class_name="SparseControlNetModel", in_channels=4, conditioning_channels=4,
               block_out_channels=[64, 128], layers_per_block=1,
               down_block_types=["CrossAttnDownBlockMotion", "DownBlockMotion"], attention_head_dim=2,
               cross_attention_dim=64, norm_num_groups=32, motion_num_attention_heads=2, motion_max_seq_length=32,
               conditioning_embedding_out_channels=[16, 32, 32, 64], use_linear_projection=False,
               concat_conditioning_mask=True, use_simplified_condition_embedding=True,
               transformer_layers_per_block=1, temporal_transformer_layers_per_block=1)
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    save_file({k: v.contiguous() for k, v in src.state_dict().items()},
              str(tmp_path / "diffusion_pytorch_model.safetensors"))
    got = SparseControlNetModel.from_pretrained(tmp_path, device="cpu", torch_dtype=torch.float16)
    assert got.dtype == torch.bfloat16 and got.torch_dtype == torch.float16
    want = src.state_dict()
    assert set(got.state_dict()) == set(want)
    for k, v in got.state_dict().items():
        if not k.endswith(".pos_embed.pe"):
            assert torch.equal(v.float(), want[k].float()), k
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        SparseControlNetModel.from_pretrained([tmp_path, tmp_path])
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        got.prepare()


# ---------------------------------------------------------------- the conditioning
def test_restatement_conditioning_by_hand():
    key = torch.arange(1, 1 + 2 * 3 * 2, dtype=torch.float32).reshape(1, 2, 3, 2, 1)  # (B, C, K, h, w)
    cond, mask = S.prepare_sparse_control_conditioning(key, 4, [0])
    assert tuple(cond.shape) == (1, 2, 4, 2, 1) and tuple(mask.shape) == (1, 1, 4, 2, 1)
    assert torch.equal(cond[:, :, 0], key[:, :, 0]) and not cond[:, :, 1:].any()
    assert mask[0, 0, :, 0, 0].tolist() == [1, 0, 0, 0]
    cond, mask = S.prepare_sparse_control_conditioning(key, 4, [0, 3])
    assert torch.equal(cond[:, :, 0], key[:, :, 0]) and torch.equal(cond[:, :, 3], key[:, :, 1])
    assert not cond[:, :, 1:3].any() and mask[0, 0, :, 1, 0].tolist() == [1, 0, 0, 1]
    cond, mask = S.prepare_sparse_control_conditioning(key, 4, [-1])
    assert torch.equal(cond[:, :, 3], key[:, :, 0]) and not cond[:, :, :3].any()
    assert mask[0, 0, :, 0, 0].tolist() == [0, 0, 0, 1]
    cond, mask = S.prepare_sparse_control_conditioning(key, 4, [2, 1, 2])      # duplicates: the last wins
    assert torch.equal(cond[:, :, 2], key[:, :, 2]) and torch.equal(cond[:, :, 1], key[:, :, 1])
    assert mask[0, 0, :, 0, 0].tolist() == [0, 1, 1, 0]
    with pytest.raises(IndexError):
        S.prepare_sparse_control_conditioning(key, 4, [4])


def test_sparse_cond_validates_indices_before_any_library_call(monkeypatch):
    def no_lib():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(ops, "lib", no_lib)
    rows = torch.zeros(8, 8, dtype=torch.bfloat16)
    assert ops.sparse_frame_indices([0, -1, 3, -4], 4) == [0, 3, 3, 0]
    for bad in ([4], [-5], [0, 17]):
        with pytest.raises(IndexError, match="out of bounds for 4 frames"):
            ops.sparse_cond(rows, bad, 1, 4, 4, 4)
    with pytest.raises(TypeError):
        ops.sparse_cond(rows, [0.5], 1, 4, 4, 4)
    with pytest.raises(ValueError, match="condition channels"):
        ops.sparse_cond(rows, [0], 1, 4, 4, 8)
    with pytest.raises(ValueError, match="no CPU fallback"):   # past the index checks: host rows are refused
        ops.sparse_cond(rows, [0, 1], 1, 4, 4, 4)
    assert ops.ROWS_SPARSE_COND == 8 and ops.ROWS_SPARSE_CH_SHIFT == 8


def test_op8_refuses_host_operands_and_a_plain_op():
    """Host memory: nothing is launched.  The documented form with y on the host is refused for y
    alone; a plain op 8 (cc = 0) stays refused as before the op existed."""
    import vdiff._lib as L
    h = L.lib()
    assert h.vd_version() == 6
    buf = torch.zeros(3, 512, dtype=torch.bfloat16)
    px, po, py = buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr()

    def call(op=8 | (4 << 8), x=px, ldx=8, y=py, K=1, y_f32=1, hw=2, F=2, rows=4, C=8, out=po, ldo=8):
        return h.vd_rows_eltwise(op, x, ldx, y, K, y_f32, hw, F, rows, C, out, ldo, None)

    assert call() == 1000
    assert call(op=8) == 1000 and call(op=8 | (8 << 8)) == 1000 and call(op=8 | (4 << 8) | (1 << 16)) == 1000
    assert call(C=16) == 1000 and call(K=0) == 1000 and call(K=257) == 1000 and call(F=0) == 1000
    assert call(F=257, rows=257 * 2) == 1000 and call(hw=0) == 1000 and call(rows=5) == 1000
    assert call(x=None) == 1000 and call(out=None) == 1000 and call(out=px) == 1000 and call(y=None) == 1000
    assert call(ldx=4) == 1000 and call(ldo=4) == 1000 and call(y=py + 2) == 1000 and call(y_f32=0) == 1000


# ---------------------------------------------------------------- refusals of the pipeline
def test_pipeline_refusals_by_name():
    unet, cn = UNetMotionModel("tiny"), SparseControlNetModel("tiny")
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        AnimateDiffSparseControlNetPipeline(unet, [cn, cn])
    with pytest.raises(NotImplementedError, match="frame-sharded"):
        AnimateDiffSparseControlNetPipeline(unet, cn, dist=object())
    with pytest.raises(ValueError, match="SparseControlNetModel"):
        AnimateDiffSparseControlNetPipeline(unet, vdiff.ControlNetModel("tiny"))
    with pytest.raises(ValueError, match="ControlNetModel"):
        vdiff.AnimateDiffControlNetPipeline(unet, cn)
    pipe = AnimateDiffSparseControlNetPipeline(unet, cn)
    ehs = torch.zeros(1, 77, 64)
    kw = dict(prompt_embeds=ehs, negative_prompt_embeds=ehs, num_frames=4, height=64, width=64,
              num_inference_steps=2, output_type="latent")
    frames = torch.rand(1, 3, 64, 64)
    pipe.dist = object()
    with pytest.raises(NotImplementedError, match="frame-sharded"):
        pipe(**kw, conditioning_frames=frames)
    pipe.dist = None
    with pytest.raises(NotImplementedError, match="cfg_shard"):
        pipe(**kw, conditioning_frames=frames, cfg_shard=object())
    pipe.enable_free_init(num_iters=2)
    with pytest.raises(NotImplementedError, match="FreeInit"):
        pipe(**kw, conditioning_frames=frames)
    pipe.disable_free_init()
    pipe._free_noise = (16, 4, "shuffle_context")
    with pytest.raises(NotImplementedError, match="FreeNoise"):
        pipe(**kw, conditioning_frames=frames)
    pipe._free_noise = None
    with pytest.raises(ValueError, match="conditioning_frames required"):
        pipe(**kw)
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        pipe(**kw, conditioning_frames=frames, controlnet_conditioning_scale=[1.0, 0.5])
    with pytest.raises(ValueError, match="motion_max_seq_length"):
        pipe(**dict(kw, num_frames=33), conditioning_frames=frames)
    with pytest.raises(IndexError, match="out of bounds for 4 frames"):
        pipe(**kw, conditioning_frames=frames, controlnet_frame_indices=[4])
    with pytest.raises(ValueError, match="2 controlnet_frame_indices for 1 conditioning frames"):
        pipe(**kw, conditioning_frames=frames, controlnet_frame_indices=[0, 3])
    with pytest.raises(ValueError, match="VAE with its encoder"):   # the simplified embedding needs latents
        pipe(**kw, conditioning_frames=frames)
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        SparseControlConditioning([cn, cn], torch.zeros(4, 8), 1, 1, 2, 2)
    assert pipe._control is None


# ---------------------------------------------------------------- what the restatement must show
@pytest.mark.parametrize("simplified", [True, False])
def test_restatement_ignores_the_latents_and_mixes_frames(simplified):
    c = S.tiny_case()
    v = c[simplified]
    base = v["res_fp32"]
    assert len(base) == 5 and [tuple(r.shape) for r in base] == [(8, 64, 8, 8), (8, 64, 8, 8), (8, 64, 4, 4),
                                                                 (8, 128, 4, 4), (8, 128, 4, 4)]
    with torch.no_grad():
        other = S.sparse_controlnet_forward(v["csd"], v["ccfg"], torch.randn_like(c["x2"]), 961, c["ehs"], v["cond"],
                                            v["mask"])
        keys = v["keys"].clone()
        keys[:, :, 0] = keys[:, :, 0].flip(-1) + 0.25          # the key frame at frame 0 alone
        cond, mask = S.prepare_sparse_control_conditioning(keys, S.NF, S.IDX)
        moved = S.sparse_controlnet_forward(v["csd"], v["ccfg"], c["x2"], 961, c["ehs"], cond, mask)
    for i, (a, b, m) in enumerate(zip(base, other, moved)):
        assert torch.equal(a, b), i                                # no residual reads the latents
        last = [S.NF - 1, 2 * S.NF - 1]                            # the last frame of either video
        assert torch.equal(cond[:, :, S.NF - 1], v["cond"][:, :, S.NF - 1])
        # residual 0 is the embedding's own zero conv, per frame; every later one sits behind a
        # motion module: frame 0's condition reached frame 3
        assert torch.equal(a[last], m[last]) == (i == 0), i
    assert not torch.equal(base[0][0], moved[0][0])


def test_restatement_reads_the_condition_through_the_embedding_alone():
    c = S.tiny_case()
    v = c[True]
    sd = dict(v["csd"])
    for k in ("controlnet_cond_embedding.weight", "controlnet_cond_embedding.bias"):
        sd[k] = torch.zeros_like(sd[k])
    with torch.no_grad():
        a = S.sparse_controlnet_forward(sd, v["ccfg"], c["x2"], 961, c["ehs"], v["cond"], v["mask"])
        b = S.sparse_controlnet_forward(sd, v["ccfg"], c["x2"], 961, c["ehs"], torch.randn_like(v["cond"]),
                                        1 - v["mask"])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], v["res_fp32"][0])
