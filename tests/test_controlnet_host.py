"""ControlNet on the host: the module tree against the published SD-1.5 ControlNet size and
diffusers' key names, the scale table against diffusers' rule written by hand, the refusals, the
entry point's VD_EINVAL cases (host pointers: nothing is launched), loading from a local folder,
and the precondition the GPU tests rest on — with the tests' random weights no residual is
negligible (tests/controlnet_ref.py)."""
import json

import pytest
import torch

import controlnet_ref as R
import vdiff
import vdiff._lib as L
from vdiff import AnimateDiffControlNetPipeline, ControlNetConditioning, ControlNetModel, UNetMotionModel, ops
from vdiff.models.controlnet import (control_scale_table, controlnet_config, controlnet_config_from_diffusers,
                                     guess_mode_scales)


# ---------------------------------------------------------------- the tree
def test_full_parameter_count_and_diffusers_names():
    with torch.device("meta"):
        m = ControlNetModel("full")
    n = {k: sum(p.numel() for kk, p in m.named_parameters() if kk.startswith(k))
         for k in ("controlnet_cond_embedding.", "controlnet_down_blocks.", "controlnet_mid_block.")}
    zero = n["controlnet_down_blocks."] + n["controlnet_mid_block."]
    total = sum(p.numel() for p in m.parameters())
    assert n["controlnet_cond_embedding."] == 1_086_480
    assert zero == 11_479_680
    assert total - zero - n["controlnet_cond_embedding."] == 348_712_960
    assert total == 361_279_120  # the published size of the SD-1.5 ControlNets
    keys = set(m.state_dict())
    assert not any("motion_modules" in k for k in keys)
    for k in ("conv_in.weight", "time_embedding.linear_2.bias", "controlnet_cond_embedding.conv_in.weight",
              "controlnet_cond_embedding.blocks.5.bias", "controlnet_cond_embedding.conv_out.weight",
              "down_blocks.0.attentions.1.transformer_blocks.0.attn2.to_k.weight",
              "down_blocks.2.downsamplers.0.conv.weight", "down_blocks.3.resnets.1.conv2.bias",
              "mid_block.attentions.0.proj_out.weight", "mid_block.resnets.1.time_emb_proj.weight",
              "controlnet_down_blocks.0.weight", "controlnet_down_blocks.11.bias", "controlnet_mid_block.weight"):
        assert k in keys, k
    assert "controlnet_down_blocks.12.weight" not in keys and "down_blocks.3.downsamplers.0.conv.weight" not in keys
    sd = m.state_dict()
    emb = [tuple(sd[f"controlnet_cond_embedding.blocks.{i}.weight"].shape[:2]) for i in range(6)]
    assert emb == [(16, 16), (32, 16), (32, 32), (96, 32), (96, 96), (256, 96)]
    assert tuple(sd["controlnet_cond_embedding.conv_in.weight"].shape) == (16, 3, 3, 3)
    assert tuple(sd["controlnet_cond_embedding.conv_out.weight"].shape) == (320, 256, 3, 3)
    assert [m.controlnet_cond_embedding.blocks[i].stride[0] for i in range(6)] == [1, 2, 1, 2, 1, 2]
    assert m.residual_channels() == [320] * 4 + [640] * 3 + [1280] * 6 and m.num_residuals == 13
    assert tuple(sd["controlnet_down_blocks.4.weight"].shape) == (640, 640, 1, 1)


def test_tiny_config_matches_the_tiny_unet():
    cn = ControlNetModel("tiny")
    unet = UNetMotionModel("tiny")
    assert cn.config["conditioning_embedding_out_channels"] == (16, 32, 32, 64)
    assert cn.num_residuals == 5
    assert cn.residual_channels() == [c for _, c in unet.control_residual_shapes(1, 8, 8)]
    assert unet.control_residual_shapes(4, 8, 8) == [(256, 64), (256, 64), (64, 64), (64, 128), (64, 128)]
    assert controlnet_config("full")["block_out_channels"] == vdiff.FULL["block_out_channels"]
    assert "up_block_types" not in cn.config and "motion_max_seq_length" not in cn.config


# ---------------------------------------------------------------- the scale table
def diffusers_keep(n, start, end):
    """AnimateDiffControlNetPipeline.__call__: controlnet_keep, one ControlNet."""
    keep = []
    for i in range(n):
        keeps = [1.0 - float(i / n < s or (i + 1) / n > e) for s, e in zip([start], [end])]
        keep.append(keeps[0])
    return keep


@pytest.mark.parametrize("guess", [False, True])
@pytest.mark.parametrize("window", [(0.0, 1.0), (0.0, 0.5), (0.4, 1.0), (0.0, 0.0)])
def test_scale_table_follows_diffusers(window, guess):
    start, end = window
    for n, n_res, scale in ((1, 13, 1.0), (3, 5, 1.0), (4, 13, 0.7), (10, 13, 1.5), (25, 13, 1.0)):
        got = control_scale_table(n, n_res, scale, guess, start, end)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, n_res)
        keep = diffusers_keep(n, start, end)
        for i in range(n):
            cond_scale = scale * keep[i]                       # diffusers: controlnet_cond_scale * controlnet_keep[i]
            if guess:                                          # ControlNetModel.forward: scales = logspace * scale
                want = torch.logspace(-1, 0, n_res) * cond_scale
            else:
                want = torch.full((n_res,), cond_scale)
            assert torch.equal(got[i], want.float()), (n, i)
        assert torch.equal(got, R.scale_table(n, n_res, scale, guess, start, end))
    if window == (0.0, 0.0):
        assert not control_scale_table(7, 13, 1.0, guess, 0.0, 0.0).any()
    if window == (0.0, 0.5):
        t = control_scale_table(3, 5, 1.0, False, 0.0, 0.5)
        assert t[:, 0].tolist() == [1.0, 0.0, 0.0]             # the GPU tests' run: the scale changes between replays
    assert guess_mode_scales(13)[0] == pytest.approx(0.1) and guess_mode_scales(13)[-1] == 1.0


def test_scale_table_refuses_bad_windows():
    with pytest.raises(ValueError, match="larger or equal"):
        control_scale_table(4, 13, 1.0, False, 0.5, 0.5)
    with pytest.raises(ValueError, match="outside"):
        control_scale_table(4, 13, 1.0, False, 0.0, 1.5)
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        control_scale_table(4, 13, [1.0, 0.5])


# ---------------------------------------------------------------- refusals
def test_config_flags_outside_the_tree_are_refused():
    base = dict(block_out_channels=[320, 640, 1280, 1280], down_block_types=["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"],
                attention_head_dim=8, cross_attention_dim=768, layers_per_block=2,
                conditioning_embedding_out_channels=[16, 32, 96, 256])
    cfg = controlnet_config_from_diffusers(base)
    assert cfg["num_attention_heads"] == 8 and cfg["conditioning_embedding_out_channels"] == (16, 32, 96, 256)
    for extra, match in ((dict(use_linear_projection=True), "use_linear_projection"),
                         (dict(class_embed_type="timestep"), "class / addition"),
                         (dict(num_class_embeds=10), "class / addition"),
                         (dict(addition_embed_type="text_time"), "class / addition"),
                         (dict(global_pool_conditions=True), "global_pool_conditions"),
                         (dict(controlnet_conditioning_channel_order="bgr"), "channel_order")):
        with pytest.raises(NotImplementedError, match=match):
            controlnet_config_from_diffusers(dict(base, **extra))


def test_multi_controlnet_and_sharding_are_refused():
    unet, cn = UNetMotionModel("tiny"), ControlNetModel("tiny")
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        AnimateDiffControlNetPipeline(unet, [cn, cn])
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        ControlNetModel.from_pretrained(["a", "b"])
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        ControlNetConditioning([cn, cn], None)
    with pytest.raises(NotImplementedError, match="frame-sharded"):
        AnimateDiffControlNetPipeline(unet, cn, dist=object())
    with pytest.raises(ValueError, match="ControlNetModel"):
        AnimateDiffControlNetPipeline(unet, unet)
    pipe = AnimateDiffControlNetPipeline(unet, cn)
    ehs = torch.zeros(1, 77, 64)
    kw = dict(prompt_embeds=ehs, negative_prompt_embeds=ehs, num_frames=2, height=64, width=64,
              num_inference_steps=2, output_type="latent")
    frames = torch.rand(2, 3, 64, 64)
    pipe.dist = object()
    with pytest.raises(NotImplementedError, match="frame-sharded"):
        pipe(**kw, conditioning_frames=frames)
    pipe.dist = None
    pipe.enable_free_init(num_iters=2)
    with pytest.raises(NotImplementedError, match="FreeInit"):
        pipe(**kw, conditioning_frames=frames)
    pipe.disable_free_init()
    with pytest.raises(ValueError, match="conditioning_frames required"):
        pipe(**kw)
    with pytest.raises(ValueError, match="3 conditioning frames for num_frames=2"):
        pipe(**kw, conditioning_frames=torch.rand(3, 3, 64, 64))
    with pytest.raises(ValueError, match="asked for 64 x 64"):
        pipe(**kw, conditioning_frames=torch.rand(2, 3, 32, 64))
    with pytest.raises(NotImplementedError, match="MultiControlNet"):
        pipe(**kw, conditioning_frames=frames, controlnet_conditioning_scale=[1.0, 0.5])
    with pytest.raises(ValueError, match="larger or equal"):
        pipe(**kw, conditioning_frames=frames, control_guidance_start=0.6, control_guidance_end=0.2)
    assert pipe._control is None


def test_unet_refuses_a_wrong_count_or_shape():
    unet = UNetMotionModel("tiny")
    shapes = unet.control_residual_shapes(4, 8, 8)
    maps = [torch.zeros(4, c, 8 if r == 256 else 4, 8 if r == 256 else 4) for r, c in shapes]
    with pytest.raises(ValueError, match="go together"):
        unet._control_residuals(maps[:-1], None, 4, 8, 8)
    with pytest.raises(ValueError, match="3 down-block residuals for this UNet's 4 skips"):
        unet._control_residuals(maps[:3], maps[-1], 4, 8, 8)
    bad = list(maps)
    bad[2] = torch.zeros(4, 64, 8, 8)
    with pytest.raises(ValueError, match="control residual 2 of shape"):
        unet._control_residuals(bad[:-1], bad[-1], 4, 8, 8)
    bad = list(maps)
    bad[4] = torch.zeros(4, 64, 4, 4)
    with pytest.raises(ValueError, match="control residual 4 of shape"):
        unet._control_residuals(bad[:-1], bad[-1], 4, 8, 8)
    with pytest.raises(ValueError, match="no CPU fallback"):  # past the checks: the rows must be on the GPU
        unet._control_residuals(maps[:-1], maps[-1], 4, 8, 8)
    assert unet._control_residuals(None, None, 4, 8, 8) is None


# ---------------------------------------------------------------- loading
def test_from_pretrained_local_folder_round_trip(tmp_path):
    from safetensors.torch import save_file
    src = R.random_controlnet("tiny", seed=3)
    cfg = dict(_class_name="ControlNetModel", in_channels=4, block_out_channels=[64, 128], layers_per_block=1,
               down_block_types=["CrossAttnDownBlock2D", "DownBlock2D"], attention_head_dim=2, cross_attention_dim=64,
               norm_num_groups=32, conditioning_embedding_out_channels=[16, 32, 32, 64], use_linear_projection=False,
               class_embed_type=None, global_pool_conditions=False, controlnet_conditioning_channel_order="rgb")
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    save_file({k: v.contiguous() for k, v in src.state_dict().items()},
              str(tmp_path / "diffusion_pytorch_model.safetensors"))
    got = ControlNetModel.from_pretrained(tmp_path, device="cpu", torch_dtype=torch.float16)
    assert got.dtype == torch.bfloat16 and got.torch_dtype == torch.float16
    want = src.state_dict()
    assert set(got.state_dict()) == set(want)
    for k, v in got.state_dict().items():
        assert torch.equal(v.float(), want[k].float()), k  # the synthetic weights are bf16 values
    (tmp_path / "config.json").write_text(json.dumps(dict(cfg, use_linear_projection=True)))
    with pytest.raises(NotImplementedError, match="use_linear_projection"):
        ControlNetModel.from_pretrained(tmp_path, device="cpu")
    with pytest.raises(FileNotFoundError, match="not a local directory"):
        ControlNetModel.from_pretrained("lllyasviel/control_v11f1p_sd15_depth")
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        got.prepare()


# ---------------------------------------------------------------- the entry point
def test_op7_refuses_before_launch():
    """Each call differs from the documented form (op 7 | column 1 of a 3-column, 2-row table over
    4 rows of 8 columns) in the one argument named; all return VD_EINVAL (1000) and nothing is
    launched: the operands are host memory, which the entry point refuses for y on its own."""
    h = L.lib()
    assert ops.ROWS_CTRL_ADD == 7 and ops.ROWS_CTRL_COL_SHIFT == 8 and ops.CTRL_HEADER == 4
    assert h.vd_version() == 6
    buf = torch.zeros(3, 512, dtype=torch.bfloat16)  # host memory: never dereferenced
    px, po, py = buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr()
    assert px % 16 == 0 and po % 16 == 0 and py % 16 == 0

    def call(op=7 | (1 << 8), x=px, ldx=8, y=py, ldy=3, y_f32=1, period=2, rows=4, C=8, out=po, ldo=8):
        return h.vd_rows_eltwise(op, x, ldx, y, ldy, y_f32, 1, period, rows, C, out, ldo, None)

    assert call() == 1000                                    # y is host memory
    assert call(x=None) == 1000 and call(y=None) == 1000 and call(out=None) == 1000
    assert call(x=px + 2) == 1000 and call(y=py + 4) == 1000 and call(out=po + 8) == 1000  # not 16-byte aligned
    assert call(y_f32=0) == 1000 and call(y_f32=2) == 1000
    assert call(ldy=0) == 1000 and call(ldy=65) == 1000 and call(ldy=-1) == 1000
    assert call(op=7 | (3 << 8)) == 1000 and call(op=7 | (64 << 8), ldy=64) == 1000     # i >= ldy
    assert call(op=7 | (1 << 8) | (1 << 16)) == 1000 and call(op=7 | (1 << 8) | (1 << 30)) == 1000
    assert call(op=-(1 << 31) | 7) == 1000                  # the sign bit
    assert call(period=0) == 1000 and call(period=-3) == 1000
    assert call(C=12) == 1000 and call(C=0) == 1000 and call(rows=0) == 1000
    assert call(out=px) == 1000                              # x == out
    assert call(ldx=4) == 1000 and call(ldo=4) == 1000 and call(ldo=12) == 1000
    for op in range(6):                                      # no other op carries a column
        assert h.vd_rows_eltwise(op | (1 << 8), px, 8, py, 8, 1, 2, 2, 4, 8, po, 8, None) == 1000
    assert h.vd_rows_eltwise(8, px, 8, py, 8, 1, 2, 2, 4, 8, po, 8, None) == 1000


def test_wrappers_refuse_host_tensors_and_bad_tables():
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.ctrl_block(torch.ones(3, 5))
    with pytest.raises(ValueError, match="table"):
        ops.ctrl_block(torch.ones(3, 65), device="cuda")
    with pytest.raises(ValueError, match="table"):
        ops.ctrl_block(torch.ones(5), device="cuda")
    a = torch.zeros(4, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.ctrl_add_(a, a.clone(), torch.zeros(9), 0, cols=5)


# ---------------------------------------------------------------- the precondition of the GPU tests
def test_random_weights_make_every_residual_matter():
    """The zero convs are not zero; in the fp32 restatement every residual (scale 1) has norm >=
    0.1 x its skip's; dropping one residual, or swapping two of equal shape, moves the UNet output
    by more than 3 x the bar of the UNet-with-residuals checks."""
    c = R.tiny_case()
    for z in [*c["cnet"].controlnet_down_blocks, c["cnet"].controlnet_mid_block]:
        assert z.weight.abs().max() > 0
    assert len(c["res_fp32"]) == len(c["skips_fp32"]) == 5
    for i, (r, s) in enumerate(zip(c["res_fp32"], c["skips_fp32"])):
        assert tuple(r.shape) == tuple(s.shape)
        ratio = (r.norm() / s.norm()).item()
        print(f"residual {i} {tuple(r.shape)}: |res| / |skip| = {ratio:.3f}")
        assert ratio >= 0.1, (i, ratio)
    bar = c["unet_bar_modules"]  # the larger of the two bars
    assert bar >= c["unet_bar"]
    print(f"bf16-emulating restatement vs fp32: fast path {c['unet_emulated']:.5f}, module path "
          f"{c['unet_emulated_modules']:.5f}; bars {c['unet_bar']:.5f} / {bar:.5f}")

    def run(res):
        with torch.no_grad():
            return R.unet_forward_residuals(c["usd"], c["cfg"], c["x2"], c["t"], c["ehs"], res, "fp32")

    for i in range(5):
        res = [r.clone() for r in c["given"]]
        res[i].zero_()
        d = R.rel_l2(run(res), c["out_fp32"])
        print(f"dropping residual {i} moves the output by {d:.4f}")
        assert d > 3 * bar, (i, d)
    pairs = [(a, b) for a in range(5) for b in range(a + 1, 5) if c["given"][a].shape == c["given"][b].shape]
    assert pairs == [(0, 1), (3, 4)]
    for a, b in pairs:
        res = list(c["given"])
        res[a], res[b] = res[b], res[a]
        d = R.rel_l2(run(res), c["out_fp32"])
        print(f"swapping residuals {a} and {b} moves the output by {d:.4f}")
        assert d > 3 * bar, (a, b, d)
    assert R.rel_l2(c["out_plain"], c["out_fp32"]) > 3 * bar   # and so does ignoring them all
