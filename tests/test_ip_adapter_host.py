"""IP-Adapter, the CPU side: the argument checks of VD_ATTN_TAIL (they return before any launch,
so they run without a GPU as tests/test_clip_host.py's do) and the conditioning of the inputs the
GPU parity tests use — the image segment must matter far more than any GPU bar allows.
"""
import ctypes as C

import pytest
import torch

import ip_adapter_ref as ref
import vdiff._lib

EINVAL, EUNSUPPORTED = 1000, 1001


def _attention_ex(sq, skv, d, kv_div, kernel, batch=2, scale=0.125):
    L = vdiff._lib.lib()
    p = 256  # aligned dummy operands: the argument checks read sizes and alignments only and launch nothing
    return L.vd_attention_ex(p, 320, p, 320, p, 320, p, 320, batch, 2, sq, skv, d, kv_div, C.c_float(scale), 0, kernel,
                             None)


def tail(n):
    return n << 16


def test_tail_flag_encoding():
    from vdiff import ops
    assert ops.ATTN_TAIL_SHIFT == 16
    hdr = (vdiff._lib.LIB_PATH.parents[2] / "include" / "vdiff.h").read_text()
    assert "VD_ATTN_TAIL_SHIFT = 16" in hdr and "VD_ATTN_TAIL_MASK = 0x7f0000" in hdr
    assert vdiff._lib.lib().vd_version() == 6


def test_tail_flag_argument_checks():
    assert _attention_ex(64, 81, 64, 1, tail(81)) == EINVAL           # n >= skv (and n > 64)
    assert _attention_ex(64, 4, 64, 1, tail(4)) == EINVAL             # n == skv: no text segment left
    assert _attention_ex(64, 3, 64, 1, tail(4)) == EINVAL             # n > skv
    assert _attention_ex(81, 81, 64, 1, tail(4) | 0x100) == EINVAL    # a tail with VD_ATTN_CAUSAL
    assert _attention_ex(64, 200, 64, 1, tail(65)) == EINVAL          # n = 65: one key tile holds 64
    assert _attention_ex(64, 200, 64, 1, tail(127)) == EINVAL
    assert _attention_ex(64, 81, 64, 1, tail(4), scale=0.0) == EINVAL  # scale <= 0
    assert _attention_ex(64, 81, 64, 1, tail(4), scale=-0.125) == EINVAL
    assert _attention_ex(64, 81, 64, 1, tail(4) | 4) == EINVAL        # kernel code above 3 under the flag
    assert _attention_ex(64, 81, 128, 1, tail(4)) == EUNSUPPORTED     # d = 128: no tailed instance
    assert _attention_ex(64, 81, 512, 1, tail(4)) == EUNSUPPORTED
    assert _attention_ex(64, 81, 48, 1, tail(4)) == EUNSUPPORTED
    assert _attention_ex(77, 77, 64, 1, 0x200) == EINVAL              # the bit below the tail field: still unknown
    assert _attention_ex(77, 77, 64, 1, 0x800000) == EINVAL           # ... and the bit above it
    assert _attention_ex(77, 77, 64, 1, 0x8000) == EINVAL


def test_ops_attention_refuses_a_tail_outside_the_field():
    from vdiff import ops
    t = torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="tail"):
        ops.attention(t, t, t, 1, 1, 8, 8, 64, tail=128)
    with pytest.raises(ValueError, match="tail"):
        ops.attention(t, t, t, 1, 1, 8, 8, 64, tail=-1)


def test_kernel_inputs_are_sensitive_to_the_tail():
    """On the inputs of the GPU kernel test the two-softmax result differs from the text-only
    attention by rel-L2 >= 0.2; every GPU bar stays <= 0.1, so no tolerance can hide a missing
    tail (or one folded into the text's softmax)."""
    import test_gpu_ip_adapter as T
    for d, main, n, sq, kv_div, _ in T.KERNEL_CASES:
        q, k, v = T.make_inputs(d, main, n, sq, kv_div)
        want = ref.two_softmax_attention(q, k, v, T.HEADS, n, kv_div)
        text = ref.sdpa(q.double(), k[:, :main].double().repeat_interleave(kv_div, 0),
                        v[:, :main].double().repeat_interleave(kv_div, 0), T.HEADS)
        one = ref.sdpa(q.double(), k.double().repeat_interleave(kv_div, 0), v.double().repeat_interleave(kv_div, 0),
                       T.HEADS)
        assert T.rel_l2(text, want) >= 0.2, (d, main, n, sq)
        if main > 1:  # the single softmax over all skv keys is a different function too
            assert T.rel_l2(one, want) >= 0.2, (d, main, n, sq)
    assert T.TAIL_M * 0.02 <= 0.1  # the kernel bar's ceiling (the composition's own error is asserted < 0.02)


# ---------------------------------------------------------------- vision tower / preprocessing restatements
VISION_CONFIGS = ref.VISION_TINY


@pytest.mark.parametrize("name", sorted(VISION_CONFIGS))
def test_vision_restatement_equals_transformers(name):
    tr = pytest.importorskip("transformers")
    cfg = VISION_CONFIGS[name]
    torch.manual_seed(3)
    m = tr.CLIPVisionModelWithProjection(tr.CLIPVisionConfig(**cfg)).eval()
    px = torch.randn(2, 3, cfg["image_size"], cfg["image_size"])
    with torch.no_grad():
        o = m(pixel_values=px, output_hidden_states=True)
        e, last, hs = ref.vision_tower(m.state_dict(), cfg, px)
    assert (e - o.image_embeds).abs().max() < 1e-5
    assert (last - o.last_hidden_state).abs().max() < 1e-5
    assert len(hs) == len(o.hidden_states)
    for a, b in zip(hs, o.hidden_states):
        assert (a - b).abs().max() < 1e-5


def test_vision_model_keys_are_transformers_own():
    tr = pytest.importorskip("transformers")
    import vdiff
    for cfg in VISION_CONFIGS.values():
        want = {k: tuple(v.shape) for k, v in tr.CLIPVisionModelWithProjection(tr.CLIPVisionConfig(**cfg)).state_dict().items()
                if not k.endswith("position_ids")}
        got = {k: tuple(v.shape) for k, v in vdiff.CLIPVisionModelWithProjection(cfg).state_dict().items()}
        assert got == want


def _images():
    import numpy as np
    from PIL import Image
    rs = np.random.RandomState(7)
    return [Image.fromarray((rs.rand(h, w, 3) * 255).astype(np.uint8)) for (w, h) in ((37, 61), (300, 224))]


def test_preprocessing_equals_transformers():
    """Compared with transformers' own CLIPImageProcessor (without torchvision it resolves to its
    PIL backend, which is the class this was checked against) and with the PIL formulas."""
    import numpy as np
    import vdiff
    proc = vdiff.CLIPImageProcessor()
    try:
        from transformers import CLIPImageProcessor as TrProc
        theirs = TrProc()
    except Exception:  # not importable here: the PIL formulas below are the comparison
        theirs = None
    for im in _images():
        ours = proc(im).pixel_values
        assert ours.shape == (1, 3, 224, 224) and ours.dtype == torch.float32
        assert (ours[0].double() - ref.preprocess(im)).abs().max() < 1e-5
        if theirs is not None:
            t = torch.from_numpy(np.asarray(theirs(im)["pixel_values"][0]))
            assert (ours[0] - t).abs().max() < 1e-5
    # arrays and tensors go the same way as the PIL image they hold
    im = _images()[0]
    a = np.array(im)
    for other in (a, torch.from_numpy(a), torch.from_numpy(a).permute(2, 0, 1), a.astype(np.float32) / 255):
        assert torch.equal(proc(other).pixel_values, proc(im).pixel_values)
    assert proc([im, im]).pixel_values.shape == (2, 3, 224, 224)


# ---------------------------------------------------------------- loader
def _tiny_unet():
    from vdiff import UNetMotionModel, init_synthetic_
    return init_synthetic_(UNetMotionModel("tiny"), seed=0)


def synthetic_adapter(unet, n=4, clip_dim=48, seed=0, scale=1.0):
    """A plain IP-Adapter state dict (flat keys, as a .safetensors file holds them) for `unet`."""
    g = torch.Generator().manual_seed(seed)
    cross = unet.config["cross_attention_dim"]
    sd = {"image_proj.proj.weight": torch.randn(n * cross, clip_dim, generator=g) * clip_dim ** -0.5,
          "image_proj.proj.bias": torch.randn(n * cross, generator=g) * 0.1,
          "image_proj.norm.weight": 1 + 0.1 * torch.randn(cross, generator=g),
          "image_proj.norm.bias": 0.1 * torch.randn(cross, generator=g)}
    for i, a in enumerate(unet.spatial_cross_attentions()):
        inner = a.heads * a.dim_head
        for kv in "kv":
            sd[f"ip_adapter.{2 * i + 1}.to_{kv}_ip.weight"] = torch.randn(inner, cross, generator=g) * scale * cross ** -0.5
    return sd


def test_key_id_table_and_block_order():
    from vdiff import pretrained as P
    assert P.IP_ADAPTER_BLOCK_ORDER == ("down_blocks", "up_blocks", "mid_block")
    assert P.ip_adapter_key_ids(16) == list(range(1, 32, 2))
    unet = _tiny_unet()
    attns = unet.spatial_cross_attentions()
    names = {id(m): n for n, m in unet.named_modules()}
    order = [names[id(a)] for a in attns]
    assert all(".attn2" in n and "motion_modules" not in n for n in order)
    top = [n.split(".")[0] for n in order]
    assert top == sorted(top, key=P.IP_ADAPTER_BLOCK_ORDER.index) and top[-1] == "mid_block"
    assert len(attns) == sum(1 for n, _ in unet.named_modules() if n.endswith(".attn2") and "motion_modules" not in n)
    # the full config has the 16 cross-attentions the ids 1..31 number
    with torch.device("meta"):
        from vdiff import UNetMotionModel
        assert len(UNetMotionModel("full").spatial_cross_attentions()) == 16


def test_loader_reads_both_layouts_and_takes_the_token_count_from_the_shapes(tmp_path):
    from safetensors.torch import save_file
    from vdiff import ImageProjection
    from vdiff import pretrained as P
    unet = _tiny_unet()
    cross = unet.config["cross_attention_dim"]
    for n in (4, 16):
        sd = synthetic_adapter(unet, n=n)
        save_file(sd, str(tmp_path / "a.safetensors"))
        nested = {"image_proj": {k[len("image_proj."):]: v for k, v in sd.items() if k.startswith("image_proj.")},
                  "ip_adapter": {k[len("ip_adapter."):]: v for k, v in sd.items() if k.startswith("ip_adapter.")}}
        torch.save(nested, str(tmp_path / "a.bin"))
        for wn in ("a.safetensors", "a.bin"):
            proj, ip = P.read_ip_adapter(tmp_path, weight_name=wn)
            P.check_ip_adapter_variant(proj, ip)
            kv = P.ip_adapter_kv_weights(ip, len(unet.spatial_cross_attentions()))
            assert torch.equal(kv[1][0], sd["ip_adapter.3.to_k_ip.weight"]) and torch.equal(kv[1][1], sd["ip_adapter.3.to_v_ip.weight"])
            m = ImageProjection.from_state_dict(proj, cross)
            assert m.num_image_text_embeds == n and m.proj.in_features == 48
    with pytest.raises(FileNotFoundError):
        P.read_ip_adapter(tmp_path, weight_name="missing.safetensors")
    with pytest.raises(KeyError, match="do not fit"):
        P.ip_adapter_kv_weights(ip, 3)


def test_loader_refuses_the_other_variants():
    from vdiff import AnimateDiffPipeline, DDIMScheduler
    unet = _tiny_unet()
    pipe = AnimateDiffPipeline(unet, DDIMScheduler())
    base = synthetic_adapter(unet)
    plus = dict(base, **{"image_proj.latents": torch.zeros(1, 16, 8)})
    face = {k: v for k, v in base.items() if not k.startswith("image_proj.proj")}
    face["image_proj.proj.0.weight"] = torch.zeros(8, 8)
    lora = dict(base, **{"ip_adapter.1.to_k_lora.down.weight": torch.zeros(4, 8)})
    for sd, word in ((plus, "Plus"), (face, "FaceID"), (lora, "FaceID")):
        with pytest.raises(NotImplementedError, match=word):
            pipe.load_ip_adapter(sd)
    with pytest.raises(NotImplementedError, match="list"):
        pipe.load_ip_adapter([base, base])
    with pytest.raises(NotImplementedError, match="list"):
        pipe.load_ip_adapter("somewhere", weight_name=["a.safetensors", "b.safetensors"])
    assert not unet.has_ip_adapter and pipe.image_projection is None
    pipe.load_ip_adapter(base)
    with pytest.raises(NotImplementedError, match="per-block"):
        pipe.set_ip_adapter_scale({"down": {"block_2": [0.0, 1.0]}})


def test_unload_restores_the_exact_state_dict_key_set():
    from vdiff import AnimateDiffPipeline, DDIMScheduler
    unet = _tiny_unet()
    before = {k: v.clone() for k, v in unet.state_dict().items()}
    params = sum(p.numel() for p in unet.parameters())
    pipe = AnimateDiffPipeline(unet, DDIMScheduler())
    with pytest.raises(ValueError, match="no IP-Adapter"):
        pipe.set_ip_adapter_scale(0.5)
    pipe.load_ip_adapter(synthetic_adapter(unet))
    extra = set(unet.state_dict()) - set(before)
    assert len(extra) == 2 * len(unet.spatial_cross_attentions())
    assert all(k.endswith(("attn2.to_k_ip.weight", "attn2.to_v_ip.weight")) and "motion_modules" not in k for k in extra)
    assert pipe.image_projection.num_image_text_embeds == 4
    pipe.set_ip_adapter_scale(0.5)
    assert all(a.ip_scale == 0.5 for a in unet.spatial_cross_attentions())
    pipe.unload_ip_adapter()
    after = unet.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert sum(p.numel() for p in unet.parameters()) == params
    assert all(a.ip_scale == 1.0 and not hasattr(a, "_wkv_ip") for a in unet.spatial_cross_attentions())
    assert pipe.image_projection is None and pipe.image_encoder is None


def test_image_arguments_need_a_loaded_adapter():
    from vdiff import AnimateDiffPipeline, DDIMScheduler
    pipe = AnimateDiffPipeline(_tiny_unet(), DDIMScheduler())
    for kw in (dict(ip_adapter_image=_images()[0]), dict(ip_adapter_image_embeds=torch.zeros(1, 1, 48))):
        with pytest.raises(ValueError, match="no IP-Adapter"):
            pipe.prepare_ip_adapter_image_embeds(kw.get("ip_adapter_image"), kw.get("ip_adapter_image_embeds"), 1, 1, True)


def test_module_path_refuses_the_tuple_form():
    from vdiff.models.layers import Attention
    a = Attention(64, 2, 32, cross_attention_dim=64)
    x = torch.zeros(1, 4, 64)
    with pytest.raises(NotImplementedError, match="text-only"):
        a(x, encoder_hidden_states=(x, [x]))


def test_block_and_vision_fixtures_are_sensitive():
    """The preconditions of the GPU parity bars (all <= 0.1): on the block inputs the restatement
    with the adapter differs from the one without by rel-L2 >= 0.2 (so a block that ignores the
    image tokens cannot pass), and the vision fixtures move by >= 0.2 when the attention is masked
    causally (so the tower's attention matters to what the golden file pins)."""
    import numpy as np
    import test_gpu_ip_adapter as T
    for case, (dim, heads, dh, cross, hw, frames, L, n) in ref.BLOCK_CASES.items():
        sd, h_half, ehs, ip = ref.block_inputs(case)
        h = torch.cat([h_half, h_half]).double()
        e, i = ehs.double().repeat_interleave(frames, 0), ip.double().repeat_interleave(frames, 0)
        with_ip, without = ref.transformer_block(sd, h, e, i, heads), ref.transformer_block(sd, h, e, None, heads)
        assert T.rel_l2(without, with_ip) >= 0.2, case
        assert T.rel_l2(ref.transformer_block(sd, h, e, i, heads, 0.0), without) < 1e-12
    gold = np.load(T.Path(T.__file__).parent / "golden" / "ip_adapter_vision.npz")
    for name, cfg in ref.VISION_TINY.items():
        sd, px = ref.vision_synthetic_state_dict(cfg, 0), ref.vision_fixture_pixels(cfg)
        assert torch.equal(px, torch.from_numpy(gold[f"{name}.pixel_values"]))
        e, last, _ = ref.vision_tower(sd, cfg, px.double())
        assert T.rel_l2(e, torch.from_numpy(gold[f"{name}.image_embeds"])) < 1e-5
        assert T.rel_l2(last, torch.from_numpy(gold[f"{name}.last_hidden_state"])) < 1e-5
        ec, _, _ = ref.vision_tower(sd, cfg, px.double(), causal=True)
        assert T.rel_l2(ec, e) >= 0.2
    assert T.BAR_CEILING <= 0.1
