"""Perturbed-attention guidance without a GPU: the layer-matching rule, the per-step scale table,
the pipeline's switches, the entry points' flag word (every call returns before a launch), the
host wrappers' checks, and tests/pag_ref.py itself — at scale 0 its loop is the existing DDIM
reference loop bit for bit, identity attention moves the perturbed eps, and the shared block
case separates perturbed from unperturbed output by more than 10 x the device tests' bar.
"""
import ctypes

import pytest
import torch

import controlnet_ref as C
import pag_ref as R
import vdiff._lib as L
from oracle import ddim_ref
from vdiff import AnimateDiffPAGPipeline, DDIMScheduler, PerturbedAttentionGuidance, UNetMotionModel, ops
from vdiff.models.unet_motion import pag_layer_matches, pag_select

MID_SPATIAL = "mid_block.attentions.0.transformer_blocks.0.attn1"
MID_MOTION1 = "mid_block.motion_modules.0.transformer_blocks.0.attn1"
MID_MOTION2 = "mid_block.motion_modules.0.transformer_blocks.0.attn2"


@pytest.fixture(scope="module")
def unet():
    return UNetMotionModel("tiny")


# ---------------------------------------------------------------- 1. layer matching
def test_self_attention_names_of_the_tiny_unet(unet):
    names = unet.self_attention_names()
    assert len(names) == 18
    assert sorted(names) == R.self_attention_names(unet.state_dict())
    # a spatial block's attn2 reads the text: never a candidate; a motion block's attn2 is one
    assert not any(".attentions." in n and n.endswith("attn2") for n in names)
    assert MID_MOTION2 in names and "down_blocks.0.attentions.0.transformer_blocks.0.attn1" in names


def test_default_layers_select_both_mid_block_attn1(unet):
    names = unet.self_attention_names()
    assert pag_select("mid_block.*attn1", names) == [MID_SPATIAL, MID_MOTION1]
    assert R.select_layers("mid_block.*attn1", names) == [MID_SPATIAL, MID_MOTION1]
    # a bare "mid_block" also takes the motion module's attn2
    assert pag_select("mid_block", names) == [MID_SPATIAL, MID_MOTION1, MID_MOTION2]
    assert pag_select(["mid_block"], names) == R.select_layers(["mid_block"], names)


def test_a_layer_id_ending_in_digits_is_not_followed_by_a_digit(unet):
    ten = "down_blocks.10.attentions.0.transformer_blocks.0.attn1"
    one = "down_blocks.1.motion_modules.0.transformer_blocks.0.attn1"
    assert pag_layer_matches("down_blocks.1", one) and not pag_layer_matches("down_blocks.1", ten)
    assert pag_layer_matches("down_blocks.10", ten) and pag_layer_matches("down_blocks", ten)
    assert pag_select("down_blocks.1", [one, ten]) == [one] == R.select_layers("down_blocks.1", [one, ten])
    with pytest.raises(ValueError, match="down_blocks.1"):
        pag_select("down_blocks.1", [ten])
    # on the real names: level 1 of the tiny UNet has motion modules only
    got = pag_select("down_blocks.1", unet.self_attention_names())
    assert got and all(n.startswith("down_blocks.1.motion_modules.") for n in got)
    assert got == R.select_layers("down_blocks.1", unet.self_attention_names())


def test_spatial_cross_attention_is_never_selected_and_an_unmatched_id_raises(unet):
    names = unet.self_attention_names()
    with pytest.raises(ValueError, match="Cannot find PAG layer"):
        pag_select(r"mid_block\.attentions\.0.*attn2", names)
    assert pag_select("attn2", names) and all(".motion_modules." in n for n in pag_select("attn2", names))
    with pytest.raises(ValueError, match="no_such_block"):
        pag_select(["mid_block", "no_such_block"], names)
    with pytest.raises(ValueError, match="no_such_block"):
        R.select_layers(["mid_block", "no_such_block"], names)
    with pytest.raises(ValueError, match="no_such_block"):
        unet.set_pag_applied_layers("no_such_block")


def test_unet_marks_and_clears(unet):
    assert unet.set_pag_applied_layers("mid_block.*attn1") == [MID_SPATIAL, MID_MOTION1]
    assert unet.pag_applied_layers() == [MID_SPATIAL, MID_MOTION1]
    assert unet.mid_block.attentions[0].transformer_blocks[0].attn1.pag
    assert not unet.mid_block.attentions[0].transformer_blocks[0].attn2.pag
    assert unet.set_pag_applied_layers("up_blocks.1") and MID_SPATIAL not in unet.pag_applied_layers()
    assert unet.set_pag_applied_layers(None) == [] and unet.pag_applied_layers() == []


# ---------------------------------------------------------------- 2. the scale table
def ddim(n):
    s = DDIMScheduler.from_config(None, beta_schedule="linear", steps_offset=1, clip_sample=False)
    s.set_timesteps(n)
    return s


def test_adaptive_scale_clamps_at_zero():
    ts = ddim(4).timesteps
    assert ts.tolist() == ddim_ref.timesteps_leading(4).tolist() == [751, 501, 251, 1]
    want = R.scale_table(3.0, 0.005, ts.tolist())
    # on the reference: the last two steps clamp, the first two do not
    assert want[0] > 0 and want[1] > 0 and want[2] == 0 and want[3] == 0
    assert [R.get_pag_scale(3.0, 0.005, t) for t in (751, 501)] == [3.0 - 0.005 * 249, 3.0 - 0.005 * 499]
    got = ops.pag_scales(PerturbedAttentionGuidance(3.0, 0.005).table(ts))
    assert got.dtype == torch.float32 and torch.equal(got, want)
    # no adaptive scaling: the scale itself on every step
    assert torch.equal(ops.pag_scales(PerturbedAttentionGuidance(3.0, 0.0).table(ts)), torch.full((4,), 3.0))
    assert torch.equal(R.scale_table(3.0, 0.0, ts.tolist()), torch.full((4,), 3.0))
    # float timesteps (Euler's linspace) go through the same formula
    assert PerturbedAttentionGuidance(2.0, 0.001).scale_at(999.0) == R.get_pag_scale(2.0, 0.001, 999.0) == 2.0 - 0.001


def test_guidance_object_and_scales_refuse_bad_values():
    for bad in [(0.0, 0.0), (-1.0, 0.0), (3.0, -0.1), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("nan"))]:
        with pytest.raises(ValueError, match="pag_scale"):
            PerturbedAttentionGuidance(*bad)
    for bad in [[1.0, -0.5], [float("nan")], [float("inf"), 1.0], []]:
        with pytest.raises(ValueError, match="PAG scales"):
            ops.pag_scales(bad)


def test_pag_coef_layout():
    """n scales, zero padding to a multiple of 4 floats, then the scheduler's table, flattened."""
    assert [ops.pag_prefix(n) for n in (1, 3, 4, 5, 8, 9)] == [4, 4, 4, 8, 8, 12]
    rows = torch.arange(20, dtype=torch.float32).view(5, 4) + 100
    buf = ops.pag_coef([0.5, 1.5, 2.5, 3.5, 4.5], rows)
    assert buf.shape == (8 + 20,) and buf.dtype == torch.float32
    assert buf[:8].tolist() == [0.5, 1.5, 2.5, 3.5, 4.5, 0, 0, 0]
    assert torch.equal(buf[8:], rows.reshape(-1))
    with pytest.raises(ValueError, match="PAG scales"):
        ops.pag_coef([1.0, -1.0], rows)
    assert ops.STEP_PAG == L.VD_STEP_PAG == 0x800


def test_step_ops_check_the_prefixed_buffer_before_the_library():
    eps, lat = torch.zeros(8, 1), torch.zeros(1, 1, 1, 1, 4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.ddim_cfg_step(eps, 2, 1.0, lat, torch.zeros(8), pag_n=1)


# ---------------------------------------------------------------- 3. the pipeline's switches
def test_do_perturbed_attention_guidance_truth_table(unet):
    pipe = AnimateDiffPAGPipeline(unet)
    assert pipe.pag_applied_layers == ["mid_block.*attn1"] and unet.pag_applied_layers() == [MID_SPATIAL, MID_MOTION1]
    assert (pipe.pag_scale, pipe.pag_adaptive_scale) == (3.0, 0.0)
    rows = [(3.0, 0.0), (3.0, 0.005), (0.0, 0.0), (0.0, 0.005), (-1.0, 0.0), (3.0, -0.1)]
    for layers in (["mid_block.*attn1"], []):
        pipe.set_pag_applied_layers(layers)
        for scale, adaptive in rows:
            pipe._pag_scale, pipe._pag_adaptive_scale = scale, adaptive
            want = R.do_perturbed_attention_guidance(scale, adaptive, layers)
            assert want == (scale > 0 and adaptive >= 0 and bool(layers))
            assert pipe.do_perturbed_attention_guidance is want, (layers, scale, adaptive)
            assert pipe.do_pag_adaptive_scaling is (adaptive > 0 and scale > 0 and bool(layers))
    assert unet.pag_applied_layers() == []   # an empty list cleared the marks
    pipe.set_pag_applied_layers("mid_block")
    assert pipe.pag_applied_layers == ["mid_block"] and len(unet.pag_applied_layers()) == 3
    with pytest.raises(ValueError, match="no_such_block"):
        AnimateDiffPAGPipeline(unet, pag_applied_layers=["no_such_block"])
    with pytest.raises(ValueError, match="list of strings"):
        pipe.set_pag_applied_layers([1])


# ---------------------------------------------------------------- 4. the flag word
def test_entry_points_validate_the_flag_word_before_any_launch():
    """VD_STEP_PAG = 0x800 rides on ncfg: under it the low byte is 2 or 3, without it 3 stays
    VD_EINVAL, 0x200 stays VD_EINVAL with it as without, coef must be 16-byte aligned, and
    vd_euler_cfg_step takes this flag alone.  No GPU needed: every call returns before a launch."""
    h = L.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    args = lambda ncfg, coef=p: (p, 8, ncfg, 1.0, p, 1, 4, 1, 2, 2, coef, 1, None, None, None, 0, None)  # noqa: E731
    PAG, LCM, DPM = L.VD_STEP_PAG, L.VD_STEP_LCM, L.VD_STEP_DPM
    for fn in (h.vd_ddim_cfg_step, h.vd_euler_cfg_step):
        for low in (0, 1, 4, 5, 0xFF):
            assert fn(*args(low | PAG)) == L.VD_EINVAL, low
        assert fn(*args(3)) == L.VD_EINVAL
        assert fn(*args(2 | PAG | 0x200)) == L.VD_EINVAL
        assert fn(*args(3 | PAG | 0x200)) == L.VD_EINVAL
        assert fn(*args(2 | PAG | 0x1000)) == L.VD_EINVAL
        assert fn(*args(2 | PAG, coef=p + 4)) == L.VD_EINVAL
        assert fn(*args(3 | PAG, coef=p + 8)) == L.VD_EINVAL
        assert fn(*args(3 | PAG, coef=None)) == L.VD_EINVAL
    for flag in (LCM, DPM):
        assert h.vd_ddim_cfg_step(*args(1 | PAG | flag)) == L.VD_EINVAL
        assert h.vd_ddim_cfg_step(*args(4 | PAG | flag)) == L.VD_EINVAL
        assert h.vd_ddim_cfg_step(*args(3 | flag)) == L.VD_EINVAL
        assert h.vd_ddim_cfg_step(*args(3 | PAG | flag, coef=p + 4)) == L.VD_EINVAL
        assert h.vd_euler_cfg_step(*args(3 | PAG | flag)) == L.VD_EINVAL
        assert h.vd_euler_cfg_step(*args(2 | PAG | flag)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(3 | PAG | LCM | DPM)) == L.VD_EINVAL
    assert h.vd_ddim_cfg_step(*args(3 | PAG | DPM)) == L.VD_EINVAL   # DPM without its history
    assert h.vd_version() == 6


# ---------------------------------------------------------------- 5. the reference
@pytest.fixture(scope="module")
def case():
    return R.pag_case()


def test_reference_at_scale_zero_is_the_plain_cfg_loop(case):
    c = case
    acp = ddim_ref.alphas_cumprod()

    def unet_fn(x, t, ehs):
        return C.unet_forward_residuals(c["usd"], c["cfg"], x, t, ehs)
    with torch.no_grad():
        for g in (7.5, 1.0):
            want = ddim_ref.denoise_loop(unet_fn, c["lat"], c["ehs"] if g > 1 else c["ehs"][1:], 2, g, acp)
            got = R.ddim_loop(c["usd"], c["cfg"], c["lat"], c["ehs"], 2, g, 0.0, 0.0, c["layers"])
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), g
            on = R.ddim_loop(c["usd"], c["cfg"], c["lat"], c["ehs"], 2, g, 3.0, 0.0, c["layers"])
            assert torch.isfinite(on).all() and C.rel_l2(on, want) > 1e-3


def test_identity_attention_moves_the_perturbed_eps(case):
    c = case
    assert c["layers"] == [MID_SPATIAL, MID_MOTION1]
    with torch.no_grad():
        cond = C.unet_forward_residuals(c["usd"], c["cfg"], c["lat"], 961, c["ehs"][1:])
        pert = R.perturbed_eps(c["usd"], c["cfg"], c["lat"], 961, c["ehs"][1:], c["layers"])
        none = R.perturbed_eps(c["usd"], c["cfg"], c["lat"], 961, c["ehs"][1:], [])
    assert torch.equal(none, cond)
    assert torch.isfinite(pert).all() and C.rel_l2(pert, cond) > 1e-3
    # the combine, spelled out
    u = torch.full((3,), 1.0)
    assert R.combine([u, 2 * u, 4 * u], 7.5, 0.5).tolist() == [(1 + 7.5 * 1) + 0.5 * (2 - 4)] * 3
    assert R.combine([2 * u, 4 * u], 7.5, 0.5).tolist() == [2 + 0.5 * (2 - 4)] * 3


@pytest.mark.parametrize("kind", ["spatial", "motion"])
def test_block_case_separates_perturbed_from_plain_by_ten_bars(kind):
    """The device test's bars (3 x the bf16-emulating restatement's deviation) against what identity
    attention does to the same video in the fp32 restatement alone."""
    b = R.block_case(kind)
    bar = max(b["bar_kept"], b["bar_pert"])
    print(f"PAG block {kind}: emulated kept {b['emulated_kept']:.5f} pert {b['emulated_pert']:.5f} "
          f"separation {b['separation']:.5f} = {b['separation'] / bar:.1f} bars")
    assert 0 < bar <= R.BAR_CEILING
    assert b["separation"] >= 10 * bar
