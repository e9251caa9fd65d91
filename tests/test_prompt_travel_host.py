"""FreeNoise prompt travel, CPU side: the reference's own properties, the host wrapper's and the
entry point's refusals, the pipelines' refusals by name, and that the planted faults the GPU tests
must catch move the reference by far more than their bar."""
import pytest
import torch

import free_noise_ref as R
import prompt_travel_case as T
import prompt_travel_ref as P
from vdiff import (AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline, AutoencoderKL, DDIMScheduler, DenoiseLoop,
                   UNetMotionModel, ops)
from vdiff.config import TINY
from vdiff.models.blocks import Ctx, text_rows_per_frame


# ---------------------------------------------------------------- the reference
def test_lerp_ref_reproduces_key_frames_and_a_single_prompt():
    g = torch.Generator().manual_seed(5)
    keys = torch.randn(2, 3, 5, 8, generator=g).to(T.BF)
    out = P.lerp_ref(keys, [0, 2, 6], 7)
    assert out.shape == (2, 7, 5, 8) and out.dtype == torch.float64
    for k, f in enumerate([0, 2, 6]):
        assert torch.equal(out[:, f], keys[:, k].double())
    assert torch.equal(out[:, 1], 0.5 * keys[:, 0].double() + 0.5 * keys[:, 1].double())
    w = (torch.tensor(3.0) / torch.tensor(4.0)).double()  # frame 5 between key frames 2 and 6
    assert torch.equal(out[:, 5], (1 - w) * keys[:, 1].double() + w * keys[:, 2].double())
    # {0: p}: the last prompt is repeated at the last frame, and every frame is that prompt
    frames, texts = P.normalise_prompt("a cat", 9)
    assert (frames, texts) == ([0, 8], ["a cat", "a cat"])
    one = P.lerp_ref(keys[:, [0, 0]], frames, 9)
    assert all(torch.equal(one[:, f], keys[:, 0].double()) for f in range(9))
    assert torch.equal(P.lerp_ref(keys[:, :1], [0], 1)[:, 0], keys[:, 0].double())
    assert torch.equal(P.lerp_operands(keys, [0, 2, 6], 7)[:, 1], torch.maximum(keys[:, 0].abs(), keys[:, 1].abs()).double())


def test_normalisation_and_its_errors():
    assert P.normalise_prompt({4: "b", 0: "a"}, 7) == ([0, 4, 6], ["a", "b", "b"])
    assert P.normalise_prompt({0: "a", 6: "b"}, 7) == ([0, 6], ["a", "b"])
    assert P.normalise_prompt({0: "a"}, 1) == ([0], ["a"])
    for norm in (P.normalise_prompt, AnimateDiffPipeline._prompt_travel_keys):
        with pytest.raises(ValueError, match="either `str` or `dict`"):
            norm(["a"], 7)
        with pytest.raises(ValueError, match="integer keys and string values"):
            norm({0: "a", "3": "b"}, 7)
        with pytest.raises(ValueError, match="integer keys and string values"):
            norm({0: "a", 3: 4}, 7)
        with pytest.raises(ValueError, match="minimum frame index in `prompt` dict must be 0"):
            norm({1: "a", 3: "b"}, 7)
        with pytest.raises(ValueError, match="maximum frame index in `negative_prompt` dict must be lesser than"):
            norm({0: "a", 7: "b"}, 7, "negative_prompt")
        assert norm({4: "b", 0: "a"}, 7) == ([0, 4, 6], ["a", "b", "b"])
    for bad, what in (([0, 3, 2, 6], "strictly increasing"), ([1, 6], "first frame index"), ([0, 5], "last frame index")):
        with pytest.raises(ValueError, match=what):
            P.lerp_ref(torch.zeros(len(bad), 1, 8), bad, 7)


def test_per_frame_reference_with_repeated_text_is_the_per_video_one_bitwise():
    _, sd = T.model()
    c = T.case(7)
    with torch.no_grad():
        want = R.unet_forward_free_noise(sd, TINY, c["x2"], 961, c["pv"], T.FN, "fp32")
        assert torch.equal(P.unet_forward_per_frame(sd, TINY, c["x2"], 961, c["pv"], T.FN, "fp32"), want)
        rep = c["pv"].repeat_interleave(7, 0)
        assert torch.equal(P.unet_forward_per_frame(sd, TINY, c["x2"], 961, rep, T.FN, "fp32"), want)
        with pytest.raises(ValueError, match="text rows"):
            P.unet_forward_per_frame(sd, TINY, c["x2"], 961, rep[:5], T.FN, "fp32")
    from oracle import unet_ref
    assert unet_ref.transformer2d.__module__ == "oracle.unet_ref"  # the patch is gone


def test_reference_moves_far_more_than_the_bar():
    """The GPU tests hold the device within BAR of this reference; each fault they must catch moves
    the reference itself by at least 5 BAR.  Measured on this model and these inputs (F = 7,
    FreeNoise (4, 2, "pyramid"), rel-L2 against the fp32 reference with per-frame text):
      the bf16-emulating reference                                  0.01578
      every frame given frame 0's text (a kv_div left at `frames`)  0.3579
      the text rolled by one frame (an off-by-one frame index)      0.2732
      the CFG halves swapped                                        0.3567
    With the stock (unsharpened) attn2 weights the text moves the output by 0.0024 only."""
    ref = T.reference(7, True)
    emu = T.rel_l2(T.reference(7, True, "bf16"), ref)
    print(f"bf16-emulating reference vs fp32: {emu:.5f}; BAR {T.BAR:.5f}")
    assert T.BAR >= 1.3 * emu
    for fault in ("frame0", "rolled", "swapped"):
        d = T.rel_l2(T.reference(7, True, "fp32", fault), ref)
        print(f"{fault}: {d:.4f} = {d / T.BAR:.1f} BAR")
        assert d >= 5 * T.BAR, (fault, d)


# ---------------------------------------------------------------- ops.prompt_lerp and the entry point
def test_prompt_lerp_wrapper_refusals(monkeypatch):
    def no_lib():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(ops, "lib", no_lib)
    assert ops.ROWS_PROMPT_LERP == 9 and ops.PROMPT_MAX == 256
    rows = torch.zeros(3 * 4, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="strictly increasing"):
        ops.prompt_lerp(rows, [0, 4, 2], 1, 7, 4)
    with pytest.raises(ValueError, match="strictly increasing"):
        ops.prompt_lerp(rows, [0, 2, 2], 1, 7, 4)
    with pytest.raises(ValueError, match="first frame index must be 0"):
        ops.prompt_lerp(rows, [1, 2, 6], 1, 7, 4)
    with pytest.raises(ValueError, match="last frame index must be 6"):
        ops.prompt_lerp(rows, [0, 2, 5], 1, 7, 4)
    with pytest.raises(TypeError, match="not an integer"):
        ops.prompt_lerp(rows, [0, 2.0, 6], 1, 7, 4)
    with pytest.raises(ValueError, match="key prompts and frames"):
        ops.prompt_lerp(rows, [0, 256], 1, 257, 4)
    with pytest.raises(ValueError, match="are not 1 videos x 3 key prompts x 5 tokens"):
        ops.prompt_lerp(rows, [0, 2, 6], 1, 7, 5)
    with pytest.raises(ValueError, match="are not 2 videos"):
        ops.prompt_lerp(rows, [0, 2, 6], 2, 7, 4)
    with pytest.raises(ValueError, match="C % 8"):
        ops.prompt_lerp(torch.zeros(12, 12, dtype=torch.bfloat16), [0, 2, 6], 1, 7, 4)
    with pytest.raises(ValueError, match="no CPU fallback"):  # past the index and shape checks
        ops.prompt_lerp(rows, [0, 2, 6], 1, 7, 4)


def test_op9_refuses_host_operands_and_every_bad_argument():
    """Host memory: nothing is launched.  The documented form with y on the host is refused for y
    alone; every other item of the VD_EINVAL list is refused whatever y is."""
    import vdiff._lib as L
    h = L.lib()
    assert h.vd_version() == 6
    buf = torch.zeros(3, 512, dtype=torch.bfloat16)
    px, po, py = buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr()

    def call(op=9, x=px, ldx=8, y=py, K=2, y_f32=1, L=2, F=2, rows=4, C=8, out=po, ldo=8):
        return h.vd_rows_eltwise(op, x, ldx, y, K, y_f32, L, F, rows, C, out, ldo, None)

    assert call() == 1000  # y is host memory
    assert call(op=9 | (1 << 8)) == 1000 and call(op=9 | (1 << 16)) == 1000
    assert call(K=0) == 1000 and call(K=257) == 1000 and call(F=0) == 1000 and call(F=257, rows=257 * 2) == 1000
    assert call(L=0) == 1000 and call(rows=5) == 1000 and call(rows=0) == 1000
    assert call(C=12, ldx=16, ldo=16) == 1000 and call(C=0) == 1000
    assert call(x=None) == 1000 and call(out=None) == 1000 and call(x=px + 2) == 1000 and call(out=po + 2) == 1000
    assert call(out=px) == 1000
    assert call(C=16, ldx=8, ldo=16) == 1000 and call(C=16, ldx=16, ldo=8) == 1000
    assert call(ldx=12) == 1000 and call(ldo=12) == 1000
    assert call(y=None) == 1000 and call(y=py + 2) == 1000 and call(y_f32=0) == 1000


# ---------------------------------------------------------------- the row forms
def test_text_row_forms():
    assert text_rows_per_frame(2 * 77, 2, 7, 77) is False and text_rows_per_frame(14 * 77, 2, 7, 77) is True
    assert text_rows_per_frame(2 * 77, 2, 1, 77) is False  # one frame: the two forms coincide
    with pytest.raises(ValueError, match="per-frame form"):
        text_rows_per_frame(3 * 77, 2, 7, 77)
    rows = torch.zeros(14 * 77, 64)
    assert Ctx(2, 7, None, rows, 77).text_per_frame and not Ctx(2, 7, None, rows[:2 * 77], 77).text_per_frame
    assert not Ctx(2, 7, None, None, 77).text_per_frame
    with pytest.raises(NotImplementedError, match="IP-Adapter"):
        Ctx(2, 7, None, rows, 77, ip_rows=torch.zeros(8, 64))
    with pytest.raises(NotImplementedError, match="frame sharding"):
        Ctx(2, 7, None, rows, 77, dist=object())
    unet = UNetMotionModel("tiny")
    unet._prepared = True  # the row count is refused before any operand is touched
    with pytest.raises(ValueError, match="one per frame"):
        unet(torch.zeros(2, 4, 7, 8, 8), 1, torch.zeros(3, 77, 64))


# ---------------------------------------------------------------- the pipelines' refusals
class _NoTokenizer:
    model_max_length = 77

    def __call__(self, *a, **k):
        raise AssertionError("the tokenizer was reached")


def test_pipeline_refusals_by_name():
    unet = UNetMotionModel("tiny")
    travel = {0: "a cat", 4: "a dog"}
    for cls, extra in ((AnimateDiffPipeline, dict(num_frames=7)),
                       (AnimateDiffVideoToVideoPipeline, dict(latents=torch.zeros(1, 4, 7, 8, 8)))):
        pipe = cls(unet, **({} if cls is AnimateDiffPipeline else {"vae": AutoencoderKL("tiny", encoder=True)}))
        pipe.tokenizer = _NoTokenizer()
        kw = dict(extra, output_type="latent", num_inference_steps=2)
        # FreeNoise disabled: refused before any tokenizer or device work, and it says what is needed
        for p in (dict(prompt=travel), dict(prompt="a cat", negative_prompt={0: "blurry"})):
            with pytest.raises(NotImplementedError, match="prompt dict.*enable_free_noise"):
                pipe(**p, **kw)
        with pytest.raises(NotImplementedError, match="prompt_interpolation_callback"):
            pipe.enable_free_noise(prompt_interpolation_callback=lambda *a: None)
        assert not pipe.free_noise_enabled
        with pytest.raises(NotImplementedError, match="need FreeNoise"):  # precomputed per-frame embeddings
            pipe(prompt_embeds=torch.zeros(1, 7, 77, 64), negative_prompt_embeds=torch.zeros(1, 7, 77, 64), **kw)
        pipe.enable_free_noise(context_length=4, context_stride=2)
        try:
            with pytest.raises(NotImplementedError, match="IP-Adapter"):
                pipe(prompt=travel, ip_adapter_image_embeds=torch.zeros(2, 1, 32), **kw)
            with pytest.raises(NotImplementedError, match="cfg_shard"):
                pipe(prompt=travel, cfg_shard=object(), **kw)
            pipe.dist = object()
            with pytest.raises(NotImplementedError, match="frame-sharded"):
                pipe(prompt=travel, **kw)
            pipe.dist = None
            with pytest.raises(ValueError, match="either `str` or `dict`"):
                pipe(prompt=travel, negative_prompt=["blurry"], **kw)
            with pytest.raises(ValueError, match="maximum frame index in `prompt` dict"):
                pipe(prompt={0: "a cat", 7: "a dog"}, **kw)
            with pytest.raises(ValueError, match="minimum frame index in `negative_prompt` dict"):
                pipe(prompt=travel, negative_prompt={2: "blurry"}, **kw)
        finally:
            pipe.disable_free_noise()


def test_denoise_loop_refuses_per_frame_text_by_name():
    """Before any device work: the model is not even prepared."""
    unet = UNetMotionModel("tiny")
    sched = DDIMScheduler(beta_schedule="linear", steps_offset=1, clip_sample=False)
    sched.set_timesteps(3)
    lat, pf = torch.zeros(1, 4, 7, 8, 8), torch.zeros(2 * 7, 77, 64)
    with pytest.raises(NotImplementedError, match="per-frame text.*ip_embeds"):
        DenoiseLoop(unet, sched, lat, pf, 7.5, ip_embeds=torch.zeros(2, 4, 64))
    with pytest.raises(NotImplementedError, match="per-frame text.*cfg_shard"):
        DenoiseLoop(unet, sched, lat, pf, 7.5, cfg_shard=object())
    with pytest.raises(NotImplementedError, match="per-frame text.*perturbed-attention"):
        DenoiseLoop(unet, sched, lat, torch.zeros(3 * 7, 77, 64), 7.5, pag=object())
    unet.dist = object()
    with pytest.raises(NotImplementedError, match="per-frame text.*frame sharding"):
        DenoiseLoop(unet, sched, lat, pf, 7.5)
    assert not unet._prepared
