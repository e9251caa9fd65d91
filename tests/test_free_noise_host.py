"""FreeNoise on the CPU: the reference (tests/free_noise_ref.py) against itself and against the
oracle, the enable_free_noise / disable_free_noise surface, the rescheduled initial noise, and the
entry point's refusals before any launch."""
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

import free_noise_ref as R
import vdiff._lib as L
from oracle import unet_ref
from vdiff import AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline, UNetMotionModel, init_synthetic_, ops
from vdiff.config import TINY
from vdiff.models.blocks import AnimateDiffTransformer3D, free_noise_frame_weights

GOLD = Path(__file__).resolve().parent / "golden"

# (F, L, s) of the GPU kernel tests with the windows and the tail length each must give
WINDOWS = {
    (5, 4, 1): ([0, 1], 0),
    (7, 4, 2): ([0, 2, 3], 1),
    (9, 4, 3): ([0, 3, 5], 2),
    (8, 4, 4): ([0, 4], 0),
    (28, 16, 4): ([0, 4, 8, 12], 0),
    (20, 16, 4): ([0, 4], 0),
    (33, 32, 1): ([0, 1], 0),
    (6, 4, 2): ([0, 2], 0),
    (32, 16, 4): ([0, 4, 8, 12, 16], 0),
    (25, 16, 4): ([0, 4, 8, 9], 1),  # diffusers' own example: (0, 16), (4, 20), (8, 24), (9, 25)
    (40, 4, 2): (list(range(0, 37, 2)), 0),
}


# ---------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("fls", list(WINDOWS), ids=lambda v: "x".join(map(str, v)))
def test_window_lists(fls):
    F, Lc, s = fls
    starts, tail = WINDOWS[fls]
    idx, tail_len = R.frame_indices(F, Lc, s)
    assert [a for a, _ in idx] == starts and all(b - a == Lc for a, b in idx) and tail_len == tail
    assert ops.window_starts(F, Lc, s) == (starts, tail)
    # the issue's formulas
    n_reg = (F - Lc) // s + 1
    assert len(starts) == n_reg + (1 if (n_reg - 1) * s + Lc < F else 0)
    assert tail == F - ((n_reg - 1) * s + Lc)
    covered = set()
    for a, b in idx:
        covered |= set(range(a, b))
    assert covered == set(range(F))


def test_frame_indices_refuse_short_videos():
    with pytest.raises(ValueError):
        R.frame_indices(3, 4, 2)
    with pytest.raises(ValueError):
        ops.window_starts(3, 4, 2)
    with pytest.raises(ValueError):
        ops.window_starts(8, 4, 5)


def test_frame_weights():
    assert R.frame_weights(4, "flat") == [1.0] * 4
    assert R.frame_weights(4, "pyramid") == [1, 2, 2, 1]
    assert R.frame_weights(5, "pyramid") == [1, 2, 3, 2, 1]
    assert R.frame_weights(16, "pyramid") == [1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 6, 5, 4, 3, 2, 1]
    assert R.frame_weights(4, "delayed_reverse_sawtooth") == [0.01, 2, 2, 1]
    assert R.frame_weights(5, "delayed_reverse_sawtooth") == [0.01, 0.01, 3, 2, 1]
    assert R.frame_weights(6, "delayed_reverse_sawtooth") == [0.01, 0.01, 3, 3, 2, 1]
    for scheme in R.SCHEMES:
        for n in (1, 2, 3, 4, 5, 16, 31, 32):
            w = R.frame_weights(n, scheme)
            assert len(w) == n and all(v > 0 for v in w)
            assert free_noise_frame_weights(n, scheme) == w  # the product's table
    with pytest.raises(ValueError):
        R.frame_weights(4, "triangle")
    with pytest.raises(ValueError):
        free_noise_frame_weights(4, "triangle")


def test_merge_takes_the_tail_windows_last_frames_only():
    idx, tail = R.frame_indices(7, 4, 2)  # (0,4) (2,6) (3,7), tail 1
    chunks = [torch.full((1, 4, 1), float(v)) for v in (1, 2, 100)]
    out = R.merge_windows(chunks, idx, tail, [1, 2, 2, 1], 7)[0, :, 0]
    # frames 2, 3: (2 * 1 + 1 * 2) / 3 and (1 * 1 + 2 * 2) / 3; frame 6: the tail window alone
    torch.testing.assert_close(out, torch.tensor([1, 1, 4 / 3, 5 / 3, 2, 2, 100.0]))


@pytest.fixture(scope="module")
def tiny_sd():
    return {k: v.float() for k, v in init_synthetic_(UNetMotionModel("tiny"), seed=0).state_dict().items()}


@pytest.mark.parametrize("scheme", R.SCHEMES)
def test_one_window_is_the_plain_module_bitwise(tiny_sd, scheme):
    p = "down_blocks.0.motion_modules.0"
    x = torch.randn(2 * 4, 64, 3, 5, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        for rnd in (unet_ref._ident, unet_ref._bf16_round):
            want = unet_ref.motion_module(tiny_sd, p, x, 4, 2, 32, 32, rnd)
            got = R.motion_module(tiny_sd, p, x, 4, 2, 32, 32, (4, 2, scheme), rnd)
            assert torch.equal(got, want)
        more = R.motion_module(tiny_sd, p, torch.cat([x[:4], x[:2], x[4:], x[4:6]]), 6, 2, 32, 32, (4, 2, scheme))
    assert more.shape == (12, 64, 3, 5) and torch.isfinite(more).all()


def test_unet_forward_free_noise_without_it_is_the_oracle_bitwise(tiny_sd):
    g = np.load(GOLD / "tiny_unet.npz")
    lat = torch.from_numpy(g["latents"])[:1, :, :2, :16, :16]
    lat = torch.cat([lat, lat.flip(2), lat], 2)  # 6 frames
    x, ehs = torch.cat([lat, lat]), torch.from_numpy(g["ehs"])
    with torch.no_grad():
        for act in ("fp32", "bf16"):
            want = unet_ref.unet_forward(tiny_sd, TINY, x, 961, ehs, act=act)
            assert torch.equal(R.unet_forward_free_noise(tiny_sd, TINY, x, 961, ehs, None, act), want), act
        on = R.unet_forward_free_noise(tiny_sd, TINY, x, 961, ehs, (4, 2, "pyramid"), "fp32")
    assert on.shape == want.shape and not torch.equal(on, want)


# ---------------------------------------------------------------- API
def test_signatures_are_diffusers():
    want = ["self", "context_length", "context_stride", "weighting_scheme", "noise_type",
            "prompt_interpolation_callback"]
    for owner in (AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline):
        sig = inspect.signature(owner.enable_free_noise)
        assert list(sig.parameters) == want
        assert [p.default for p in list(sig.parameters.values())[1:]] == [16, 4, "pyramid", "shuffle_context", None]
        assert list(inspect.signature(owner.disable_free_noise).parameters) == ["self"]
        assert isinstance(owner.free_noise_enabled, property)
    sig = inspect.signature(UNetMotionModel.enable_free_noise)
    assert list(sig.parameters) == want[:4]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [16, 4, "pyramid"]
    assert isinstance(UNetMotionModel.free_noise_enabled, property)
    assert AnimateDiffVideoToVideoPipeline.enable_free_noise is AnimateDiffPipeline.enable_free_noise
    assert AnimateDiffVideoToVideoPipeline.disable_free_noise is AnimateDiffPipeline.disable_free_noise


def test_enable_free_noise_sets_every_motion_module_and_no_state_dict_key():
    m = UNetMotionModel("tiny")
    keys, names = list(m.state_dict()), [n for n, _ in m.named_modules()]
    mods = [x for x in m.modules() if isinstance(x, AnimateDiffTransformer3D)]
    assert len(mods) == 7 and mods == m.motion_modules_in_order()
    assert not m.free_noise_enabled and not any(x.free_noise_enabled for x in mods)
    m.enable_free_noise()
    assert m.free_noise_enabled
    assert all((x.context_length, x.context_stride, x.weighting_scheme) == (16, 4, "pyramid") for x in mods)
    m.enable_free_noise(context_length=None, context_stride=8, weighting_scheme="flat")
    assert all((x.context_length, x.context_stride, x.weighting_scheme) == (32, 8, "flat") for x in mods)
    assert list(m.state_dict()) == keys and [n for n, _ in m.named_modules()] == names
    m.disable_free_noise()
    assert not m.free_noise_enabled
    assert all((x.context_length, x.context_stride, x.weighting_scheme, x._fn_wt) == (None,) * 4 for x in mods)


def test_pipelines_forward_to_the_unet():
    unet = UNetMotionModel("tiny")
    pipe = AnimateDiffPipeline(unet)
    assert not pipe.free_noise_enabled
    pipe.enable_free_noise(context_length=8, context_stride=2, weighting_scheme="delayed_reverse_sawtooth",
                           noise_type="repeat_context")
    assert pipe.free_noise_enabled and unet.free_noise_enabled
    m = unet.mid_block.motion_modules[0]
    assert (m.context_length, m.context_stride, m.weighting_scheme) == (8, 2, "delayed_reverse_sawtooth")
    pipe.disable_free_noise()
    assert not pipe.free_noise_enabled and not unet.free_noise_enabled


def test_value_errors():
    unet = UNetMotionModel("tiny")
    pipe = AnimateDiffPipeline(unet)
    for owner in (unet, pipe):
        with pytest.raises(ValueError, match="weighting_scheme"):
            owner.enable_free_noise(weighting_scheme="triangle")
        with pytest.raises(ValueError, match="motion_max_seq_length"):
            owner.enable_free_noise(context_length=33)
        with pytest.raises(ValueError, match="context_length"):
            owner.enable_free_noise(context_length=0)
        with pytest.raises(ValueError, match="context_stride"):
            owner.enable_free_noise(context_length=8, context_stride=9)
        with pytest.raises(ValueError, match="context_stride"):
            owner.enable_free_noise(context_stride=0)
        assert not owner.free_noise_enabled  # a refused call changes nothing
    with pytest.raises(ValueError, match="noise_type"):
        pipe.enable_free_noise(noise_type="pink")
    assert not pipe.free_noise_enabled and not unet.free_noise_enabled


def test_out_of_scope_is_not_implemented_by_name():
    unet = UNetMotionModel("tiny")
    pipe = AnimateDiffPipeline(unet)
    with pytest.raises(NotImplementedError, match="prompt_interpolation_callback"):
        pipe.enable_free_noise(prompt_interpolation_callback=lambda *a: None)
    assert not pipe.free_noise_enabled
    with pytest.raises(NotImplementedError, match="SplitInferenceModule"):
        pipe.enable_free_noise_split_inference()
    with pytest.raises(NotImplementedError, match="prompt dict"):
        pipe(prompt={0: "a cat", 8: "a dog"}, num_frames=16, output_type="latent")
    # fewer frames than a window, and FreeNoise under a frame shard: refused before any launch
    unet.enable_free_noise(context_length=4, context_stride=2)
    m = unet.mid_block.motion_modules[0]
    with pytest.raises(ValueError, match="fewer than context_length"):
        m._free_noise_windows(3)
    with pytest.raises(NotImplementedError, match="FrameShard"):
        m._free_noise_windows(8, dist=object())
    assert m._free_noise_windows(4) is None  # one window: today's path
    unet.disable_free_noise()
    assert m._free_noise_windows(3) is None and m._free_noise_windows(8, dist=object()) is None


# ---------------------------------------------------------------- the initial noise
def cpu_pipe(**fn):
    pipe = AnimateDiffPipeline(UNetMotionModel("tiny"))
    pipe.enable_free_noise(**fn)
    return pipe


@pytest.mark.parametrize("F,Lc,s", [(16, 8, 4), (21, 8, 4), (11, 4, 3), (40, 16, 4)])
@pytest.mark.parametrize("dtype", [None, torch.float16])
def test_shuffle_context_noise(F, Lc, s, dtype):
    pipe = cpu_pipe(context_length=Lc, context_stride=s)
    pipe.torch_dtype = dtype
    got = pipe._prepare_latents_free_noise(2, F, 3, 5, generator=torch.Generator().manual_seed(11), device="cpu")
    want = R.prepare_latents_free_noise((2, 4, F, 3, 5), F, Lc, s, "shuffle_context",
                                        generator=torch.Generator().manual_seed(11), dtype=dtype or torch.float32)
    assert got.shape == (2, 4, F, 3, 5) and got.dtype == (dtype or torch.float32)
    assert torch.equal(got, want)
    plain = torch.randn((2, 4, F, 3, 5), generator=torch.Generator().manual_seed(11), dtype=dtype or torch.float32)
    assert torch.equal(got[:, :, :Lc], plain[:, :, :Lc])  # the first window is as drawn
    for f in range(Lc, F):  # every later frame is a copy of an earlier one, from the window L back
        src = [e for e in range(f) if torch.equal(got[:, :, f], got[:, :, e])]
        assert src, f
        i = Lc + (f - Lc) // s * s
        assert any(i - Lc <= e < i - Lc + s for e in src), (f, src)


def test_repeat_context_and_random_noise():
    pipe = cpu_pipe(context_length=4, context_stride=2, noise_type="repeat_context")
    got = pipe._prepare_latents_free_noise(1, 11, 3, 5, generator=torch.Generator().manual_seed(5), device="cpu")
    want = R.prepare_latents_free_noise((1, 4, 11, 3, 5), 11, 4, 2, "repeat_context",
                                        generator=torch.Generator().manual_seed(5))
    assert got.shape == (1, 4, 11, 3, 5) and torch.equal(got, want)
    drawn = torch.randn((1, 4, 4, 3, 5), generator=torch.Generator().manual_seed(5))
    for f in range(11):
        assert torch.equal(got[:, :, f], drawn[:, :, f % 4])
    pipe.enable_free_noise(context_length=4, context_stride=2, noise_type="random")
    got = pipe._prepare_latents_free_noise(1, 11, 3, 5, generator=torch.Generator().manual_seed(5), device="cpu")
    assert torch.equal(got, torch.randn((1, 4, 11, 3, 5), generator=torch.Generator().manual_seed(5)))


def test_user_latents():
    pipe = cpu_pipe(context_length=4, context_stride=2)
    full = torch.randn(1, 4, 9, 3, 5)
    assert torch.equal(pipe._prepare_latents_free_noise(1, 9, 3, 5, latents=full, device="cpu"), full)
    short = torch.randn(1, 4, 4, 3, 5)
    g = torch.Generator().manual_seed(2)
    ext = pipe._prepare_latents_free_noise(1, 9, 3, 5, generator=g, latents=short.clone(), device="cpu")
    want = R.prepare_latents_free_noise((1, 4, 9, 3, 5), 9, 4, 2, "shuffle_context",
                                        generator=torch.Generator().manual_seed(2), latents=short.clone())
    assert ext.shape == (1, 4, 9, 3, 5) and torch.equal(ext, want) and torch.equal(ext[:, :, :4], short)
    with pytest.raises(ValueError, match="frames"):
        pipe._prepare_latents_free_noise(1, 9, 3, 5, latents=torch.randn(1, 4, 5, 3, 5), device="cpu")


# ---------------------------------------------------------------- ops and the entry point
def test_ops_refuse_cpu_tensors():
    x, wt = torch.zeros(2 * 6 * 3, 8, dtype=torch.bfloat16), torch.ones(4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.window_gather(x, 2, 6, 3, 4, 2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.window_merge(torch.zeros(2 * 2 * 4 * 3, 8, dtype=torch.bfloat16), wt, 2, 6, 3, 4, 2)


def test_entry_point_refuses_before_launch():
    """Each call differs from a valid one (op 5 | stride 2 over B = 1, F = 6, hw = 2, L = 4, C = 8,
    the weights behind y; for op 4 y = NULL, y_f32 = 0) in the one argument named; all return
    VD_EINVAL (1000) with no launch."""
    h = L.lib()
    buf = torch.zeros(3, 512, dtype=torch.bfloat16)  # host memory: never dereferenced
    px, po, py = buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr()
    assert px % 16 == 0 and po % 16 == 0 and py % 4 == 0
    ST = ops.ROWS_WIN_STRIDE_SHIFT

    def call(op=5, s=2, x=px, y=py, Lc=4, y_f32=1, hw=2, F=6, rows=12, out=po):
        if op == 4 and y == py and y_f32 == 1:
            y, y_f32 = None, 0
        return h.vd_rows_eltwise(op | (s << ST), x, 8, y, Lc, y_f32, hw, F, rows, 8, out, 8, None)

    for op in (4, 5):
        assert call(op, s=0) == 1000            # s < 1: the plain op
        assert call(op, s=5) == 1000            # s > L
        assert call(op, Lc=0) == 1000           # L < 1 (and s > L)
        assert call(op, Lc=33, s=2, F=40, rows=80) == 1000  # L > 32
        assert call(op, F=3, rows=6) == 1000    # F < L
        assert call(op, rows=13) == 1000        # rows % (F * hw) != 0
        assert call(op, out=px) == 1000         # in place
        assert call(op, x=None) == 1000
        assert call(op, out=None) == 1000
        assert call(op, s=0x100) == 1000        # bits above the stride byte
    assert call(5, y=None) == 1000              # no weights
    assert call(5, y=py + 2) == 1000            # misaligned weights
    assert call(5, y_f32=0) == 1000
    assert call(4, y=py + 4) == 1000 and call(4, y=None, y_f32=1) == 1000
    for op in (0, 1, 2, 3):                     # no other op carries a stride
        assert h.vd_rows_eltwise(op | (2 << ST), px, 8, py, 8, 1, 2, 2, 4, 8, po, 8, None) == 1000
    assert h.vd_rows_eltwise(-1, px, 8, py, 0, 1, 2, 2, 4, 8, po, 8, None) == 1000
    assert h.vd_rows_eltwise(6 | (2 << ST), px, 8, py, 4, 1, 2, 6, 12, 8, po, 8, None) == 1000
