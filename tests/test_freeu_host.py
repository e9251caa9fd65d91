"""FreeU on the CPU: the reference (tests/freeu_ref.py) against itself and against the oracle, the
enable_freeu / disable_freeu surface, and the entry point's refusals before any launch."""
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

import freeu_ref as R
import vdiff._lib as L
from oracle import unet_ref
from vdiff import AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline, UNetMotionModel, init_synthetic_
from vdiff.config import TINY

GOLD = Path(__file__).resolve().parent / "golden"
FREEU = (0.9, 0.2, 1.2, 1.4)  # s1, s2, b1, b2


@pytest.mark.parametrize("hw", [(2, 2), (2, 7), (3, 5), (5, 2), (6, 4), (8, 8), (16, 16)])
@pytest.mark.parametrize("s", [0.2, 0.9])
def test_closed_form_is_the_fourier_filter(hw, s):
    x = torch.randn(2, 3, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(hw[0] * 17 + hw[1]))
    err = (R.closed_form(x, s) - R.fourier_filter(x, 1, s)).abs().max().item()
    assert err <= 1e-12, err


def test_unet_forward_freeu_without_freeu_is_the_oracle_bitwise():
    g = np.load(GOLD / "tiny_unet.npz")
    sd = {k: v.float() for k, v in init_synthetic_(UNetMotionModel("tiny"), seed=0).state_dict().items()}
    lat = torch.from_numpy(g["latents"])[:, :, :2, :32, :32]
    x, ehs = torch.cat([lat, lat]), torch.from_numpy(g["ehs"])
    with torch.no_grad():
        for act in ("fp32", "bf16"):
            want = unet_ref.unet_forward(sd, TINY, x, 961, ehs, act=act)
            assert torch.equal(R.unet_forward_freeu(sd, TINY, x, 961, ehs, None, act), want), act
        on = R.unet_forward_freeu(sd, TINY, x, 961, ehs, FREEU, "fp32")
    assert not torch.equal(on, want)


def test_apply_freeu_touches_blocks_0_and_1_only():
    h, r = torch.randn(2, 16, 4, 6), torch.randn(2, 8, 4, 6)
    h0, r0 = R.apply_freeu(0, h, r, *FREEU)
    assert torch.equal(h0[:, :8], h[:, :8] * 1.2) and torch.equal(h0[:, 8:], h[:, 8:])
    torch.testing.assert_close(r0, R.fourier_filter(r, 1, 0.9))
    h1, r1 = R.apply_freeu(1, h, r, *FREEU)
    assert torch.equal(h1[:, :8], h[:, :8] * 1.4)
    torch.testing.assert_close(r1, R.closed_form(r, 0.2), rtol=1e-5, atol=1e-6)
    h2, r2 = R.apply_freeu(2, h, r, *FREEU)
    assert h2 is h and r2 is r


# ---------------------------------------------------------------- API
def test_enable_freeu_sets_every_up_block_and_activates_two():
    m = UNetMotionModel("tiny")
    assert [b.resolution_idx for b in m.up_blocks] == list(range(len(m.up_blocks)))
    assert not any(b.freeu_active for b in m.up_blocks)
    assert all((b.s1, b.s2, b.b1, b.b2) == (None,) * 4 for b in m.up_blocks)
    m.enable_freeu(0.9, 0.2, 1.2, 1.4)
    for b in m.up_blocks:
        assert (b.s1, b.s2, b.b1, b.b2) == (0.9, 0.2, 1.2, 1.4)
    m.disable_freeu()
    assert all((b.s1, b.s2, b.b1, b.b2) == (None,) * 4 for b in m.up_blocks)
    assert not any(b.freeu_active for b in m.up_blocks)


def test_only_resolution_idx_0_and_1_are_active():
    with torch.device("meta"):  # four up blocks; module construction only
        m = UNetMotionModel("full")
    m.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
    assert [b.freeu_active for b in m.up_blocks] == [True, True, False, False]
    m.up_blocks[0].b1 = None  # all four must be set
    assert not m.up_blocks[0].freeu_active


def test_signatures_are_diffusers():
    for owner in (UNetMotionModel, AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline):
        assert list(inspect.signature(owner.enable_freeu).parameters) == ["self", "s1", "s2", "b1", "b2"]
        assert list(inspect.signature(owner.disable_freeu).parameters) == ["self"]


def test_pipeline_methods_forward_to_the_unet():
    assert AnimateDiffVideoToVideoPipeline.enable_freeu is AnimateDiffPipeline.enable_freeu
    assert AnimateDiffVideoToVideoPipeline.disable_freeu is AnimateDiffPipeline.disable_freeu
    unet = UNetMotionModel("tiny")
    pipe = AnimateDiffPipeline(unet)
    pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
    assert [b.freeu_active for b in unet.up_blocks] == [True, True]
    assert (unet.up_blocks[1].s2, unet.up_blocks[1].b2) == (0.2, 1.4)
    pipe.disable_freeu()
    assert not any(b.freeu_active for b in unet.up_blocks)


def test_half_of_the_hidden_channels_must_be_a_multiple_of_8():
    m = UNetMotionModel("tiny")
    m.enable_freeu(*FREEU)
    with pytest.raises(NotImplementedError, match="hidden channels"):
        m.up_blocks[0]._freeu_operands(24)


def test_ops_refuse_cpu_tensors():
    from vdiff import ops
    x, s = torch.zeros(8, 8, dtype=torch.bfloat16), torch.ones(1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.freeu_filter(x, 2, 2, 2, s)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.scale_rows_(x, s)


# ---------------------------------------------------------------- refusals before any launch
def test_entry_point_refuses_before_launch():
    """Each call differs from a valid one (op 2 on 4 rows of 8 channels, H = W = 2, out != x, the
    scalar behind y) in the one argument named; all return VD_EINVAL (1000) with no launch."""
    h = L.lib()
    buf = torch.zeros(3, 64, dtype=torch.bfloat16)  # host memory: never dereferenced
    px, po, py = buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr()
    assert px % 16 == 0 and po % 16 == 0 and py % 4 == 0

    def call(op=2, x=px, y=py, ldy=0, y_f32=1, W=2, H=2, rows=4, out=po):
        return h.vd_rows_eltwise(op, x, 8, y, ldy, y_f32, W, H, rows, 8, out, 8, None)

    assert call(H=1, rows=2) == 1000          # H < 2
    assert call(W=1, rows=2) == 1000          # W < 2
    assert call(rows=6) == 1000               # rows % (H * W) != 0
    assert call(y=None) == 1000               # no scalar
    assert call(out=px) == 1000               # in place
    assert call(x=None) == 1000
    assert call(y=py + 2) == 1000             # the scalar is not 4-byte aligned
    assert call(y_f32=0) == 1000 and call(ldy=8) == 1000
    assert call(H=4000, W=4000, rows=16000000) == 1000  # the twiddle table is bounded
    assert call(op=3, y=None) == 1000 and call(op=3, y_f32=0) == 1000
    assert call(op=4) == 1000 and call(op=-1) == 1000
