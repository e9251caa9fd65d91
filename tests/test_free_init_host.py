"""FreeInit on the CPU: the reference (tests/free_init_ref.py) against itself, the half-spectrum
identity the kernel rests on with ops.free_init_table, the enable_free_init / disable_free_init
surface, and the entry point's refusals before any launch."""
import inspect
import math

import pytest
import torch

import free_init_ref as R
import vdiff._lib as L
from vdiff import AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline, UNetMotionModel, ops

METHODS = ("butterworth", "gaussian", "ideal")
SHAPES = [(1, 1, 3, 4, 6), (2, 4, 4, 8, 8), (1, 2, 5, 6, 10), (1, 1, 7, 9, 5), (1, 4, 16, 32, 32), (1, 1, 32, 24, 40),
          (1, 4, 16, 64, 64)]


# ---------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("method", METHODS)
def test_mask_is_zero_at_stop_frequency_zero(method):
    for ds, dt in ((0, 0.25), (0.25, 0), (0, 0)):
        assert not R._get_free_init_freq_filter((1, 4, 4, 6, 8), method, 4, ds, dt).any()
        assert not ops.free_init_mask(4, 6, 8, method, 4, ds, dt).any()
        assert not ops.free_init_table(4, 6, 8, method, 4, ds, dt).any()


def test_mask_formulas_at_hand_computed_points():
    shape, ds, dt = (1, 1, 4, 8, 8), 0.25, 0.5
    # (t, h, w) = (1, 2, 6): d^2 = ((0.25 / 0.5) * (2 / 4 - 1))^2 + (4 / 8 - 1)^2 + (12 / 8 - 1)^2
    d2 = (0.5 * -0.5) ** 2 + 0.25 + 0.25
    assert d2 == 0.5625
    b = R._get_free_init_freq_filter(shape, "butterworth", 2, ds, dt)
    assert b.shape == shape and b.dtype == torch.float64
    assert b[0, 0, 1, 2, 6].item() == pytest.approx(1 / (1 + (d2 / 0.0625) ** 2), rel=1e-15)  # 1 / 82
    g = R._get_free_init_freq_filter(shape, "gaussian", 4, ds, dt)
    assert g[0, 0, 1, 2, 6].item() == pytest.approx(math.exp(-d2 / (2 * 0.0625)), rel=1e-15)
    i = R._get_free_init_freq_filter(shape, "ideal", 4, ds, dt)
    assert i[0, 0, 1, 2, 6].item() == 0.0          # 0.5625 > 2 * 0.25
    assert i[0, 0, 2, 2, 6].item() == 1.0          # t at the centre: d^2 = 0.5 <= 0.5
    assert i[0, 0, 2, 2, 7].item() == 0.0          # 0.25 + 0.5625 > 0.5
    # the centre (N / 2 on every axis) is d^2 = 0
    for method, m in (("butterworth", b), ("gaussian", g), ("ideal", i)):
        assert m[0, 0, 2, 4, 4].item() == R.centre_value(method, 4, ds) == 1.0
    with pytest.raises(NotImplementedError, match="`filter_type` must be one of gaussian, butterworth or ideal"):
        R._get_free_init_freq_filter(shape, "box", 4, ds, dt)
    with pytest.raises(NotImplementedError, match="`filter_type` must be one of gaussian, butterworth or ideal"):
        ops.free_init_table(4, 8, 8, "box")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_half_spectrum_identity(shape, method):
    """noise + irfftn(table * rfftn(x - noise)) is the literal reference in fp64 (measured: at
    most 2.2e-15), the odd sizes included, where the mask is not its own mirror."""
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, dtype=torch.float64, generator=g)
    noise = torch.randn(shape, dtype=torch.float64, generator=g)
    F, H, W = shape[-3:]
    lpf = R._get_free_init_freq_filter((1,) + shape[1:], method, 4, 0.25, 0.25)
    assert torch.equal(lpf[0, 0], ops.free_init_mask(F, H, W, method, 4, 0.25, 0.25))
    want = R._apply_freq_filter(x, noise, lpf)
    table = ops.free_init_table(F, H, W, method, 4, 0.25, 0.25, dtype=torch.float64)
    assert table.shape == (F, H, W // 2 + 1) and table.is_contiguous()
    err = (R.half_spectrum_filter(x, noise, table) - want).abs().max().item()
    assert err <= 1e-12, err
    t32 = ops.free_init_table(F, H, W, method, 4, 0.25, 0.25)
    assert t32.dtype == torch.float32 and torch.equal(t32, table.float())  # one rounding
    if F % 2 == 0 and H % 2 == 0 and W % 2 == 0:
        # un-shifted: DC holds the mask's centre value, and the mask was even already
        assert table[0, 0, 0].item() == lpf[0, 0, F // 2, H // 2, W // 2].item() == 1.0
        # (up to the rounding of 2 n / N - 1, which is not mirror-symmetric for every N)
        raw = torch.fft.ifftshift(lpf[0, 0], dim=(0, 1, 2))[:, :, :W // 2 + 1]
        assert (table - raw).abs().max().item() <= 1e-15
    else:
        # without the symmetrisation the identity fails: the mask differs from its mirror
        raw = torch.fft.ifftshift(lpf[0, 0], dim=(0, 1, 2))[:, :, :W // 2 + 1]
        assert (R.half_spectrum_filter(x, noise, raw) - want).abs().max().item() > 1e-6


def test_filter_moves_the_result_away_from_both_inputs():
    shape = (1, 4, 16, 32, 32)
    g = torch.Generator().manual_seed(0)
    x, noise = (torch.randn(shape, dtype=torch.float64, generator=g) for _ in range(2))
    want = R._apply_freq_filter(x, noise, R._get_free_init_freq_filter((1,) + shape[1:], "butterworth", 4, 0.25, 0.25))
    assert (want - noise).abs().max() > 0.03 and (want - x).abs().max() > 3


# ---------------------------------------------------------------- API
def test_signatures_are_diffusers():
    want = ["self", "num_iters", "use_fast_sampling", "method", "order", "spatial_stop_frequency",
            "temporal_stop_frequency"]
    for owner in (AnimateDiffPipeline, AnimateDiffVideoToVideoPipeline):
        sig = inspect.signature(owner.enable_free_init)
        assert list(sig.parameters) == want
        assert [p.default for p in list(sig.parameters.values())[1:]] == [3, False, "butterworth", 4, 0.25, 0.25]
        assert {k: p.default for k, p in list(sig.parameters.items())[1:]} == R.FREE_INIT_DEFAULTS
        assert list(inspect.signature(owner.disable_free_init).parameters) == ["self"]
        assert isinstance(owner.free_init_enabled, property)
        assert callable(owner._apply_free_init)
    assert AnimateDiffVideoToVideoPipeline.enable_free_init is AnimateDiffPipeline.enable_free_init
    assert AnimateDiffVideoToVideoPipeline.disable_free_init is AnimateDiffPipeline.disable_free_init


def test_enable_disable_and_refusals():
    pipe = AnimateDiffPipeline(UNetMotionModel("tiny"))
    assert not pipe.free_init_enabled
    pipe.enable_free_init()
    assert pipe.free_init_enabled
    assert (pipe._free_init_num_iters, pipe._free_init_use_fast_sampling, pipe._free_init_method,
            pipe._free_init_order, pipe._free_init_spatial_stop_frequency,
            pipe._free_init_temporal_stop_frequency) == (3, False, "butterworth", 4, 0.25, 0.25)
    pipe.disable_free_init()
    assert not pipe.free_init_enabled
    with pytest.raises(ValueError, match="num_iters"):
        pipe.enable_free_init(num_iters=0)
    with pytest.raises(NotImplementedError, match="`filter_type` must be one of gaussian, butterworth or ideal"):
        pipe.enable_free_init(method="box")
    with pytest.raises(ValueError, match="order"):
        pipe.enable_free_init(order=0)
    with pytest.raises(ValueError, match="stop frequencies"):
        pipe.enable_free_init(spatial_stop_frequency=-0.1)
    with pytest.raises(ValueError, match="stop frequencies"):
        pipe.enable_free_init(temporal_stop_frequency=-0.1)
    assert not pipe.free_init_enabled  # a refused call changes nothing
    pipe.enable_free_init(num_iters=1, method="ideal", spatial_stop_frequency=0)
    assert pipe.free_init_enabled and pipe._free_init_method == "ideal"


@pytest.mark.parametrize("n,iters", [(25, 3), (4, 3), (1, 3), (50, 5)])
def test_fast_sampling_step_counts(n, iters):
    pipe = AnimateDiffPipeline(UNetMotionModel("tiny"))
    pipe.enable_free_init(num_iters=iters, use_fast_sampling=True)
    got = [pipe._free_init_steps(n, i) for i in range(iters)]
    assert got == [max(1, int(n / iters * (i + 1))) for i in range(iters)]
    assert got == [R.fast_sampling_steps(n, iters, i) for i in range(iters)]
    pipe.enable_free_init(num_iters=iters)
    assert [pipe._free_init_steps(n, i) for i in range(iters)] == [n] * iters


def test_apply_free_init_on_the_cpu_is_the_reference():
    """The first iteration keeps the latents and sets the schedule; the reference's later iteration,
    composed with the half-spectrum identity in fp64, matches its literal form."""
    pipe = AnimateDiffPipeline(UNetMotionModel("tiny"))
    pipe.enable_free_init(num_iters=3, use_fast_sampling=True)
    lat = torch.randn(1, 4, 4, 8, 8, generator=torch.Generator().manual_seed(3))
    out, ts = pipe._apply_free_init(lat, 0, 6)
    assert out is lat and torch.equal(pipe._free_init_initial_noise, lat) and pipe._free_init_initial_noise is not lat
    assert len(ts) == 2 and torch.equal(ts, pipe.scheduler.timesteps)
    assert pipe._free_init_table.shape == (4, 8, 5) and pipe._free_init_scratch.numel() == 4 * 4 * 8 * 10

    def randn(shape, generator=None, device=None, dtype=None):
        return torch.randn(shape, generator=generator, dtype=dtype)

    ref = R.FreeInit(pipe.scheduler, randn, num_iters=3, use_fast_sampling=True)
    same, n0 = ref.apply(lat, 0, 6, None)
    assert same is lat and n0 == 2
    x = torch.randn(1, 4, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    got, n1 = ref.apply(x, 1, 6, torch.Generator().manual_seed(5), dtype=torch.float64)
    assert n1 == 4
    z_t = pipe.scheduler.add_noise(x, lat, torch.full((1,), 999))
    z_rand = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
    table = ops.free_init_table(4, 8, 8, dtype=torch.float64)
    want = R.half_spectrum_filter(z_t.double(), z_rand.double(), table).float()
    assert (got - want).abs().max() <= 1e-6


# ---------------------------------------------------------------- ops and the entry point
def test_ops_refuse_cpu_tensors():
    z = torch.zeros(2, 3, 4, 6)
    table = ops.free_init_table(3, 4, 6)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.free_init_filter(z, z.clone(), table)


def test_entry_point_refuses_before_launch():
    """One valid baseline per pass (n_vol = 2, F = 3, H = 4, W = 6, so Wh = 4 and a complex row is
    8 floats); each call differs from it in the one argument named and returns VD_EINVAL (1000)
    with no launch."""
    h = L.lib()
    buf = torch.zeros(4, 1024, dtype=torch.float32)  # host memory: never dereferenced
    px, pn, ps, po = (buf[i].data_ptr() for i in range(4))
    assert all(p % 16 == 0 for p in (px, pn, ps, po))
    F, H, W, Wh, rows = 3, 4, 6, 4, 24
    base = {
        1: dict(x=px, ldx=W, y=pn, ldy=W, y_f32=1, out=ps, ldo=2 * Wh),
        2: dict(x=ps, ldx=2 * Wh, y=None, ldy=0, y_f32=0, out=ps, ldo=2 * Wh),
        3: dict(x=ps, ldx=2 * Wh, y=pn, ldy=Wh, y_f32=1, out=ps, ldo=2 * Wh),
        4: dict(x=ps, ldx=2 * Wh, y=None, ldy=0, y_f32=0, out=ps, ldo=2 * Wh),
        5: dict(x=ps, ldx=2 * Wh, y=pn, ldy=W, y_f32=1, out=po, ldo=W),
    }

    def call(p, op=None, H=H, F=F, rows=rows, W=W, **kw):
        a = dict(base[p], **kw)
        op = (6 | (p << ops.ROWS_SPEC_PASS_SHIFT)) if op is None else op
        return h.vd_rows_eltwise(op, a["x"], a["ldx"], a["y"], a["ldy"], a["y_f32"], H, F, rows, W, a["out"],
                                 a["ldo"], None)

    assert ops.ROWS_SPECTRAL == 6 and ops.ROWS_SPEC_PASS_SHIFT == 8
    for p in range(1, 6):
        assert call(p, op=6) == 1000                       # the plain op: no pass
        assert call(p, op=6 | (6 << 8)) == 1000            # pass 6
        assert call(p, op=6 | (p << 8) | (1 << 16)) == 1000  # a bit above the pass byte
        assert call(p, op=6 | (p << 8) | (1 << 30)) == 1000
        assert call(p, rows=25) == 1000                    # rows % (F * H) != 0
        assert call(p, x=None) == 1000
        assert call(p, out=None) == 1000
        assert call(p, x=base[p]["x"] + 4, **({"out": base[p]["out"] + 4} if p in (2, 3, 4) else {})) == 1000
        assert call(p, F=ops.SPECTRAL_MAX + 1, rows=(ops.SPECTRAL_MAX + 1) * H) == 1000   # beyond the limit
        assert call(p, H=ops.SPECTRAL_MAX + 1, rows=(ops.SPECTRAL_MAX + 1) * F) == 1000
        assert call(p, W=ops.SPECTRAL_MAX + 1, ldx=1024, ldo=1024, ldy=1024) == 1000
        assert call(p, F=0) == 1000 and call(p, H=0) == 1000 and call(p, W=0) == 1000
    assert ops.SPECTRAL_MAX >= 128
    for p in (1, 5):
        assert call(p, out=base[p]["x"]) == 1000           # in place
        assert call(p, out=base[p]["out"] + 4) == 1000     # out not 16-byte aligned
        assert call(p, y=None) == 1000
        assert call(p, y=pn + 4) == 1000                   # misaligned
        assert call(p, y_f32=0) == 1000
        assert call(p, ldy=W - 1) == 1000                  # strides shorter than the row
    assert call(1, ldx=W - 1) == 1000 and call(1, ldo=2 * Wh - 2) == 1000
    assert call(5, ldo=W - 1) == 1000 and call(5, ldx=2 * Wh - 2) == 1000
    assert call(1, ldo=2 * Wh + 1) == 1000 and call(5, ldx=2 * Wh + 1) == 1000   # an odd complex stride
    for p in (2, 3, 4):
        assert call(p, out=po) == 1000                     # not in place
        assert call(p, ldx=2 * Wh - 2, ldo=2 * Wh - 2) == 1000
        assert call(p, ldo=2 * Wh + 2) == 1000             # one buffer, two strides
    for p in (2, 4):
        assert call(p, y=pn) == 1000                       # y set where the pass does not read it
        assert call(p, y_f32=1) == 1000
    assert call(3, y=None) == 1000 and call(3, y=pn + 4) == 1000 and call(3, y_f32=0) == 1000
    assert call(3, ldy=Wh + 1) == 1000                     # the table is contiguous
    # the call tests/test_free_noise_host.py pinned before op 6 existed
    b16 = torch.zeros(3, 512, dtype=torch.bfloat16)
    qx, qo, qy = b16[0].data_ptr(), b16[1].data_ptr(), b16[2].data_ptr()
    assert h.vd_rows_eltwise(6 | (2 << 8), qx, 8, qy, 4, 1, 2, 6, 12, 8, qo, 8, None) == 1000
    # ops 0-5 still refuse a pass byte with these operands, and ops 0-3 with their own
    for op in range(6):
        assert call(1, op=op | (1 << 8)) == 1000
    for op in (0, 1, 2, 3):
        assert h.vd_rows_eltwise(op | (2 << 8), qx, 8, qy, 8, 1, 2, 2, 4, 8, qo, 8, None) == 1000
    assert h.vd_rows_eltwise(7, qx, 8, qy, 8, 1, 2, 2, 4, 8, qo, 8, None) == 1000
