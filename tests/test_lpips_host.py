"""LPIPS host side (CPU): checkpoint layouts -> the packed parameter blob, argument validation of
the vd_conv2d_f32 / vd_lpips_* entry points before any launch, and the unchanged behaviour of
measure_videos' signature."""
import ctypes
import inspect
from pathlib import Path

import pytest
import torch

import lpips_ref
import vdiff._lib as L
from vdiff import metrics, ops

EINVAL = 1000


@pytest.fixture(scope="module")
def sds():
    return lpips_ref.synthetic_state_dicts(1)


def test_blob_offsets_match_the_header():
    off = metrics.lpips_param_offsets()
    assert [off[f"w{l}"] for l in range(5)] == [0, 23232, 330432, 993984, 1878720]
    assert [off[f"b{l}"] for l in range(5)] == [2468544, 2468608, 2468800, 2469184, 2469440]
    assert [off[f"lin{l}"] for l in range(5)] == [2469696, 2469760, 2469952, 2470336, 2470592]
    assert (off["shift"], off["scale"], off["size"]) == (2470848, 2470851, 2470854)
    txt = (Path(__file__).resolve().parents[1] / "include" / "vdiff.h").read_text()
    for v in (23232, 330432, 993984, 1878720, 2468544, 2469696, 2470848, 2470851):
        assert str(v) in txt, v


def test_ohwi_repack_element_by_element(sds):
    alex, lin = sds
    blob = metrics.lpips_pack_params(alex, lin)
    off = metrics.lpips_param_offsets()
    assert blob.dtype == torch.float32 and blob.numel() == off["size"]
    for l, (idx, cin, cout, k, _, _) in enumerate(lpips_ref.CONVS):
        w = alex[f"features.{idx}.weight"]
        packed = blob[off[f"w{l}"]:off[f"w{l}"] + w.numel()].reshape(cout, k, k, cin)
        for o, i, y, x in ((0, 0, 0, 0), (cout - 1, cin - 1, k - 1, k - 1), (5, 2, 1, 2), (cout // 2, cin // 2, 0, k - 1)):
            assert packed[o, y, x, i] == w[o, i, y, x]
        assert torch.equal(packed, w.permute(0, 2, 3, 1))
        assert torch.equal(blob[off[f"b{l}"]:off[f"b{l}"] + cout], alex[f"features.{idx}.bias"])
        assert torch.equal(blob[off[f"lin{l}"]:off[f"lin{l}"] + cout], lin[f"lin{l}.model.1.weight"].reshape(-1))
    assert torch.equal(blob[off["shift"]:off["shift"] + 3], torch.tensor(lpips_ref.SHIFT))
    assert torch.equal(blob[off["scale"]:off["scale"] + 3], torch.tensor(lpips_ref.SCALE))


def test_both_checkpoint_layouts_load_to_the_same_blob(sds, tmp_path):
    alex, lin = sds
    want = metrics.LPIPS.from_state_dicts(alex, lin, device="cpu").params
    # torchvision AlexNet (with classifier keys, ignored) + the lpips package's alex.pth
    tv = dict(alex)
    tv["classifier.1.weight"], tv["classifier.1.bias"] = torch.zeros(8, 8), torch.zeros(8)
    torch.save(tv, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    got = metrics.LPIPS.from_files(tmp_path / "alexnet.pth", tmp_path / "alex.pth", device="cpu").params
    assert torch.equal(got, want)
    # one full lpips.LPIPS.state_dict(), with and without the lins.* aliases
    for alias in (True, False):
        torch.save(lpips_ref.full_state_dict(alex, lin, alias), tmp_path / "full.pth")
        got = metrics.LPIPS.from_files(tmp_path / "full.pth", device="cpu").params
        assert torch.equal(got, want)
    full = lpips_ref.full_state_dict(alex, lin)
    only_lins = {k: v for k, v in full.items() if not k.startswith("lin0.")}
    assert torch.equal(metrics.LPIPS.from_state_dicts(only_lins, device="cpu").params, want)
    # the library's own synthetic weights are the restatement's
    assert torch.equal(metrics.LPIPS.synthetic(1, device="cpu").params, want)
    with pytest.raises(FileNotFoundError):
        metrics.LPIPS.from_files(tmp_path / "absent.pth")


def test_missing_or_misshaped_keys_name_the_key(sds):
    alex, lin = sds
    bad = dict(alex)
    del bad["features.6.bias"]
    with pytest.raises(ValueError, match=r"features\.6\.bias"):
        metrics.lpips_pack_params(bad, lin)
    bad = dict(alex)
    bad["features.3.weight"] = alex["features.3.weight"].permute(0, 2, 3, 1)
    with pytest.raises(ValueError, match=r"features\.3\.weight"):
        metrics.lpips_pack_params(bad, lin)
    bad = dict(lin)
    bad["lin2.model.1.weight"] = lin["lin2.model.1.weight"].reshape(-1)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight"):
        metrics.lpips_pack_params(alex, bad)
    bad = dict(lin)
    del bad["lin4.model.1.weight"]
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight"):
        metrics.lpips_pack_params(alex, bad)
    full = lpips_ref.full_state_dict(alex, lin)
    del full["net.slice5.10.weight"]
    with pytest.raises(ValueError, match=r"net\.slice5\.10\.weight"):
        metrics.lpips_pack_params(full)
    with pytest.raises(ValueError, match="blob"):
        metrics.LPIPS(torch.zeros(7), device="cpu")


def test_entry_points_validate_before_launch():
    h = L.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    # vd_conv2d_f32: null operands, unsupported Cin / Cout, a kernel larger than the padded image
    ok = (p, 1, 8, 8, 4, p, p, 64, 3, 3, 1, 1, 1, p, None)
    for i in (0, 5, 13):
        a = list(ok)
        a[i] = None
        assert h.vd_conv2d_f32(*a) == EINVAL
    assert h.vd_conv2d_f32(p, 1, 8, 8, 5, p, p, 64, 3, 3, 1, 1, 1, p, None) == EINVAL
    assert h.vd_conv2d_f32(p, 1, 8, 8, 4, p, p, 96, 3, 3, 1, 1, 1, p, None) == EINVAL
    assert h.vd_conv2d_f32(p, 1, 2, 2, 4, p, p, 64, 5, 5, 1, 1, 0, p, None) == EINVAL
    assert h.vd_conv2d_f32(p, 0, 8, 8, 4, p, p, 64, 3, 3, 1, 1, 1, p, None) == EINVAL
    assert h.vd_conv2d_f32(p, 1, 8, 8, 4, p, p, 64, 3, 3, 0, 1, 1, p, None) == EINVAL
    assert h.vd_conv2d_f32(p + 4, 1, 8, 8, 4, p, p, 64, 3, 3, 1, 1, 1, p, None) == EINVAL  # unaligned float4 path
    # vd_lpips_layer: null operands, C not a multiple of 64 / too wide, no pairs, a short workspace
    nb = h.vd_lpips_layer_workspace(2)
    assert nb > 0 and h.vd_lpips_layer_workspace(0) == -1
    okl = (p, p, 2, 6, 64, p, p, 0, p, nb, None)
    for i in (0, 1, 5, 6, 8):
        a = list(okl)
        a[i] = None
        assert h.vd_lpips_layer(*a) == EINVAL
    assert h.vd_lpips_layer(p, p, 2, 6, 96, p, p, 0, p, nb, None) == EINVAL
    assert h.vd_lpips_layer(p, p, 2, 6, 576, p, p, 0, p, nb, None) == EINVAL
    assert h.vd_lpips_layer(p, p, 0, 6, 64, p, p, 0, p, nb, None) == EINVAL
    assert h.vd_lpips_layer(p, p, 2, 0, 64, p, p, 0, p, nb, None) == EINVAL
    assert h.vd_lpips_layer(p, p, 2, 6, 64, p, p, 0, p, nb - 1, None) == EINVAL
    # vd_lpips_workspace / vd_lpips_pairs: H = 30, frames = 1, null operands, one byte short
    assert h.vd_lpips_workspace(2, 30, 64) == -1 and h.vd_lpips_workspace(2, 64, 30) == -1
    assert h.vd_lpips_workspace(0, 64, 64) == -1
    need = h.vd_lpips_workspace(2, 31, 31)
    assert need > 0
    okp = (p, 1, 2, 31, 31, p, p, p, need, None)
    for i in (0, 5, 6, 7):
        a = list(okp)
        a[i] = None
        assert h.vd_lpips_pairs(*a) == EINVAL
    assert h.vd_lpips_pairs(p, 1, 2, 30, 31, p, p, p, need, None) == EINVAL
    assert h.vd_lpips_pairs(p, 1, 2, 31, 30, p, p, p, need, None) == EINVAL
    assert h.vd_lpips_pairs(p, 1, 1, 31, 31, p, p, p, need, None) == EINVAL
    assert h.vd_lpips_pairs(p, 0, 2, 31, 31, p, p, p, need, None) == EINVAL
    assert h.vd_lpips_pairs(p, 1, 2, 31, 31, p, p, p, need - 1, None) == EINVAL


def test_workspace_counts_every_buffer():
    """31x31: taps 7x7x64, 3x3x192, 1x1x{384,256,256}, pools 3x3x64 and 1x1x192, the scaled input
    and 64 fp64 partials per image."""
    floats = 31 * 31 * 3 + 1 + 49 * 64 + 9 * 64 + 9 * 192 + 192 + 384 + 256 + 256  # input padded to 4 floats
    assert L.lib().vd_lpips_workspace(1, 31, 31) == floats * 4 + 64 * 8
    assert L.lib().vd_lpips_workspace(16, 512, 512) < 16 * (16 << 20)


def test_cpu_tensors_are_refused():
    x = torch.zeros(1, 2, 32, 32, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        metrics.LPIPS.synthetic(0, device="cpu")(x)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.conv2d_f32(torch.zeros(1, 8, 8, 4), torch.zeros(64, 3, 3, 4))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.lpips_layer(torch.zeros(1, 6, 64), torch.zeros(1, 6, 64), torch.zeros(64))


def test_measure_videos_signature_unchanged():
    sig = inspect.signature(metrics.measure_videos)
    assert list(sig.parameters) == ["videos_u8", "lpips", "flow", "workspace_cap"]
    assert sig.parameters["lpips"].default is None and sig.parameters["flow"].default is True
    # None and a list of per-pair values go through video_metrics as before
    rec = metrics.video_metrics([10, 20], [3], 100, None)
    assert rec["mean_lpips"] is None and rec["std_lpips"] is None and rec["temporal_consistency_score"] is None
    assert all(m["lpips"] is None for m in rec["frame_metrics"])
    rec = metrics.video_metrics([10, 20], [3], 100, [0.25, 0.75])
    assert rec["mean_lpips"] == 0.5 and rec["std_lpips"] == 0.25
    assert [m["lpips"] for m in rec["frame_metrics"]] == [0.25, 0.75]
    from oracle import metrics_ref
    mse = [m["mse"] for m in rec["frame_metrics"]]
    assert rec["temporal_consistency_score"] == pytest.approx(metrics_ref.consistency_score(mse, [0.25, 0.75]), rel=1e-12)
    with pytest.raises(ValueError, match="no CPU fallback"):
        metrics.measure_videos(torch.zeros(1, 2, 32, 32, 3, dtype=torch.uint8), lpips=None)
