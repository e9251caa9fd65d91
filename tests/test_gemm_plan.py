"""The GEMM plan, pinned on the CPU: every descriptor of tests/golden/make_plan_golden.py's grid goes
through vd_gemm_plan and vd_gemm_ws_bytes (host-only, no launch; without a device the library plans
for the MI355X's 256 CUs) and must give the kernel, split and workspace size recorded in
tests/golden/gemm_plan.npz.  The plan fixes the kernel, the N tile and split-K, hence the summation
order: a changed entry changes the model's bits."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def table():
    spec = importlib.util.spec_from_file_location("make_plan_golden", GOLDEN / "make_plan_golden.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(GOLDEN / "gemm_plan.npz")
    want = tuple(want[k] for k in ("rc", "kernel", "split", "ws_bytes"))
    got = gen.evaluate()
    return gen, want, got


def test_plan_table_matches_golden(table):
    gen, want, got = table
    assert len(got[1]) == len(want[1]), f"the grid has {len(got[1])} descriptors, the table {len(want[1])}"
    bad = np.zeros(len(want[1]), bool)
    for w, g in zip(want, got):
        bad |= w != g
    if bad.any():
        first = set(np.flatnonzero(bad)[:8].tolist())
        lines = []
        for i, d in enumerate(gen.grid()):
            if i in first:
                lines.append(f"#{i} {gen.describe(d)}: rc {want[0][i]} -> {got[0][i]}, kernel {want[1][i]} -> "
                             f"{got[1][i]}, split {want[2][i]} -> {got[2][i]}, ws_bytes {want[3][i]} -> {got[3][i]}")
                if len(lines) == len(first):
                    break
        pytest.fail(f"{int(bad.sum())} of {len(bad)} plan decisions differ from tests/golden/gemm_plan.npz; "
                    "the first:\n" + "\n".join(lines))


def test_plan_grid_reaches_every_kernel_and_split(table):
    """A thinned grid cannot pass silently: every kernel id, and a split > 1 on each kernel that
    splits K."""
    _, want, got = table
    for kernel, split in (want[1:3], got[1:3]):
        assert set(kernel.tolist()) == {0, 1, 2, 3, 5, 6, 8, 9}
        for ver in (2, 3, 5, 6):
            assert (split[kernel == ver] > 1).any(), f"no split > 1 on v{ver}"
        assert split.min() >= 1 and split.max() == 32
