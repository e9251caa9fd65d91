"""The attention plan, pinned on the CPU against the commit before the attention source was split:
tests/golden/attention_plan.npz holds, for every case of make_attention_plan_golden.py's grid, what
that commit's launch_flash / launch_flash_causal / launch_flash_tail / attention_entry decided
(written from the generator's Python restatement of those rules, not from the library), and
vd_attention_plan (host-only, no launch) must reproduce it entry for entry: return code, kernel
family, QBLK, unit-scale instance, workgroup count and flash40's exact-pass workgroup count."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def table():
    spec = importlib.util.spec_from_file_location("make_attention_plan_golden",
                                                  GOLDEN / "make_attention_plan_golden.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(GOLDEN / "attention_plan.npz")
    want = tuple(want[k] for k in gen.FIELDS)
    return gen, want, gen.evaluate(), list(gen.grid())


def test_plan_table_matches_golden(table):
    gen, want, got, cases = table
    assert len(got[0]) == len(want[0]) == len(cases), f"the grid has {len(cases)} cases, the table {len(want[0])}"
    bad = np.zeros(len(want[0]), bool)
    for w, g in zip(want, got):
        bad |= w != g
    if bad.any():
        lines = []
        for i in np.flatnonzero(bad)[:8].tolist():
            lines.append(f"#{i} {gen.describe(cases[i])}: " + ", ".join(
                f"{name} {w[i]} -> {g[i]}" for name, w, g in zip(gen.FIELDS, want, got)))
        pytest.fail(f"{int(bad.sum())} of {len(bad)} plan decisions differ from tests/golden/attention_plan.npz; "
                    "the first:\n" + "\n".join(lines))


def test_restatement_still_writes_the_table(table):
    """The committed table is what the generator's restatement of the parent's rules gives."""
    gen, want, _, _ = table
    for name, w, t in zip(gen.FIELDS, want, gen.table()):
        assert np.array_equal(w, t), f"{name}: attention_plan.npz is not what make_attention_plan_golden.py writes"


def test_plan_grid_reaches_every_decision(table):
    """A thinned grid cannot pass silently: the table and the library's answers each hold every
    family, both QBLKs, both unit-scale values on the three kernels that have the instance, an
    exact-pass grid, both refusals, and each way a forced kernel falls through."""
    gen, want, got, cases = table
    d, skv, o, ldo, out_f32, word = (np.asarray([c[j] for c in cases]) for j in (0, 2, 6, 7, 8, 9))
    forced, untouched = word & 0xFF, (word >> 8) == 0  # no causal, no tail
    ldo_al = ldo % np.where(out_f32 == 1, 4, 8) == 0
    for rc, family, qblk, unit, grid, exact in (want, got):
        ok = rc == gen.OK
        assert set(family[ok].tolist()) == {gen.FLASH, gen.FLASH32, gen.FLASH40, gen.FLASH80, gen.FLASH512}
        assert set(qblk[family == gen.FLASH].tolist()) == {2, 4} and not qblk[family != gen.FLASH].any()
        for fam in (gen.FLASH32, gen.FLASH40, gen.FLASH80):
            assert set(unit[family == fam].tolist()) == {0, 1}, f"family {fam}: one unit-scale value only"
        assert (exact[family == gen.FLASH40] > 0).all() and not exact[family != gen.FLASH40].any()
        assert set(rc.tolist()) == {gen.OK, gen.EINVAL, gen.EUNSUPPORTED}
        assert (grid[ok] > 0).all() and (grid[ok] > 0x7FFFFFFF).any() and not grid[~ok].any()
        # the fall-throughs of a forced kernel
        f40, f80 = ok & untouched & (forced == 3) & (d == 40), ok & untouched & (forced == 3) & (d == 80)
        assert (family[f40 & (skv == 64) & (o % 16 == 0) & ldo_al] == gen.FLASH32).all() and (f40 & (skv == 64)).any()
        assert (family[f40 & ~ldo_al] == gen.FLASH).all() and (f40 & ~ldo_al & (skv >= 128)).any()
        f32 = ok & untouched & (forced == 2) & (d == 40) & (o % 16 == 8)
        assert (family[f32] == gen.FLASH).all() and f32.any()
        assert (family[f80 & (skv == 64)] == gen.FLASH).all() and (f80 & (skv == 64)).any()
        # and the forced kernels do run where they take the shape
        assert (family[f40 & (skv >= 128) & (o % 16 == 0) & ldo_al] == gen.FLASH40).all()
        assert (family[f80 & (skv >= 128) & (o % 16 == 0) & ldo_al] == gen.FLASH80).all()
