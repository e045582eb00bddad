"""CPU test of the conv kernel selection: the planner (csrc/conv3d_f16x3_plan.hip) and every size query are host code, so the library
answers without a GPU.  Its answers are compared, row by row and exactly, with tests/golden/conv_selection.json — recorded (by
tools/record_conv_selection.py) from the commit before the choice was moved into one planner, never from the code under test."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_conv_selection as rec  # noqa: E402

TABLE = rec.load(os.path.join(ROOT, "tests", "golden", "conv_selection.json"))
BASE = TABLE["rows"][0]
DIRECT_2, DIRECT_4, LOCKSTEP, ROLE_SPLIT, BIG_TILE, TWO_FRAME = range(6)


def expected(name):
    return TABLE["rows"][list(TABLE["settings"]).index(name)]


def kernels(rows, roi=0):
    found, kern = TABLE["columns"].index(f"plan_roi{roi}.found"), TABLE["columns"].index(f"plan_roi{roi}.kernel")
    return [r[kern] for r in rows if r[found]]


def test_table_is_the_sweep_the_recorder_runs():
    assert TABLE["shapes"] == [list(s) for s in rec.shapes()] and TABLE["columns"] == rec.COLUMNS and TABLE["groups"] == rec.GROUPS
    assert list(TABLE["settings"]) == list(rec.settings())
    for name, (env, half) in rec.settings().items():
        assert TABLE["settings"][name]["env"] == env and TABLE["settings"][name]["half_products"] == half
    assert len(TABLE["rows"]) == len(TABLE["settings"]) and list(TABLE["settings"])[0] == "none"
    assert all(len(per_shape) == len(TABLE["shapes"]) and all(len(r) == len(rec.COLUMNS) for r in per_shape) for per_shape in TABLE["rows"])


def test_table_covers_every_kernel():
    """Every kernel of the choice occurs, and the four defaults occur with no switch set; the F(2,3) A/B schedules answer their switch."""
    default = kernels(BASE)
    assert {DIRECT_2, DIRECT_4, ROLE_SPLIT, TWO_FRAME} == set(default)
    seen = set()
    for name in TABLE["settings"]:
        seen |= set(kernels(expected(name))) | set(kernels(expected(name), roi=1))
    assert seen == {DIRECT_2, DIRECT_4, LOCKSTEP, ROLE_SPLIT, BIG_TILE, TWO_FRAME}
    assert LOCKSTEP in kernels(expected("MPHIP_WINO_PP=0")) and BIG_TILE in kernels(expected("MPHIP_WINO_PP=2"))
    # the big-tile kernel has no one-product arithmetic: under the half-products flag its launches fall back to the role-split kernel
    assert BIG_TILE not in kernels(expected("MPHIP_WINO_PP=2,half_products")) and ROLE_SPLIT in kernels(expected("MPHIP_WINO_PP=2,half_products"))
    assert TWO_FRAME not in kernels(BASE, roi=1)   # demand-driven launches of a depth-2 volume stay on the direct kernel


@pytest.mark.parametrize("name", list(rec.settings()))
def test_library_matches_recorded_selection(name):
    """One fresh child process per setting (some switches are fixed at first use); every row, every column, exactly."""
    got, want = rec.run_setting(name), expected(name)
    assert len(got) == len(want)
    bad = [(TABLE["shapes"][i], {c: (g, w) for c, g, w in zip(rec.COLUMNS, got[i], want[i]) if g != w}) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"{len(bad)} of {len(want)} rows differ under {name!r}; first (shape, column: (library, recorded)): {bad[:3]}"
