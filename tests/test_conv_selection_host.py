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


# ---------------------------------------------------------------------------------------------------------------------------------
# The exact-fp32 kernels (precision 0).  tests/test_gpu_conv_f32_branches.py runs one bit-exact case per kernel instantiation; here the
# library's own planner (mphip_debug_conv3d_f32_plan, mphip_debug_conv3d_bwd_weight_f32_kernel: host code) is swept over a fixed grid and
# every instantiation it can reach must have a case there.  A planner change that opens a new one fails here, without a GPU.
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_conv_f32_branches as f32  # noqa: E402

F32_CHANNELS = [1, 3, 5, 8, 16, 17, 24, 32, 40, 48, 50, 64, 96, 100, 128, 192, 256, 384, 512]
# (N, D, H, W), up to 16384 voxels: 1x1x1, Dx1x1, depth-2, ragged, tile-aligned, batched
F32_VOLUMES = [(1, 1, 1, 1), (1, 4, 1, 1), (1, 7, 1, 1), (1, 2, 2, 2), (1, 1, 8, 8), (1, 2, 8, 8), (1, 2, 16, 16), (1, 2, 32, 32), (2, 2, 32, 32),
               (1, 3, 5, 7), (2, 3, 5, 7), (1, 5, 9, 11), (2, 5, 9, 11), (1, 6, 20, 36), (1, 8, 2, 32), (1, 4, 4, 4), (1, 4, 8, 8), (2, 4, 8, 8),
               (1, 6, 8, 8), (1, 6, 16, 16), (1, 8, 8, 8), (1, 8, 16, 16), (1, 16, 16, 16), (1, 16, 24, 24), (1, 8, 32, 32), (1, 16, 32, 32)]
F32_REQUIRED_EDGES = {"odd-ci", "co%32", "ragged-vox", "straddle", "idle-waves", "k1-partial", "1x1x1", "dx1x1", "offset-x", "uneven-split",
                      "co-grid-2", "n2"}


@pytest.fixture(scope="module")
def lib():
    from megaportrait_hack_amd import _lib

    return _lib.load()


def _gather_env(monkeypatch, forced):
    if forced:
        monkeypatch.setenv("MPHIP_CONV_GATHER", "1")
    else:
        monkeypatch.delenv("MPHIP_CONV_GATHER", raising=False)


def test_f32_forward_cases_cover_every_reachable_instantiation(lib, monkeypatch):
    reachable = set()
    for forced in (False, True):
        _gather_env(monkeypatch, forced)
        for k in (1, 3):
            for ci in F32_CHANNELS:
                for co in F32_CHANNELS:
                    for n, d, h, w in F32_VOLUMES:
                        tiled, mt, nt, wco, skip, splits, per_split, gx, gy, gz = f32.f32_plan(lib, (n, ci, co, d, h, w), k)
                        assert not (forced and tiled) and splits == gz >= 1 and per_split >= 1 and gx >= 1 and gy >= 1
                        reachable.add((tiled, k, mt, nt, wco, skip))
    covered = {f32.instantiation(row) for row in f32.FWD_CASES}
    assert reachable - covered == set(), f"reachable fp32 conv instantiations without a GPU case: {sorted(reachable - covered)}"
    assert covered - reachable == set(), f"cases whose instantiation the sweep does not reach (widen the grid): {sorted(covered - reachable)}"
    # every gather instantiation the dispatch can name: KS=3 x MT 1-4 x NT 1-2 x WCO 1,2,4 x SKIP, KS=1 x MT 1-4 x WCO 1,2,4; both tiled kernels
    assert len(reachable) == 48 + 12 + 2


def test_f32_case_tables_claim_what_the_library_plans(lib, monkeypatch):
    """every row of the GPU file's tables, checked against the planner without a GPU: the plan, the edges its id names, both sides of
    split-K per family, and the edge list the suite is meant to hold"""
    ids = [f32.case_id(r) for r in f32.FWD_CASES]
    assert len(set(ids)) == len(ids)
    for row in f32.FWD_CASES + f32.BWD_DATA_CASES:
        _gather_env(monkeypatch, row[2])
        f32._claim_holds(lib, row)
    for family in (f32.GATHER_CASES, f32.TILED_CASES):
        assert {row[3][5] > 1 for row in family} == {False, True}
    assert {row[3][5] for row in f32.TILED_CASES} >= {1, 2, 4} and {row[3][0] for row in f32.TILED_CASES} == {2, 4}
    assert F32_REQUIRED_EDGES <= {e for row in f32.FWD_CASES for e in row[4]}
    assert any(row[3][1] > 1 for row in f32.BWD_DATA_CASES) and {row[3][0] for row in f32.BWD_DATA_CASES} == {0, 2, 4}
    monkeypatch.delenv("MPHIP_CONV_GATHER", raising=False)
    for shape, k, claimed in f32.ROUNDING_FWD:
        assert f32.f32_plan(lib, shape, k)[:6] == claimed


def test_f32_bwd_weight_cases_cover_every_kernel(lib, monkeypatch):
    reachable = set()
    for wave in (False, True):
        if wave:
            monkeypatch.setenv("MPHIP_BWD_WEIGHT_WAVE", "1")
        else:
            monkeypatch.delenv("MPHIP_BWD_WEIGHT_WAVE", raising=False)
        for k in (1, 3):
            for aligned in (True, False):
                for ci, co in ((1, 1), (8, 12), (40, 100), (64, 96), (512, 256)):
                    for n, d, h, w in F32_VOLUMES:
                        kern, splits = f32.bwd_weight_kernel(lib, (n, ci, co, d, h, w), k, aligned)
                        assert 0 <= kern <= 3 and splits >= 1 and (kern == f32.TILED or splits == 1) and not (wave and kern == f32.SMALL_MFMA)
                        reachable.add((kern, k))
    monkeypatch.delenv("MPHIP_BWD_WEIGHT_WAVE", raising=False)
    covered = set()
    for row in f32.BWD_WEIGHT_CASES:
        shape, k, aligned, kern, splits = row
        assert f32.bwd_weight_kernel(lib, shape, k, aligned) == (kern, splits), f32.bwd_weight_id(row)
        covered.add((kern, k))
    assert reachable == covered == {(kern, k) for kern in range(4) for k in (1, 3)}
    assert any(not row[2] for row in f32.BWD_WEIGHT_CASES) and any(row[3] == f32.TILED and row[0][0] == 2 for row in f32.BWD_WEIGHT_CASES)


def test_f32_plan_queries_refuse_bad_shapes(lib):
    import ctypes

    out10, out2 = (ctypes.c_int * 10)(*([7] * 10)), (ctypes.c_int * 2)(7, 7)
    for bad in ((0, 8, 8, 4, 4, 4, 3), (1, 8, 8, 4, 4, 4, 2), (1, 8, 8, 4, 4, 0, 1), (1, 1 << 20, 8, 8, 8, 8, 3)):   # the last: x of 2 GiB
        assert lib.mphip_debug_conv3d_f32_plan(*bad, out10) == 0 and list(out10) == [0] * 10
        out10[:] = [7] * 10
    for bad in ((0, 8, 8, 4, 4, 4, 3), (1, 8, 8, 4, 4, 4, 2), (1, 8, 0, 4, 4, 4, 1)):
        assert lib.mphip_debug_conv3d_bwd_weight_f32_kernel(*bad, 1, out2) == 0 and list(out2) == [0, 0]
        out2[:] = [7, 7]
    assert lib.mphip_debug_conv3d_f32_plan(1, 8, 8, 4, 4, 4, 3, None) == 0
    assert lib.mphip_debug_conv3d_bwd_weight_f32_kernel(1, 8, 8, 4, 4, 4, 3, 1, None) == 0
    # the split count the plan reports is the one the public query and the workspace size are built on
    for shape, k in (((1, 128, 128, 8, 16, 16), 3), ((1, 100, 96, 4, 8, 16), 3), ((2, 255, 255, 3, 8, 11), 1)):
        n, ci, co, d, h, w = shape
        splits = f32.f32_plan(lib, shape, k)[5]
        assert splits > 1 and lib.mphip_conv3d_splits(*shape, k, 0) == splits
        assert lib.mphip_conv3d_workspace_bytes(*shape, k, 0) == splits * n * co * d * h * w * 4
