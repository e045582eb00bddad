"""CPU test of the precision-1 3-D forward / bwd-data conv plans behind tests/test_gpu_conv_f16x3_branches.py.  mphip_debug_conv3d_plan and
mphip_debug_conv3d_k1_plan are host code: they report what the launchers read, so the library answers without a GPU.  Every row of the GPU
file's tables must claim the plan the library reports under the row's switches, with every edge its id names; the plan classes reachable
on a fixed grid of shapes and switches — (kernel, splits > 1, chunks per split > 1, demand-driven, more logical workgroups than one
resident round), and (ks, column tiles per wave) for the 1x1x1 kernel — must be exactly the classes those tables cover, so a planner change
that opens a class, or moves the cases off one, fails here first."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_conv_f16x3_branches as gpu  # noqa: E402

CHANNELS = [16, 32, 48, 96, 192, 384, 400, 768, 784]
# (N, D, H, W), up to 80k voxels: one tile, depth 2 / 4 / 6 / 8, one to three tile columns, odd and even batches on depth 2 (the two-frame
# mode and its batch rule), launches around one resident round, the tile-walk shapes of the GPU file, H or W off the tile, odd depth
VOLUMES = [(1, 2, 8, 8), (1, 4, 8, 8), (2, 2, 8, 8), (3, 2, 8, 8), (4, 2, 8, 8), (5, 2, 8, 16), (3, 2, 8, 16), (3, 4, 16, 8), (2, 4, 8, 8),
           (1, 6, 16, 24), (1, 6, 16, 16), (2, 8, 16, 24), (1, 8, 24, 24), (1, 4, 32, 32), (2, 4, 16, 16), (1, 4, 8, 16), (1, 2, 112, 112),
           (1, 4, 80, 80), (5, 2, 64, 64), (1, 2, 184, 192), (1, 4, 136, 136), (5, 2, 88, 96), (8, 4, 16, 16), (1, 4, 12, 16), (1, 3, 8, 8),
           (1, 4, 8, 20)]
SETTINGS = [({}, False), (gpu.MT, False), (gpu.PP0, False), (gpu.PP2, False), (gpu.WINO_OFF, False), (gpu.D2_OFF, False), ({}, True),
            (gpu._join(gpu.MT, gpu.PP0), False), (gpu._join(gpu.MT, gpu.PP2), False), (gpu._join(gpu.MT, gpu.PP2), True),
            (gpu._join(gpu.MT, gpu.D2_OFF), False)]
K1_VOLUMES = [(1, 2, 8, 64), (3, 2, 8, 64), (1, 1, 1, 65600), (1, 1, 8, 120), (1, 2, 8, 65), (8, 8, 32, 32), (1, 8, 32, 32), (2, 4, 16, 16),
              (1, 1, 1, 64), (16, 1, 8, 8)]


@pytest.fixture(scope="module")
def lib():
    from megaportrait_hack_amd import _lib

    return _lib.load()


def test_gpu_cases_claim_the_plan_the_library_reports(lib, monkeypatch):
    """the claims of the GPU file's tables, every named edge included, checked here without a GPU"""
    rows = gpu.covered_plan_rows()
    assert len(rows) > 100
    for case, roi in rows:
        gpu.set_switches(monkeypatch, case.env)
        gpu.claim_holds(lib, case, roi=roi)
    gpu.set_switches(monkeypatch, {})
    for row in gpu.covered_k1_rows():
        gpu.k1_claim_holds(lib, row)
    for shape in gpu.K1_REFUSED:
        assert lib.mphip_conv3d_supported(*shape, 1, 1) == 0 and gpu.k1_plan(lib, shape) == (0, (0, 0, 0, 0, 0))
    # the demand-driven rows plan the kernel the full launch of their shape takes, except the two-frame shape
    for case, _ in gpu.ROI_CASES:
        gpu.set_switches(monkeypatch, case.env)
        assert gpu.conv3d_plan(lib, case.shape, False, case.half)[1][0] == case.kernel
    full, demand = gpu.ROI_TWO_FRAME
    assert full.shape == demand.shape and full.env == demand.env and full.kernel == gpu.TWO and demand.kernel == gpu.D2


def test_the_tables_hold_what_the_issue_of_each_section_needs(lib):
    """one case per kernel where a section promises one; tile-walk cases walk; split cases of every family keep several chunks per split"""
    kernels = set(range(6))
    assert {c.kernel for c in gpu.FWD_CASES} == kernels and {c.kernel for c in gpu.GN_CASES} == kernels
    assert {c.kernel for c, _ in gpu.GNIN_CASES} == kernels and {c.kernel for c in gpu.BWD_CASES} == kernels
    assert {c.kernel for k, c in gpu.ROUNDING_CASES if k == 3} == kernels
    assert {c.kernel for c, _ in gpu.ROI_CASES} == kernels - {gpu.TWO}
    assert {c.kernel for c in gpu.WALK_CASES} == kernels and all("walk" in c.edges for c in gpu.WALK_CASES)
    assert {c.kernel for c in gpu.FWD_CASES if c.splits > 1 and c.cps > 1} == kernels
    assert {c.kernel for c in gpu.BWD_CASES if c.splits > 1} >= {gpu.D2, gpu.D4, gpu.ROLE, gpu.TWO}
    assert all(c.shape[1] != c.shape[2] for c in gpu.BWD_CASES) and all(s[1] != s[2] for s, _ in gpu.K1_CASES)
    assert {c.half for c in gpu.FWD_CASES} == {False, True}
    assert {c[1][:2] for k, c in gpu.ROUNDING_CASES if k == 1} == {(8, 2), (4, 2), (1, 1), (1, 2)}
    lists = {nm for _, names in gpu.ROI_CASES for nm in names}
    assert lists == {"tile-edges", "corner+volume", "empty+straddle", "frames3", "volume"}


def _sweep(lib, monkeypatch):
    """(shape, roi, half, plan) of every precision-1 3x3x3 launch of the grid"""
    for env, half in SETTINGS:
        gpu.set_switches(monkeypatch, env)
        for ci in CHANNELS:
            for co in CHANNELS:
                for n, d, h, w in VOLUMES:
                    shape = (n, ci, co, d, h, w)
                    for roi in (False, True):
                        ok, plan = gpu.conv3d_plan(lib, shape, roi, half)
                        supported = lib.mphip_conv3d_supported(*shape, 3, 1)
                        assert ok == supported == int(ci % 16 == 0 and co % 96 == 0 and d % 2 == 0 and h % 8 == 0 and w % 8 == 0), (shape, env)
                        if ok:
                            yield shape, roi, half, plan
                        else:
                            assert plan == (0,) * 12


def test_reachable_plan_classes_are_exactly_the_covered_ones(lib, monkeypatch):
    reachable = {}
    for shape, roi, half, plan in _sweep(lib, monkeypatch):
        n, ci, co, d, h, w = shape
        kern, sp, cps = plan[0], plan[7], plan[8]
        assert plan[9:12] == (plan[9], co // 96, sp) and sp * cps >= ci // 16 > (sp - 1) * cps, (shape, plan)
        assert not (roi and kern == gpu.TWO) and (kern != gpu.TWO or d == 2)
        assert (plan[5] == 1) == (kern != gpu.TWO)
        reachable.setdefault(gpu.plan_class(plan, roi), shape)
    covered = {}
    for case, roi in gpu.covered_plan_rows():
        gpu.set_switches(monkeypatch, case.env)
        covered.setdefault(gpu.plan_class(gpu.conv3d_plan(lib, case.shape, roi, case.half)[1], roi), gpu.case_id(case))
    assert len(reachable) >= 40
    missing = {c: s for c, s in reachable.items() if c not in covered}
    assert not missing, f"plan classes (kernel, split, chunks > 1, roi, walk) the grid reaches and no GPU case covers: {missing}"
    unreachable = {c: s for c, s in covered.items() if c not in reachable}
    assert not unreachable, f"plan classes a GPU case covers that the grid does not reach: {unreachable}"


def test_reachable_1x1x1_geometries_are_exactly_the_covered_ones(lib, monkeypatch):
    gpu.set_switches(monkeypatch, {})
    reachable = set()
    for ci in CHANNELS:
        for co in CHANNELS:
            for n, d, h, w in K1_VOLUMES:
                shape = (n, ci, co, d, h, w)
                ok, plan = gpu.k1_plan(lib, shape)
                supported = lib.mphip_conv3d_supported(*shape, 1, 1)
                assert ok == supported == int(ci % 16 == 0 and co % 96 == 0 and (d * h * w) % 64 == 0 and n * d * h * w >= 1024), shape
                if not ok:
                    assert plan == (0, 0, 0, 0, 0)
                    continue
                ks, nt, gx, gy, block = plan
                waves = n * d * h * w // 64
                assert gy == co // 96 and block == (64 * ks if ks > 1 else 256)
                assert gx == (waves if ks > 1 else -(-waves * (2 if nt == 1 else 1) // 4)), (shape, plan)
                reachable.add((ks, nt))
    covered = {row[1][:2] for row in gpu.covered_k1_rows()}
    assert reachable == covered == {(8, 2), (4, 2), (1, 1), (1, 2)}, (reachable, covered)


def test_k1_query_follows_the_per_call_switches(lib, monkeypatch):
    gpu.set_switches(monkeypatch, {"MPHIP_F16X3_K1_KS": "4"})
    assert gpu.k1_plan(lib, (1, 16, 96, 2, 8, 64)) == (1, (4, 2, 16, 1, 256))
    gpu.set_switches(monkeypatch, {"MPHIP_F16X3_K1_MIN": "512"})
    assert gpu.k1_plan(lib, (1, 16, 96, 1, 8, 120)) == (1, (1, 1, 8, 1, 256))          # 960 voxels: 15 wave tiles, 30 half tiles on 8 workgroups
    gpu.set_switches(monkeypatch, {})
    assert gpu.k1_plan(lib, (1, 16, 96, 1, 8, 120))[0] == 0


def test_k1_query_refuses_bad_shapes(lib, monkeypatch):
    gpu.set_switches(monkeypatch, {})
    out = (ctypes.c_int * 5)(7, 7, 7, 7, 7)
    good = (1, 16, 96, 2, 8, 64)
    assert lib.mphip_debug_conv3d_k1_plan(*good, out) == 1 and list(out) == [1, 1, 8, 1, 256]
    bad = [(0, 16, 96, 2, 8, 64), (1, 0, 96, 2, 8, 64), (1, 16, 0, 2, 8, 64), (1, 16, 96, 0, 8, 64), (1, 16, 96, 2, -8, 64), (1, 16, 96, 2, 8, 0),
           (1, 16, 96, 2, 8, 65),      # D*H*W % 64 != 0
           (1, 16, 96, 1, 8, 120),     # below the voxel minimum
           (1, 24, 96, 2, 8, 64), (1, 16, 100, 2, 8, 64)]
    for shape in bad:
        for i in range(5):
            out[i] = 7
        assert lib.mphip_debug_conv3d_k1_plan(*shape, out) == 0 and list(out) == [0] * 5, shape
    assert lib.mphip_debug_conv3d_k1_plan(*good, None) == 0
    # a 3x3x3 launch is not this query's: the 3x3x3 plan answers for it, and the 1x1x1 geometry says nothing about k = 3
    plan3 = (ctypes.c_int * 12)()
    assert lib.mphip_debug_conv3d_plan(1, 16, 96, 2, 8, 8, 0, plan3) == 1 and lib.mphip_debug_conv3d_k1_plan(1, 16, 96, 2, 8, 8, out) == 0
