"""CPU test of the f16x3 backward-weight plan.  mphip_debug_conv3d_bwd_weight_f16x3_plan is host code: it reports what
bwd_weight_f16x3_launch reads (one function), so the library answers without a GPU.  The query is swept over a grid and must agree
with the support and workspace queries; the edge classes of the plan — several tiles per split, an uneven last split, a split that
crosses a sample boundary, each kernel's ragged channel blocks — must be reachable on the grid and each claimed by a bit-exact case of
tests/test_gpu_bwd_weight_f16x3_branches.py, so a planner change that moves those cases off an edge fails here."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_bwd_weight_f16x3_branches as gpu  # noqa: E402

CHANNELS = [1, 5, 32, 33, 40, 96, 97, 100, 130, 200, 480]
# (N, D, H, W): below / above the tiny-volume rule, W % 8 != 0, D*H*W % 128 != 0, odd D, ragged H, one to four tile columns, batched
VOLUMES = [(1, 1, 1, 1), (4, 4, 1, 1), (2, 1, 3, 3), (1, 1, 8, 8), (3, 1, 3, 8), (1, 2, 8, 8), (2, 2, 8, 16), (2, 3, 8, 8), (2, 3, 12, 12),
           (2, 3, 12, 16), (2, 3, 12, 20), (1, 5, 20, 24), (2, 1, 17, 24), (2, 3, 9, 32), (1, 13, 8, 16), (3, 5, 8, 16), (2, 3, 8, 16),
           (1, 1, 1, 72), (1, 4, 16, 16), (2, 8, 32, 32), (1, 16, 64, 64), (5, 3, 24, 40)]
# edge class -> (k it belongs to, edge name in the GPU file)
EDGE_CLASSES = [(k, e) for k in (3, 1) for e in ("tps>1", "uneven-last", "cross-sample", "co%96")] + [(3, "ci%32"), (1, "ci%96")]
TILED_F32 = 3     # mphip_debug_conv3d_bwd_weight_f32_kernel: every other kernel id is a tiny-volume kernel, which serves both precisions


@pytest.fixture(scope="module")
def lib():
    from megaportrait_hack_amd import _lib

    return _lib.load()


def _sweep():
    for k in (3, 1):
        for ci in CHANNELS:
            for co in CHANNELS:
                for n, d, h, w in VOLUMES:
                    yield k, (n, ci, co, d, h, w)


def test_plan_agrees_with_support_and_workspace_queries(lib):
    seen = {0: 0, gpu.CONV3: 0, gpu.CONV1: 0}
    f32 = (ctypes.c_int * 2)()
    for k, shape in _sweep():
        n, ci, co, d, h, w = shape
        kern, splits, tps, ntiles = plan = gpu.f16x3_plan(lib, shape, k)
        seen[kern] += 1
        supported = lib.mphip_conv3d_bwd_weight_supported(*shape, k, 1)
        ws = lib.mphip_conv3d_bwd_weight_workspace_bytes(*shape, k, 1)
        assert lib.mphip_debug_conv3d_bwd_weight_f32_kernel(*shape, k, 1, f32) == 1
        tiny = f32[0] != TILED_F32
        assert supported == int(w % 8 == 0 if k == 3 else (d * h * w) % 128 == 0), (k, shape)
        if not supported:
            assert plan == (0, 0, 0, 0) and ws == 0, (k, shape, plan, ws)
        elif tiny:
            assert plan == (0, 0, 0, 0) and ws == 16, (k, shape, plan, ws)
        else:
            assert kern == (gpu.CONV3 if k == 3 else gpu.CONV1), (k, shape, plan)
            assert ntiles == (n * ((d + 1) // 2) * ((h + 7) // 8) * (w // 8) if k == 3 else n * (d * h * w // 128)), (k, shape, plan)
            assert splits >= 1 and tps >= 1 and splits * tps >= ntiles > (splits - 1) * tps, (k, shape, plan)
            assert ws == gpu.RANGE_HEAD + splits * co * ci * k ** 3 * 4, (k, shape, plan, ws)
    assert all(v > 100 for v in seen.values()), seen


def test_bad_arguments(lib):
    out = (ctypes.c_int * 4)(7, 7, 7, 7)
    for bad in ((0, 8, 8, 4, 8, 8), (1, 0, 8, 4, 8, 8), (1, 8, -1, 4, 8, 8), (1, 8, 8, 0, 8, 8), (1, 8, 8, 4, 0, 8), (1, 8, 8, 4, 8, 0)):
        assert lib.mphip_debug_conv3d_bwd_weight_f16x3_plan(*bad, 3, out) == 0 and list(out) == [0, 0, 0, 0]
    assert lib.mphip_debug_conv3d_bwd_weight_f16x3_plan(1, 8, 8, 4, 8, 8, 2, out) == 0
    assert lib.mphip_debug_conv3d_bwd_weight_f16x3_plan(1, 8, 8, 4, 8, 8, 3, None) == 0


def test_gpu_cases_claim_the_plan_the_library_reports(lib):
    """the claims of the GPU file's tables, checked here without a GPU"""
    for row in gpu.INT_CASES + gpu.ROUNDING_CASES + [r[:3] for r in gpu.ROI_CASES] + [gpu.ROI_K1_CASE[:3]] + \
            [(k, s, c) for k, (s, c) in gpu.MAGNITUDE_SHAPES.items()]:
        gpu.claim_holds(lib, row)
    for k, shape in gpu.OUTSIDE_CASES:
        assert gpu.f16x3_plan(lib, shape, k) == (0, 0, 0, 0)
    assert gpu.f16x3_plan(lib, (2, 40, 72, 3, 12, 20), 3) == (0, 0, 0, 0)       # test_gpu_backward.py's "ragged" row: W = 20
    n, ci, co, d, h, w = gpu.BWD_DATA_SHAPE
    assert lib.mphip_conv3d_kernel_variant(n, co, ci, d, h, w, 3, 1) == 1


@pytest.mark.parametrize("k,edge", EDGE_CLASSES, ids=[f"k{k}-{e}" for k, e in EDGE_CLASSES])
def test_edge_class_is_reachable_and_claimed_by_a_gpu_case(lib, k, edge):
    reachable = [shape for kk, shape in _sweep() if kk == k and (plan := gpu.f16x3_plan(lib, shape, k))[0] and gpu.edge_holds(edge, k, shape, plan)]
    assert reachable, f"no shape of the grid reaches {edge} with k = {k}"
    claimed = [row for row in gpu.INT_CASES if row[0] == k and edge in row[3]]
    assert claimed, f"no bit-exact GPU case claims {edge} with k = {k}"
    for row in claimed:
        assert gpu.edge_holds(edge, k, row[1], gpu.f16x3_plan(lib, row[1], k)), gpu.case_id(row)
