"""Every instantiation of the exact-fp32 conv kernels (precision 0: csrc/conv3d.hip forward and bwd-data, csrc/backward.hip bwd-weight),
bit for bit on integer data.

The fp32 path takes every shape the f16x3 kernels refuse, is the fallback of ops.conv3d, and is the yardstick the f16x3 tests are
measured against.  Its host dispatch picks between 62 kernel instantiations plus split-K; each case here names the one it reaches and
first asserts that the library (mphip_debug_conv3d_f32_plan / mphip_debug_conv3d_bwd_weight_f32_kernel: the launcher's own decision)
reports exactly that, so a planner change cannot silently move a case to another kernel.  tests/test_conv_selection_host.py sweeps the
planner on the CPU and fails when it can reach an instantiation that has no case in the tables below.

Why no tolerance: x, dy in [-4, 4], w in [-3, 3], bias in [-8, 8] are integers, so every product and every partial sum of a conv is an
integer of magnitude <= Ci * k^3 * 4 * 3 + 8 (bwd-weight: N * D * H * W * 4 * 4) < 2^24: exactly representable in fp32 whatever the
summation order, split-K factor or reduce.  The float64 reference is then THE answer and the kernels must be torch.equal to it; a wrong,
missing or doubled term cannot hide.  Each case asserts that bound, and that ATen's own fp32 CPU conv equals the float64 one, before it
touches the GPU.  Rounding behaviour, about which integer data says nothing, keeps four Gaussian cases under the elementwise bound of
tests/test_gpu_aux_kernels.py: |err| <= (terms + 2) * 2^-24 * sum |products|.

Edges a case id names (each is asserted from the reported plan, `_edge_holds`): odd-ci (CiP = Ci + 1), co%32, ragged-vox (voxels no
multiple of NT * 32), straddle (N >= 2 and D*H*W % 32 != 0: a 32-voxel tile spans two samples), idle-waves (the last block along x has
waves without voxels), k1-partial (k = 1, channels per split no multiple of the 16-channel pipeline stage), 1x1x1 / dx1x1 (26 / 24 of
the 27 taps are padding), offset-x (the input starts 4 bytes past a 16-byte boundary), uneven-split (tiled kernel: the last split has
fewer chunks), co-grid-2, n2.

Run time of this file on an MI355X: not recorded yet (no GPU run of it has been made; its float64 references take 2 s in all on
a 16-core CPU, the largest case is 1.9 GMAC)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXACT = 2 ** 24

# (launch shape (N, Ci, Co, D, H, W), k, MPHIP_CONV_GATHER set, claimed (tiled, MT, NT, WCO, skip, splits), edges)
# One row per (k, MT, NT, WCO, skip) the planner can reach, each the cheapest shape found for it (all <= 1.9 GMAC), then the extra edges.
GATHER_CASES = [
    ((2, 15, 1, 1, 1, 1), 1, False, (0, 1, 1, 1, 0, 2), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves', 'k1-partial')),
    ((2, 15, 33, 1, 1, 1), 1, False, (0, 1, 1, 2, 0, 2), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves', 'k1-partial')),
    ((2, 15, 100, 1, 1, 1), 1, False, (0, 1, 1, 4, 0, 2), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'k1-partial')),
    ((1, 1, 100, 16, 32, 32), 1, False, (0, 2, 1, 1, 0, 1), ('odd-ci', 'co%32', 'k1-partial')),
    ((1, 1, 384, 16, 32, 11), 1, False, (0, 2, 1, 2, 0, 1), ('odd-ci', 'k1-partial')),
    ((2, 1, 512, 3, 20, 36), 1, False, (0, 2, 1, 4, 0, 1), ('odd-ci', 'straddle', 'k1-partial')),
    ((2, 1, 384, 6, 20, 36), 1, False, (0, 3, 1, 1, 0, 1), ('odd-ci', 'idle-waves', 'k1-partial')),
    ((2, 255, 192, 3, 8, 11), 1, False, (0, 3, 1, 2, 0, 32), ('odd-ci', 'ragged-vox', 'straddle', 'idle-waves', 'k1-partial')),
    ((2, 255, 384, 2, 20, 3), 1, False, (0, 3, 1, 4, 0, 32), ('odd-ci', 'ragged-vox', 'straddle', 'k1-partial')),
    ((1, 1, 255, 16, 32, 32), 1, False, (0, 4, 1, 1, 0, 1), ('odd-ci', 'co%32', 'k1-partial')),
    ((2, 255, 255, 3, 8, 11), 1, False, (0, 4, 1, 2, 0, 32), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves', 'k1-partial')),
    ((2, 255, 512, 2, 20, 3), 1, False, (0, 4, 1, 4, 0, 32), ('odd-ci', 'ragged-vox', 'straddle', 'k1-partial')),
    ((2, 15, 1, 3, 3, 3), 3, False, (0, 1, 1, 1, 0, 2), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves')),
    ((2, 15, 1, 1, 1, 1), 3, False, (0, 1, 1, 1, 1, 2), ('1x1x1', 'odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves')),
    ((2, 15, 33, 4, 3, 3), 3, False, (0, 1, 1, 2, 0, 2), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves')),
    ((2, 15, 33, 1, 1, 1), 3, False, (0, 1, 1, 2, 1, 2), ('1x1x1', 'odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves')),
    ((2, 1, 100, 3, 3, 3), 3, False, (0, 1, 1, 4, 0, 1), ('odd-ci', 'co%32', 'ragged-vox', 'straddle')),
    ((2, 15, 100, 1, 1, 1), 3, False, (0, 1, 1, 4, 1, 2), ('1x1x1', 'odd-ci', 'co%32', 'ragged-vox', 'straddle')),
    ((2, 1, 1, 5, 20, 36), 3, False, (0, 1, 2, 1, 0, 1), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves')),
    ((2, 15, 1, 2, 32, 32), 3, False, (0, 1, 2, 1, 1, 2), ('odd-ci', 'co%32')),
    ((2, 1, 33, 3, 20, 36), 3, False, (0, 1, 2, 2, 0, 1), ('odd-ci', 'co%32', 'ragged-vox', 'straddle')),
    ((2, 1, 33, 2, 32, 32), 3, False, (0, 1, 2, 2, 1, 1), ('odd-ci', 'co%32')),
    ((2, 1, 100, 3, 20, 36), 3, False, (0, 1, 2, 4, 0, 1), ('odd-ci', 'co%32', 'ragged-vox', 'straddle')),
    ((2, 1, 100, 2, 32, 32), 3, False, (0, 1, 2, 4, 1, 1), ('odd-ci', 'co%32')),
    ((2, 255, 33, 3, 5, 36), 3, False, (0, 2, 1, 1, 0, 32), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves')),
    ((1, 127, 33, 2, 32, 32), 3, False, (0, 2, 1, 1, 1, 16), ('odd-ci', 'co%32')),
    ((2, 255, 100, 3, 8, 11), 3, False, (0, 2, 1, 2, 0, 32), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves')),
    ((2, 255, 100, 2, 20, 7), 3, False, (0, 2, 1, 2, 1, 32), ('odd-ci', 'co%32', 'ragged-vox', 'straddle')),
    ((2, 255, 512, 6, 3, 3), 3, False, (0, 2, 1, 4, 0, 32), ('odd-ci', 'ragged-vox', 'straddle')),
    ((2, 255, 512, 5, 5, 2), 3, False, (0, 2, 1, 4, 1, 32), ('odd-ci', 'ragged-vox', 'straddle')),
    ((1, 1, 255, 16, 32, 32), 3, False, (0, 2, 2, 1, 0, 1), ('odd-ci', 'co%32')),
    ((2, 127, 33, 2, 32, 32), 3, False, (0, 2, 2, 1, 1, 16), ('odd-ci', 'co%32')),
    ((2, 1, 384, 16, 32, 11), 3, False, (0, 2, 2, 2, 0, 1), ('odd-ci',)),
    ((2, 63, 100, 2, 32, 32), 3, False, (0, 2, 2, 2, 1, 8), ('odd-ci', 'co%32')),
    ((1, 1, 512, 8, 32, 32), 3, False, (0, 2, 2, 4, 0, 1), ('odd-ci',)),
    ((2, 31, 255, 2, 32, 32), 3, False, (0, 2, 2, 4, 1, 4), ('odd-ci', 'co%32')),
    ((2, 255, 65, 3, 5, 36), 3, False, (0, 3, 1, 1, 0, 32), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves')),
    ((1, 127, 65, 2, 32, 32), 3, False, (0, 3, 1, 1, 1, 16), ('odd-ci', 'co%32')),
    ((2, 255, 192, 3, 8, 11), 3, False, (0, 3, 1, 2, 0, 32), ('odd-ci', 'ragged-vox', 'straddle', 'idle-waves')),
    ((2, 255, 192, 2, 20, 7), 3, False, (0, 3, 1, 2, 1, 32), ('odd-ci', 'ragged-vox', 'straddle')),
    ((2, 255, 384, 3, 5, 8), 3, False, (0, 3, 1, 4, 0, 32), ('odd-ci', 'ragged-vox', 'straddle')),
    ((2, 255, 384, 2, 20, 3), 3, False, (0, 3, 1, 4, 1, 32), ('odd-ci', 'ragged-vox', 'straddle')),
    ((1, 1, 384, 16, 32, 32), 3, False, (0, 3, 2, 1, 0, 1), ('odd-ci',)),
    ((2, 127, 65, 2, 32, 32), 3, False, (0, 3, 2, 1, 1, 16), ('odd-ci', 'co%32')),
    ((2, 63, 192, 3, 20, 36), 3, False, (0, 3, 2, 2, 0, 8), ('odd-ci', 'ragged-vox', 'straddle')),
    ((2, 63, 192, 2, 32, 32), 3, False, (0, 3, 2, 2, 1, 8), ('odd-ci',)),
    ((2, 31, 384, 3, 20, 36), 3, False, (0, 3, 2, 4, 0, 4), ('odd-ci', 'ragged-vox', 'straddle')),
    ((2, 31, 384, 2, 32, 32), 3, False, (0, 3, 2, 4, 1, 4), ('odd-ci',)),
    ((2, 255, 100, 3, 5, 36), 3, False, (0, 4, 1, 1, 0, 32), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves')),
    ((1, 127, 100, 2, 32, 32), 3, False, (0, 4, 1, 1, 1, 16), ('odd-ci', 'co%32')),
    ((2, 255, 255, 3, 8, 11), 3, False, (0, 4, 1, 2, 0, 32), ('odd-ci', 'co%32', 'ragged-vox', 'straddle', 'idle-waves')),
    ((2, 255, 255, 2, 20, 7), 3, False, (0, 4, 1, 2, 1, 32), ('odd-ci', 'co%32', 'ragged-vox', 'straddle')),
    ((2, 255, 512, 3, 5, 8), 3, False, (0, 4, 1, 4, 0, 32), ('odd-ci', 'ragged-vox', 'straddle')),
    ((2, 255, 512, 2, 20, 3), 3, False, (0, 4, 1, 4, 1, 32), ('odd-ci', 'ragged-vox', 'straddle')),
    ((1, 1, 512, 16, 32, 32), 3, False, (0, 4, 2, 1, 0, 1), ('odd-ci',)),
    ((2, 127, 100, 2, 32, 32), 3, False, (0, 4, 2, 1, 1, 16), ('odd-ci', 'co%32')),
    ((2, 63, 255, 3, 20, 36), 3, False, (0, 4, 2, 2, 0, 8), ('odd-ci', 'co%32', 'ragged-vox', 'straddle')),
    ((2, 63, 255, 2, 32, 32), 3, False, (0, 4, 2, 2, 1, 8), ('odd-ci', 'co%32')),
    ((2, 31, 512, 3, 20, 36), 3, False, (0, 4, 2, 4, 0, 4), ('odd-ci', 'ragged-vox', 'straddle')),
    ((2, 31, 512, 2, 32, 32), 3, False, (0, 4, 2, 4, 1, 4), ('odd-ci',)),
    # SKIP with 24 dead taps, an unsplit launch over real channel counts, inputs off 16-byte alignment
    ((2, 15, 100, 5, 1, 1), 3, False, (0, 1, 1, 4, 1, 2), ("dx1x1", "odd-ci", "co%32", "ragged-vox", "straddle")),
    ((1, 7, 40, 5, 9, 11), 3, False, (0, 1, 1, 2, 0, 1), ("odd-ci", "co%32", "ragged-vox", "offset-x")),
    ((1, 5, 128, 16, 32, 32), 1, False, (0, 2, 1, 1, 0, 1), ("odd-ci", "k1-partial", "offset-x")),
    ((1, 128, 128, 8, 16, 16), 3, False, (0, 4, 1, 1, 0, 16), ("offset-x",)),
    # shapes of the tiled kernel, forced onto the gather kernel (MPHIP_CONV_GATHER): the two families must agree on them
    ((1, 128, 96, 8, 16, 16), 3, True, (0, 3, 1, 1, 0, 16), ()),
    ((1, 50, 96, 6, 8, 8), 3, True, (0, 1, 1, 1, 0, 1), ()),
]
TILED_CASES = [
    ((1, 8, 96, 4, 8, 8), 3, False, (4, 3, 2, 1, 0, 1), ()),
    ((1, 8, 96, 2, 8, 8), 3, False, (2, 3, 1, 1, 0, 1), ()),
    ((1, 50, 96, 6, 8, 8), 3, False, (2, 3, 1, 1, 0, 2), ("uneven-split",)),          # D = 6: the (2,8,8) tile; 25 chunks = 13 + 12
    ((1, 100, 96, 4, 8, 16), 3, False, (4, 3, 2, 1, 0, 4), ("uneven-split", "offset-x")),   # 50 chunks = 13 + 13 + 13 + 11
    ((1, 96, 96, 4, 8, 8), 3, False, (4, 3, 2, 1, 0, 4), ()),
    ((2, 48, 192, 4, 8, 8), 3, False, (4, 3, 2, 1, 0, 2), ("co-grid-2", "n2")),
    ((2, 24, 192, 2, 16, 8), 3, False, (2, 3, 1, 1, 0, 1), ("co-grid-2", "n2")),
]
FWD_CASES = GATHER_CASES + TILED_CASES

# bwd-data of a conv (Ci -> Co) is a forward launch (Co -> Ci) on the transposed pack: rows are LAUNCH shapes, i.e. (N, dy channels,
# dx channels, D, H, W); one per family and k, one with MT > 1, odd and ragged channel counts (pack_weight_kernel's transposed indexing)
BWD_DATA_CASES = [
    ((2, 255, 100, 3, 5, 36), 3, False, (0, 4, 1, 1, 0, 32), ("odd-ci", "co%32", "ragged-vox", "straddle", "idle-waves")),
    ((2, 15, 33, 1, 1, 1), 3, False, (0, 1, 1, 2, 1, 2), ("1x1x1", "odd-ci", "co%32")),
    ((2, 255, 192, 3, 8, 11), 1, False, (0, 3, 1, 2, 0, 32), ("odd-ci", "ragged-vox", "straddle", "k1-partial")),
    ((2, 15, 33, 1, 1, 1), 1, False, (0, 1, 1, 2, 0, 2), ("odd-ci", "co%32", "k1-partial")),
    ((1, 100, 96, 4, 8, 16), 3, False, (4, 3, 2, 1, 0, 4), ("uneven-split",)),
    ((1, 50, 96, 6, 8, 8), 3, False, (2, 3, 1, 1, 0, 2), ("uneven-split",)),
]

PER_THREAD, SMALL_MFMA, WAVE, TILED = range(4)    # kernel ids of mphip_debug_conv3d_bwd_weight_f32_kernel
# ((N, Ci, Co, D, H, W), k, dy 16-byte aligned, claimed kernel, claimed splits (None: whatever the planner says, 1 for the small kernels))
BWD_WEIGHT_CASES = [
    ((2, 8, 12, 1, 3, 3), 3, True, PER_THREAD, 1),
    ((2, 8, 12, 1, 3, 3), 1, True, PER_THREAD, 1),
    ((4, 64, 40, 4, 1, 1), 3, True, SMALL_MFMA, 1),
    ((2, 24, 16, 8, 2, 2), 1, True, SMALL_MFMA, 1),
    ((1, 12, 20, 3, 5, 7), 3, True, WAVE, 1),               # 105 voxels: no multiple of 4
    ((1, 12, 20, 3, 5, 7), 1, True, WAVE, 1),
    ((2, 8, 12, 4, 4, 4), 3, False, WAVE, 1),              # dy 4 bytes off alignment: the MFMA kernel's 16-byte loads cannot take it
    ((2, 8, 12, 4, 4, 4), 1, False, WAVE, 1),
    ((1, 32, 96, 4, 16, 16), 3, True, TILED, 2),
    ((1, 32, 96, 4, 16, 16), 1, True, TILED, 2),
    ((1, 40, 100, 6, 20, 36), 3, True, TILED, 8),          # ragged H, W tiles, Ci % 32 != 0, Co = 100: a ragged second 96-row tile
    ((1, 40, 100, 6, 20, 36), 1, True, TILED, 8),
    ((2, 10, 20, 5, 20, 28), 3, True, TILED, 8),           # N = 2 at a ragged size
    ((2, 10, 20, 5, 20, 28), 1, True, TILED, 8),
]
BWD_WEIGHT_NAMES = ("per-thread", "small-mfma", "wave", "tiled")


def case_id(row):
    (n, ci, co, d, h, w), k, gather, (tiled, mt, nt, wco, skip, splits), edges = row
    kern = f"tiled{tiled}" if tiled else "gather"
    return (f"{kern}-k{k}-mt{mt}-nt{nt}-wco{wco}{'-skip' if skip else ''}-s{splits}-{n}x{ci}x{co}@{d}x{h}x{w}{'-forced' if gather else ''}"
            + "".join(f"-{e}" for e in edges))


def bwd_weight_id(row):
    (n, ci, co, d, h, w), k, aligned, kern, splits = row
    return f"{BWD_WEIGHT_NAMES[kern]}-k{k}-s{splits}-{n}x{ci}x{co}@{d}x{h}x{w}{'' if aligned else '-offset-dy'}"


def instantiation(row):
    """(tiled, KS, MT, NT, WCO, SKIP): the kernel template a forward row claims"""
    _, k, _, (tiled, mt, nt, wco, skip, _), _ = row
    return (tiled, k, mt, nt, wco, skip)


def f32_plan(lib, shape, k):
    out = (ctypes.c_int * 10)()
    assert lib.mphip_debug_conv3d_f32_plan(*shape, k, out) == 1
    return tuple(out)


def bwd_weight_kernel(lib, shape, k, aligned):
    out = (ctypes.c_int * 2)()
    assert lib.mphip_debug_conv3d_bwd_weight_f32_kernel(*shape, k, int(aligned), out) == 1
    return tuple(out)


def _edge_holds(edge, shape, k, plan):
    n, ci, co, d, h, w = shape
    tiled, mt, nt, wco, skip, splits, per_split, gx, gy, gz = plan
    m = n * d * h * w
    vox_tiles = -(-m // (nt * 32))
    if edge == "odd-ci":
        return ci % 2 == 1
    if edge == "co%32":
        return co % 32 != 0
    if edge == "ragged-vox":
        return not tiled and m % (nt * 32) != 0
    if edge == "straddle":
        return not tiled and n >= 2 and (d * h * w) % 32 != 0
    if edge == "idle-waves":
        return not tiled and vox_tiles % (4 // wco) != 0
    if edge == "k1-partial":
        return not tiled and k == 1 and per_split % 16 != 0
    if edge == "1x1x1":
        return k == 3 and skip == 1 and (d, h, w) == (1, 1, 1)
    if edge == "dx1x1":
        return k == 3 and skip == 1 and d >= 3 and (h, w) == (1, 1)
    if edge == "uneven-split":
        return tiled and splits > 1 and (ci // 2) % splits != 0 and per_split * (splits - 1) < ci // 2 < per_split * splits
    if edge == "co-grid-2":
        return gy == 2
    if edge == "n2":
        return n == 2
    return edge == "offset-x"


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from megaportrait_hack_amd import _lib, ops

    _lib.load()
    return ops


@pytest.fixture(scope="module")
def lib():
    from megaportrait_hack_amd import _lib

    return _lib.load()


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _offset_view(t, dev):
    """A contiguous device copy of `t` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _set_gather(monkeypatch, gather):
    if gather:
        monkeypatch.setenv("MPHIP_CONV_GATHER", "1")
    else:
        monkeypatch.delenv("MPHIP_CONV_GATHER", raising=False)


def _claim_holds(lib, row):
    """the library reports the plan the row claims, and every edge its id names"""
    shape, k, _, claimed, edges = row
    plan = f32_plan(lib, shape, k)
    assert plan[:6] == claimed, (case_id(row), plan)
    for e in edges:
        assert _edge_holds(e, shape, k, plan), (case_id(row), e, plan)
    return plan


def _check_bound(name, got, truth, bound):
    """elementwise |got - truth| <= bound (float64); prints the worst error / bound ratio"""
    err = (got.detach().cpu().double() - truth).abs()
    assert err.shape == bound.shape, (err.shape, bound.shape)
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, worst err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), (name, ratio)


def _gn_groups(co):
    return next(g for g in (32, 4, 5, 3, 1) if co % g == 0)


@pytest.mark.parametrize("row", FWD_CASES, ids=case_id)
def test_conv3d_f32_forward_bit_exact(ops, lib, dev, monkeypatch, row):
    (n, ci, co, d, h, w), k, gather, claimed, edges = row
    _set_gather(monkeypatch, gather)
    _claim_holds(lib, row)
    assert ci * k ** 3 * 4 * 3 + 8 < EXACT
    gen = torch.Generator().manual_seed(20260 + 7 * FWD_CASES.index(row))
    x, wt, b = _ints((n, ci, d, h, w), -4, 4, gen), _ints((co, ci, k, k, k), -3, 3, gen), _ints((co,), -8, 8, gen)
    plain = F.conv3d(x.double(), wt.double(), None, padding=k // 2)
    want = plain + b.double().view(1, -1, 1, 1, 1)
    assert torch.equal(F.conv3d(x, wt, b, padding=k // 2).double(), want)      # a condition on the inputs: fp32 is exact on them
    assert want.abs().max().item() < EXACT
    want, plain = want.float(), plain.float()

    xd = _offset_view(x, dev) if "offset-x" in edges else x.to(dev)
    pc, pc0 = ops.PackedConv(wt.to(dev), b.to(dev)), ops.PackedConv(wt.to(dev), None)
    y = ops.conv3d(xd, pc, precision=0)
    assert torch.equal(y.cpu(), want)
    assert torch.equal(ops.conv3d(xd, pc0, precision=0).cpu(), plain)
    out = ops.conv3d_split(xd, pc, precision=0)
    assert out.splits in (1, claimed[5])
    if out.splits > 1:     # the slabs, summed here in float64, and the bias the launch left to the consumer
        assert tuple(out.data.shape) == (claimed[5], n, co, d, h, w) and out.bias is not None
        assert torch.equal(out.data.cpu().double().sum(dim=0) + b.double().view(1, -1, 1, 1, 1), want.double())
    else:
        assert torch.equal(out.data.cpu(), want)
    y_gn, stats = ops.conv3d(xd, pc, precision=0, gn_groups=_gn_groups(co))
    assert torch.equal(y_gn, y) and bool(torch.isfinite(stats).all())         # (the statistics themselves: test_gpu_groupnorm_stats.py)


@pytest.mark.parametrize("row", BWD_DATA_CASES, ids=case_id)
def test_conv3d_f32_bwd_data_bit_exact(ops, lib, dev, monkeypatch, row):
    (n, cdy, cdx, d, h, w), k, gather, claimed, edges = row
    _set_gather(monkeypatch, gather)
    _claim_holds(lib, row)
    assert cdy * k ** 3 * 4 * 3 + 8 < EXACT
    gen = torch.Generator().manual_seed(30260 + 7 * BWD_DATA_CASES.index(row))
    dy, wt = _ints((n, cdy, d, h, w), -4, 4, gen), _ints((cdy, cdx, k, k, k), -3, 3, gen)    # wt: the ORIGINAL conv's weight [Co, Ci, k, k, k]
    want = F.conv_transpose3d(dy.double(), wt.double(), None, padding=k // 2)
    assert torch.equal(F.conv_transpose3d(dy, wt, None, padding=k // 2).double(), want)
    dyd = dy.to(dev)
    _, scale = ops.grad_prep(dyd, want_bias=False)
    dx = ops.conv3d_bwd_data(dyd, ops.PackedConv(wt.to(dev), None, transposed=True), scale, precision=0)
    assert torch.equal(dx.cpu(), want.float())


def _dw64(x, dy, co, k):
    wt = torch.zeros(co, x.shape[1], k, k, k, dtype=x.dtype, requires_grad=True)
    F.conv3d(x, wt, None, padding=k // 2).backward(dy)
    return wt.grad


@pytest.mark.parametrize("row", BWD_WEIGHT_CASES, ids=bwd_weight_id)
def test_conv3d_f32_bwd_weight_bit_exact(ops, lib, dev, monkeypatch, row):
    (n, ci, co, d, h, w), k, aligned, kern, splits = row
    monkeypatch.delenv("MPHIP_BWD_WEIGHT_WAVE", raising=False)
    assert bwd_weight_kernel(lib, (n, ci, co, d, h, w), k, aligned) == (kern, splits), bwd_weight_id(row)
    assert n * d * h * w * 4 * 4 < EXACT
    gen = torch.Generator().manual_seed(40260 + 7 * BWD_WEIGHT_CASES.index(row))
    x, dy = _ints((n, ci, d, h, w), -4, 4, gen), _ints((n, co, d, h, w), -4, 4, gen)
    want = _dw64(x.double(), dy.double(), co, k)
    assert torch.equal(_dw64(x, dy, co, k).double(), want)
    dyd = dy.to(dev) if aligned else _offset_view(dy, dev)
    assert (dyd.data_ptr() % 16 == 0) == aligned
    dw = ops.conv3d_bwd_weight(x.to(dev), dyd, k, precision=0)
    assert torch.equal(dw.cpu(), want.float())


def test_bwd_weight_wave_switch_still_selects_the_wave_kernel(ops, lib, dev, monkeypatch):
    """MPHIP_BWD_WEIGHT_WAVE (the A/B switch) moves a small-MFMA shape to the wave kernel, in the report and in the launch's result"""
    shape, k = (2, 24, 16, 8, 2, 2), 3
    monkeypatch.setenv("MPHIP_BWD_WEIGHT_WAVE", "1")
    assert bwd_weight_kernel(lib, shape, k, True) == (WAVE, 1)
    n, ci, co, d, h, w = shape
    gen = torch.Generator().manual_seed(50260)
    x, dy = _ints((n, ci, d, h, w), -4, 4, gen), _ints((n, co, d, h, w), -4, 4, gen)
    want = _dw64(x.double(), dy.double(), co, k)
    assert torch.equal(ops.conv3d_bwd_weight(x.to(dev), dy.to(dev), k, precision=0).cpu(), want.float())
    monkeypatch.delenv("MPHIP_BWD_WEIGHT_WAVE")
    assert bwd_weight_kernel(lib, shape, k, True) == (SMALL_MFMA, 1)
    assert torch.equal(ops.conv3d_bwd_weight(x.to(dev), dy.to(dev), k, precision=0).cpu(), want.float())


# Gaussian data: (launch shape, k, claimed plan) of a gather MT = 4 / NT = 2 launch, a gather k = 1 launch and the tiled kernel with 4 splits
ROUNDING_FWD = [
    ((2, 31, 512, 3, 20, 36), 3, (0, 4, 2, 4, 0, 4)),
    ((2, 255, 255, 3, 8, 11), 1, (0, 4, 1, 2, 0, 32)),
    ((1, 100, 96, 4, 8, 16), 3, (4, 3, 2, 1, 0, 4)),
]


@pytest.mark.parametrize("shape,k,claimed", ROUNDING_FWD, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_conv3d_f32_forward_rounding_bound(ops, lib, dev, monkeypatch, shape, k, claimed):
    """|err| <= (terms + 2) * 2^-24 * (|w| * |x| + |b|) elementwise, terms = Ci * k^3 + 1: every product passes at most terms - 1
    additions in any order (split-K and its reduce included), its own rounding and the bias add.  Worst measured err / bound: not recorded yet."""
    n, ci, co, d, h, w = shape
    monkeypatch.delenv("MPHIP_CONV_GATHER", raising=False)
    assert f32_plan(lib, shape, k)[:6] == claimed
    x, wt, b = R.seeded_tensor((n, ci, d, h, w), 2101, scale=2.0), R.seeded_tensor((co, ci, k, k, k), 2102, scale=0.5), R.seeded_tensor((co,), 2103)
    want = F.conv3d(x.double(), wt.double(), b.double(), padding=k // 2)
    absum = F.conv3d(x.double().abs(), wt.double().abs(), b.double().abs(), padding=k // 2)
    y = ops.conv3d(x.to(dev), ops.PackedConv(wt.to(dev), b.to(dev)), precision=0)
    _check_bound(f"conv3d f32 {shape} k={k}", y, want, (ci * k ** 3 + 1 + 2) * U * absum)


def test_conv3d_f32_bwd_weight_rounding_bound(ops, lib, dev):
    """the tiled bwd-weight kernel at its ragged shape: |err| <= (N*D*H*W + 2) * 2^-24 * sum |dy| |x|.  Worst measured err / bound: not recorded yet."""
    shape, k = (1, 40, 100, 6, 20, 36), 3
    n, ci, co, d, h, w = shape
    assert bwd_weight_kernel(lib, shape, k, True) == (TILED, 8)
    x, dy = R.seeded_tensor((n, ci, d, h, w), 2201, scale=2.0), R.seeded_tensor((n, co, d, h, w), 2202, scale=0.5)
    want = _dw64(x.double(), dy.double(), co, k)
    absum = _dw64(x.double().abs(), dy.double().abs(), co, k)
    dw = ops.conv3d_bwd_weight(x.to(dev), dy.to(dev), k, precision=0)
    _check_bound(f"conv3d_bwd_weight f32 {shape} k={k}", dw, want, (n * d * h * w + 2) * U * absum)
