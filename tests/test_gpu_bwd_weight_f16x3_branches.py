"""Every branch of the f16x3 backward-weight file (csrc/conv3d_bwd_f16x3.hip: the 3x3x3 kernel, the 1x1x1 kernel, the two slab reduces
and grad_prep), exactly.

Each case first asserts that the library (mphip_debug_conv3d_bwd_weight_f16x3_plan: the launcher's own decision) reports the kernel,
the voxel tiles, the splits and the tiles per split the case claims, that precision 1 is supported, and that every edge its id names holds
for the shape, so a planner change cannot silently move a case onto another path (ops.conv3d_bwd_weight falls back to the exact fp32
kernels without a word where precision 1 does not apply).  tests/test_bwd_weight_f16x3_host.py sweeps the query on the CPU and
requires the edge classes below to be reachable and claimed by a case here.

Why no tolerance (integer cases): x, dy are integers in [-4, 4] and both contain a 4, so both operand scales are 2^11 (max * scale =
2^13, inside [2^13, 2^14); the loose explicit x bound gives 2^2).  Every scaled operand is then an exact f16, every `lo` half is 0, every
product is an integer times 2^22 and every partial sum an integer of magnitude <= N*D*H*W*16 < 2^24 times 2^22: exact in fp32 in any
order, over any split and through the slab reduce.  The float64 gradient is THE answer and the kernels must be torch.equal to it: a
wrong, missing or doubled term of any output element cannot hide behind max|dW|.  Each case asserts the bound, and that ATen's own fp32
CPU gradient equals the float64 one, before it touches the GPU.

Edges a case id names (`edge_holds`): ci%32 / co%96 / ci%96 (ragged channel blocks), ci+1 / co+1 / co-1 (one channel past or short of a
block), odd-d (the second plane of the last 2x8x8 tile is outside the volume), ragged-h, cols2 / cols3 (tile columns along W: with three a
middle tile has both side halos), w8 (no side halo at all), d1h1 (24 of the 27 taps see only padding), co<32 (the heavy waves' co-tiles
lie partly or wholly outside Co), c1 (Ci = Co = 1), vox72 (just above the tiny-volume rule), tps>1 (several tiles per split: the 1x1x1
kernel's prefetch rotation), uneven-last (the last split holds fewer tiles), cross-sample (one split's tiles belong to two samples).

Rounding (Gaussian cases; integer data says nothing about the `lo` planes): the project's rule of tests/test_gpu_conv2d_f16x3.py,
max|got - t64| <= 4 * max|t32 - t64| + 2^-21 * A, t32 = ATen's fp32 CPU gradient, A = max over outputs of sum |dy||x|.  Each case also
shows on the CPU that the bar can fail: a float64 emulation of the one-product contract (operands rounded to f16 at their scales, exact
accumulation) must exceed it 10x, the three-product emulation (hi*hi + hi*lo + lo*hi) must stay under a tenth of it.  err, bar and their
ratio are printed per case; with MPHIP_PARITY_JSON=<file> the worst ratio of every test goes to that file
(profiles/bwd_weight_f16x3_branches.json holds one MI355X run).

Worst err / bar on an MI355X (one run, profiles/bwd_weight_f16x3_branches.json): 0.042 for test_rounding_bar, at (2,130,200,1,17,24)
k = 3 (0.040 and 0.033 at the other two shapes); the half-products case is at 0.0021 of its 1e-4 gate.  The file's 57 cases take 4 s there."""
import ctypes
import functools
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as R

pytestmark = pytest.mark.gpu

EXACT = 2 ** 24
CONV3, CONV1 = 1, 2          # kernel ids of mphip_debug_conv3d_bwd_weight_f16x3_plan (0: precision 1 does not reach the file)
RANGE_HEAD = (4100 * 4 + 255) // 256 * 256

# (k, (N, Ci, Co, D, H, W), claimed (kernel, splits, tiles per split, tiles), edges)
INT_CASES = [
    (3, (2, 40, 100, 3, 12, 16), (CONV3, 16, 1, 16), ("ci%32", "co%96", "odd-d", "ragged-h", "cols2")),
    (3, (1, 130, 200, 5, 20, 24), (CONV3, 14, 2, 27), ("ci%32", "co%96", "odd-d", "ragged-h", "cols3", "tps>1", "uneven-last")),
    (3, (2, 130, 200, 1, 17, 24), (CONV3, 9, 2, 18), ("tps>1", "cross-sample", "odd-d", "ragged-h", "cols3")),
    (3, (1, 33, 97, 2, 8, 8), (CONV3, 1, 1, 1), ("w8", "ci+1", "co+1")),
    (3, (1, 5, 7, 1, 1, 72), (CONV3, 9, 1, 9), ("d1h1", "co<32", "ci%32", "co%96", "cols3")),
    (3, (3, 1, 1, 1, 3, 8), (CONV3, 3, 1, 3), ("c1", "vox72", "w8", "odd-d", "ragged-h")),
    (1, (2, 40, 100, 2, 8, 16), (CONV1, 4, 1, 4), ("ci%96", "co%96")),
    (1, (1, 480, 480, 13, 8, 16), (CONV1, 7, 2, 13), ("tps>1", "uneven-last")),
    (1, (3, 480, 480, 5, 8, 16), (CONV1, 8, 2, 15), ("tps>1", "uneven-last", "cross-sample")),
    (1, (2, 97, 95, 3, 8, 16), (CONV1, 6, 1, 6), ("ci+1", "co-1", "ci%96", "co%96")),
    (1, (1, 1, 1, 2, 8, 8), (CONV1, 1, 1, 1), ("c1",)),
]
# just outside the supported set: precision 1 silently takes the exact fp32 kernels
OUTSIDE_CASES = [
    (3, (2, 40, 100, 3, 12, 12)),    # W = 12
    (1, (2, 40, 100, 3, 8, 8)),      # D*H*W = 192
]
# (k, shape, claimed plan): Gaussian data.  A ragged k = 3, a k = 3 with tps > 1, a k = 1 with tps > 1.
ROUNDING_CASES = [
    (3, (2, 40, 100, 3, 12, 16), (CONV3, 16, 1, 16)),
    (3, (2, 130, 200, 1, 17, 24), (CONV3, 9, 2, 18)),
    (1, (1, 480, 480, 13, 8, 16), (CONV1, 7, 2, 13)),
]
# 128-voxel integer cases of each kernel for the magnitude sweep
MAGNITUDE_SHAPES = {3: ((1, 33, 97, 2, 8, 8), (CONV3, 1, 1, 1)), 1: ((1, 40, 100, 2, 8, 8), (CONV1, 1, 1, 1))}
MAGNITUDE_EXPONENTS = (-126, -118, -116, -60, 0, 60, 97, 99, 112)
# dy is zero outside one box {lx, ly, lz, ex, ey, ez} per frame.  Per shape: box lists that between them hold a box that ends exactly on
# a tile edge in each axis (and one that starts on one), a one-voxel box in the far corner, a box covering the volume, a frame whose
# box has zero extent, and a box that straddles tile edges.
ROI_CASES = [
    (3, (2, 40, 100, 3, 12, 16), (CONV3, 16, 1, 16), {
        "tile-edges": [(0, 0, 0, 8, 8, 2), (8, 8, 2, 8, 4, 1)],
        "corner-voxel+volume": [(15, 11, 2, 1, 1, 1), (0, 0, 0, 16, 12, 3)],
        "empty+straddle": [(5, 3, 1, 0, 4, 2), (6, 5, 1, 4, 6, 2)],
    }),
    (3, (2, 130, 200, 1, 17, 24), (CONV3, 9, 2, 18), {
        "tile-edges": [(8, 8, 0, 8, 8, 1), (16, 16, 0, 8, 1, 1)],
        "corner-voxel+volume": [(23, 16, 0, 1, 1, 1), (0, 0, 0, 24, 17, 1)],
        "empty+straddle": [(4, 4, 0, 3, 0, 1), (6, 7, 0, 12, 3, 1)],
    }),
]
ROI_K1_CASE = (1, (2, 40, 100, 2, 8, 16), (CONV1, 4, 1, 4), [(3, 2, 0, 6, 4, 1), (0, 0, 1, 16, 8, 1)])
# grad_prep alone: (N, C, S) -> what the size reaches
GRAD_PREP_CASES = [
    ((2, 3, 9), "scalar loop"),
    ((1, 2, 8196), "vector loop, a second chunk of 4 floats"),
    ((1, 2, 8193), "scalar loop, a second chunk of 1 float"),
    ((1, 1, 24580), "four chunks, S % 4 == 0, ragged last chunk"),
    ((2, 300, 16), "a second finalize block (C > 256), two samples"),
]
BWD_DATA_SHAPE = (1, 96, 96, 2, 8, 8)     # a conv (Ci -> Co) whose bwd-data launch is the direct f16x3 kernel


def case_id(row):
    k, (n, ci, co, d, h, w), (kern, splits, tps, ntiles), *rest = row
    edges = rest[0] if rest and isinstance(rest[0], tuple) else ()
    return f"k{k}-{n}x{ci}x{co}@{d}x{h}x{w}-t{ntiles}-s{splits}-tps{tps}" + "".join(f"-{e}" for e in edges)


def f16x3_plan(lib, shape, k):
    out = (ctypes.c_int * 4)()
    assert lib.mphip_debug_conv3d_bwd_weight_f16x3_plan(*shape, k, out) == 1
    return tuple(out)


def splits_of_tiles(plan):
    """[(first tile, end tile)] per split, from the reported plan"""
    _, splits, tps, ntiles = plan
    return [(s * tps, min(ntiles, (s + 1) * tps)) for s in range(splits)]


def edge_holds(edge, k, shape, plan):
    n, ci, co, d, h, w = shape
    kern, splits, tps, ntiles = plan
    cib = 32 if k == 3 else 96
    if edge == "ci%32":
        return k == 3 and ci % 32 != 0
    if edge == "ci%96":
        return k == 1 and ci % 96 != 0
    if edge == "co%96":
        return co % 96 != 0
    if edge == "ci+1":
        return ci % cib == 1 and ci > cib
    if edge == "co+1":
        return co % 96 == 1 and co > 96
    if edge == "co-1":
        return co % 96 == 95
    if edge == "odd-d":
        return k == 3 and d % 2 == 1
    if edge == "ragged-h":
        return k == 3 and h % 8 != 0
    if edge == "cols2":
        return k == 3 and w // 8 == 2
    if edge == "cols3":
        return k == 3 and w // 8 >= 3
    if edge == "w8":
        return k == 3 and w == 8
    if edge == "d1h1":
        return k == 3 and d == 1 and h == 1
    if edge == "co<32":
        return k == 3 and co < 32
    if edge == "c1":
        return ci == 1 and co == 1
    if edge == "vox72":
        return n * d * h * w == 72
    if edge == "tps>1":
        return tps > 1
    if edge == "uneven-last":
        return splits > 1 and 0 < ntiles - (splits - 1) * tps < tps
    if edge == "cross-sample":
        per_sample = ntiles // n
        return n > 1 and ntiles == n * per_sample and any(b // per_sample != (e - 1) // per_sample for b, e in splits_of_tiles(plan))
    raise AssertionError(f"unknown edge {edge}")


def claim_holds(lib, row):
    """the library reports the plan the row claims, precision 1 is supported, and every edge the id names holds"""
    k, shape, claimed, *rest = row
    plan = f16x3_plan(lib, shape, k)
    assert plan == claimed, (case_id(row), plan)
    assert lib.mphip_conv3d_bwd_weight_supported(*shape, k, 1) == 1
    assert plan[1] * plan[2] >= plan[3] > (plan[1] - 1) * plan[2]
    for e in (rest[0] if rest and isinstance(rest[0], tuple) else ()):
        assert edge_holds(e, k, shape, plan), (case_id(row), e, plan)
    return plan


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


# ---------------------------------------------------------------------------------------------------------------- references
def dw_ref(x, dy, k):
    """dW[co][ci][tap] = sum_{n,v} dy[n][co][v] * x[n][ci][v + tap] (zero padding), one float64 matrix product per tap"""
    x, dy = x.double(), dy.double()
    n, ci, d, h, w = x.shape
    co = dy.shape[1]
    a = dy.transpose(0, 1).reshape(co, -1)
    if k == 1:
        return (a @ x.transpose(0, 1).reshape(ci, -1).t()).view(co, ci, 1, 1, 1)
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    out = torch.empty(co, ci, 3, 3, 3, dtype=torch.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                b = xp[:, :, kd:kd + d, kh:kh + h, kw:kw + w].transpose(0, 1).reshape(ci, -1)
                out[:, :, kd, kh, kw] = a @ b.t()
    return out


def dw_aten32(x, dy, k):
    """ATen's own fp32 CPU gradient (autograd of F.conv3d)"""
    wt = torch.zeros(dy.shape[1], x.shape[1], k, k, k, dtype=torch.float32, requires_grad=True)
    F.conv3d(x.float(), wt, None, padding=k // 2).backward(dy.float())
    return wt.grad


def _ints(shape, gen):
    t = torch.randint(-4, 5, shape, generator=gen).float()
    t.view(-1)[0] = 4.0      # the maximum is 4 whatever the draw: the operand scale is 2^11
    return t


@functools.lru_cache(maxsize=None)
def int_case(k, shape, seed):
    """(x, dy, float64 dW) of an integer case, computed once and left unchanged; asserts that fp32 is exact on it"""
    n, ci, co, d, h, w = shape
    assert n * d * h * w * 16 < EXACT
    gen = torch.Generator().manual_seed(seed)
    x, dy = _ints((n, ci, d, h, w), gen), _ints((n, co, d, h, w), gen)
    assert x.abs().max().item() == 4 and dy.abs().max().item() == 4
    want = dw_ref(x, dy, k)
    assert torch.equal(dw_aten32(x, dy, k).double(), want)      # a condition on the inputs: ATen's fp32 gradient is exact on them
    assert want.abs().max().item() < EXACT
    return x, dy, want


def _offset_view(t, dev):
    """A contiguous device copy of `t` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _loose_range(ops, x, dev):
    """{0, 0, 1000 * max|x|, 0}: derive mode, no partial maxima, a rigorous but loose bound"""
    rng = torch.zeros(4100, dtype=torch.float32)
    rng[2] = 1000.0 * x.abs().max().item()
    return rng.to(dev)


_RECORD = {}


def _note(test, case, ratio):
    """worst err / bar per test; rewritten on every call when MPHIP_PARITY_JSON names a file"""
    cur = _RECORD.setdefault(test, {"worst_err_over_bar": -1.0, "at": None, "checks": 0})
    cur["checks"] += 1
    if ratio > cur["worst_err_over_bar"]:
        cur["worst_err_over_bar"], cur["at"] = float(f"{ratio:.4g}"), case
    out = os.environ.get("MPHIP_PARITY_JSON")
    if out:
        with open(out, "w") as f:
            json.dump({"what": "tests/test_gpu_bwd_weight_f16x3_branches.py: worst max|got - t64| / bar per test (test_rounding_bar: bar = 4 * "
                               "max|t32 - t64| + 2^-21 * max sum |dy||x|; test_half_products_keep_the_autocast_contract: bar = 1e-4 * max|dW|), "
                               "and the case it occurred at", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
                       "tests": _RECORD}, f, indent=1)
            f.write("\n")


# ---------------------------------------------------------------------------------------------------------------- a. integer cases
@pytest.mark.parametrize("row", INT_CASES, ids=case_id)
def test_bwd_weight_f16x3_bit_exact(ops, lib, dev, row):
    k, shape, claimed, edges = row
    claim_holds(lib, row)
    x, dy, want = int_case(k, shape, 60260 + 7 * INT_CASES.index(row))
    want = want.float()
    xd, dyd = x.to(dev), dy.to(dev)
    assert xd.data_ptr() % 16 == 0 and dyd.data_ptr() % 16 == 0 and ops.tensor_range(xd) is None
    db, scale = ops.grad_prep(dyd)
    assert scale.cpu().tolist()[:3] == [2.0 ** 11, 2.0 ** -11, 4.0]
    assert torch.equal(db.cpu().double(), dy.double().sum(dim=(0, 2, 3, 4)))
    first = ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1)              # x_range left to the library
    assert torch.equal(first.cpu(), want), "precision 1, library-measured x range"
    if k == 3:
        with ops.half_products(True):                                          # the <true> instantiation: every lo half is 0, same bits
            half = ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1)
        assert torch.equal(half.cpu(), want), "half products"
    assert torch.equal(ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1), first), "second launch"
    assert ops.tensor_range(xd) is None
    loose = ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1, x_range=_loose_range(ops, x, dev))
    assert torch.equal(loose.cpu(), want), "explicit loose x bound"
    measured = ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1, x_range=ops.absmax_range(xd))
    assert torch.equal(measured.cpu(), want), "x range of absmax_range"


@pytest.mark.parametrize("k,shape", OUTSIDE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_outside_the_supported_set_precision_1_is_the_fp32_kernel(ops, lib, dev, k, shape):
    assert f16x3_plan(lib, shape, k) == (0, 0, 0, 0)
    x, dy, want = int_case(k, shape, 61260 + k)
    xd, dyd = x.to(dev), dy.to(dev)
    _, scale = ops.grad_prep(dyd, want_bias=False)
    exact = ops.conv3d_bwd_weight(xd, dyd, k, precision=0)
    assert torch.equal(exact.cpu(), want.float())
    assert torch.equal(ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1), exact)


def test_the_ragged_row_of_test_conv3d_bwd_weight_never_reaches_this_file(lib):
    """tests/test_gpu_backward.py::test_conv3d_bwd_weight's (2,40,72,3,12,20) row has W = 20: both of its precisions run the fp32 kernel"""
    assert f16x3_plan(lib, (2, 40, 72, 3, 12, 20), 3) == (0, 0, 0, 0)
    assert lib.mphip_conv3d_bwd_weight_supported(2, 40, 72, 3, 12, 20, 3, 1) == 0


def test_dy_off_16_byte_alignment_takes_the_exact_kernels(ops, lib, dev):
    """dy 4 bytes past a 16-byte boundary: the f16x3 kernels' 16-byte loads cannot take it.  grad_prep reads it with its scalar loop,
    ops.conv3d_bwd_weight uses precision 0; dW and dbias stay exact."""
    k, shape = 3, (2, 40, 100, 3, 12, 16)
    assert f16x3_plan(lib, shape, k)[0] == CONV3
    x, dy, want = int_case(k, shape, 60260)
    xd, dyd = x.to(dev), _offset_view(dy, dev)
    db, scale = ops.grad_prep(dyd)
    assert scale.cpu().tolist()[:3] == [2.0 ** 11, 2.0 ** -11, 4.0]
    assert torch.equal(db.cpu().double(), dy.double().sum(dim=(0, 2, 3, 4)))
    assert torch.equal(ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1).cpu(), want.float())
    assert torch.equal(ops.conv3d_bwd_weight(_offset_view(x, dev), dy.to(dev), k, scale, precision=1).cpu(), want.float())


# ---------------------------------------------------------------------------------------------------------------- b. ROI cases
def _tile_boxes(k, shape):
    """[(sample, (w0, w1), (h0, h1), (d0, d1))] of the 3x3x3 kernel's (2,8,8) voxel tiles, in launch order, clipped to the volume"""
    n, _, _, d, h, w = shape
    assert k == 3
    return [(i, (tw * 8, tw * 8 + 8), (th * 8, min(h, th * 8 + 8)), (td * 2, min(d, td * 2 + 2)))
            for i in range(n) for td in range((d + 1) // 2) for th in range((h + 7) // 8) for tw in range(w // 8)]


def _roi_dy(shape, boxes, gen):
    n, _, co, d, h, w = shape
    full = torch.randint(-4, 5, (n, co, d, h, w), generator=gen).float()
    dy = torch.zeros_like(full)
    for i, (lx, ly, lz, ex, ey, ez) in enumerate(boxes):
        assert 0 <= lx and lx + ex <= w and 0 <= ly and ly + ey <= h and 0 <= lz and lz + ez <= d
        dy[i, :, lz:lz + ez, ly:ly + ey, lx:lx + ex] = full[i, :, lz:lz + ez, ly:ly + ey, lx:lx + ex]
    dy[-1].view(-1)[dy[-1].view(-1).nonzero()[0]] = 4.0     # (every list's last frame has a box with voxels) the maximum is 4
    return dy


ROI_PARAMS = [(k, shape, claimed, name) for k, shape, claimed, lists in ROI_CASES for name in lists]


@pytest.mark.parametrize("k,shape,claimed,name", ROI_PARAMS, ids=[f"{case_id((k, s, c))}-{nm}" for k, s, c, nm in ROI_PARAMS])
def test_roi_hint_equals_float64_and_the_unhinted_launch(ops, lib, dev, k, shape, claimed, name):
    plan = claim_holds(lib, (k, shape, claimed))
    boxes = dict((s, l) for _, s, _, l in ROI_CASES)[shape][name]
    n, ci, co, d, h, w = shape
    # the list contains what its name says
    if name == "tile-edges":
        assert any((lx + ex) % 8 == 0 and lx + ex < w and (ly + ey) % 8 == 0 and ly + ey < h for lx, ly, lz, ex, ey, ez in boxes)
        assert any(lx % 8 == 0 and lx > 0 and ly % 8 == 0 and ly > 0 for lx, ly, lz, ex, ey, ez in boxes)
        assert d == 1 or (any((b[2] + b[5]) % 2 == 0 and b[2] + b[5] < d for b in boxes) and any(b[2] % 2 == 0 and b[2] > 0 for b in boxes))
    elif name == "corner-voxel+volume":
        assert boxes[0] == (w - 1, h - 1, d - 1, 1, 1, 1) and boxes[1] == (0, 0, 0, w, h, d)
    else:
        assert 0 in boxes[0][3:] and all(e > 0 for e in boxes[1][3:])
        lx, ly, lz, ex, ey, ez = boxes[1]
        assert lx // 8 != (lx + ex - 1) // 8 and lx % 8 != 0 and (lx + ex) % 8 != 0
    # tiles the geometry says hold no voxel of their frame's box; every list but the whole-volume one leaves some split with nothing to do
    def empty(t):
        i, (w0, w1), (h0, h1), (d0, d1) = t
        lx, ly, lz, ex, ey, ez = boxes[i]
        return min(w1, lx + ex) <= max(w0, lx) or min(h1, ly + ey) <= max(h0, ly) or min(d1, lz + ez) <= max(d0, lz)
    tiles = _tile_boxes(k, shape)
    assert len(tiles) == plan[3]
    idle = [all(empty(t) for t in tiles[b:e]) for b, e in splits_of_tiles(plan)]
    assert any(idle) and not all(idle), idle

    gen = torch.Generator().manual_seed(70260 + 13 * ROI_PARAMS.index((k, shape, claimed, name)))
    x, dy = _ints((n, ci, d, h, w), gen), _roi_dy(shape, boxes, gen)
    assert n * d * h * w * 16 < EXACT and dy.abs().max().item() == 4
    want = dw_ref(x, dy, k)
    assert torch.equal(dw_aten32(x, dy, k).double(), want)
    xd, dyd = x.to(dev), dy.to(dev)
    roi = torch.tensor([list(b) + [0, 0] for b in boxes], dtype=torch.int32).to(dev)
    _, scale = ops.grad_prep(dyd, want_bias=False)
    plain = ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1)
    hinted = ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1, roi=roi)
    assert torch.equal(plain.cpu(), want.float())
    assert torch.equal(hinted.cpu(), want.float())
    assert torch.equal(hinted, plain)
    with ops.half_products(True):
        assert torch.equal(ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1, roi=roi), plain)


def test_roi_hint_is_ignored_by_the_1x1x1_kernel(ops, lib, dev):
    k, shape, claimed, boxes = ROI_K1_CASE
    claim_holds(lib, (k, shape, claimed))
    n, ci, co, d, h, w = shape
    gen = torch.Generator().manual_seed(71260)
    x, dy = _ints((n, ci, d, h, w), gen), _roi_dy(shape, boxes, gen)
    want = dw_ref(x, dy, k)
    xd, dyd = x.to(dev), dy.to(dev)
    roi = torch.tensor([list(b) + [0, 0] for b in boxes], dtype=torch.int32).to(dev)
    _, scale = ops.grad_prep(dyd, want_bias=False)
    plain = ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1)
    assert torch.equal(plain.cpu(), want.float())
    assert torch.equal(ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1, roi=roi), plain)


# ---------------------------------------------------------------------------------------------------------------- c. magnitudes
@pytest.mark.parametrize("p", MAGNITUDE_EXPONENTS, ids=lambda p: f"2^{p}")
@pytest.mark.parametrize("k", [3, 1], ids=["k3", "k1"])
def test_gradient_magnitude_sweep_is_exact(ops, lib, dev, k, p):
    """dy = integers * 2^p: the result is the integer gradient times 2^p bit for bit, from max|dy| = 2^-124 to 2^114.  Before grad_prep
    took the activations' scale rule (exponent clamped to +-120, every finite maximum accepted), p <= -117 gave scale = Inf, 1/scale = 0
    and p >= 98 (max|dy| >= 1e30) gave scale 1 (every |dy| > 65504 overflowed the f16 cast): predicted from the code, then observed on
    an MI355X with the commit before the fix, where both kernels returned NaN in every element of dW at p = -126, -118, -117, 98, 99, 112
    and the exact result at p = -116, -60, 0, 60, 97."""
    shape, claimed = MAGNITUDE_SHAPES[k]
    claim_holds(lib, (k, shape, claimed))
    x, dy, truth = int_case(k, shape, 62260 + k)
    two_p = 2.0 ** p
    want = truth * two_p                                    # exact in float64
    want32 = want.float()
    assert bool(torch.isfinite(want32).all()) and torch.equal(want32.double(), want)
    assert want32[want32 != 0].abs().min().item() >= 2.0 ** -126          # every nonzero element is a normal fp32
    dyp = (dy.double() * two_p).float()
    assert torch.equal(dyp.double(), dy.double() * two_p) and dyp.abs().max().item() == 4 * two_p
    dyd = dyp.to(dev)
    db, scale = ops.grad_prep(dyd)
    s0, s1, s2 = scale.cpu().tolist()[:3]
    assert s2 == 4 * two_p
    assert math.isfinite(s0) and math.isfinite(s1) and s0 > 0 and s1 > 0
    assert math.frexp(s0)[0] == 0.5 and math.frexp(s1)[0] == 0.5 and s0 * s1 == 1.0
    assert torch.equal(db.cpu().double(), dy.double().sum(dim=(0, 2, 3, 4)) * two_p)
    dw = ops.conv3d_bwd_weight(x.to(dev), dyd, k, scale, precision=1)
    assert torch.equal(dw.cpu(), want32)


@functools.lru_cache(maxsize=None)
def _bwd_data_case():
    n, ci, co, d, h, w = BWD_DATA_SHAPE
    x = R.seeded_tensor((n, ci, d, h, w), 21).double().requires_grad_(True)     # the data of test_gpu_backward.py::test_conv3d_bwd_data
    dy = R.seeded_tensor((n, co, d, h, w), 22)
    wt = R.seeded_tensor((co, ci, 3, 3, 3), 23, scale=0.05)
    F.conv3d(x, wt.double(), None, padding=1).backward(dy.double())
    return dy, wt, x.grad


@pytest.mark.parametrize("p", [-118, 99], ids=lambda p: f"2^{p}")
def test_conv3d_bwd_data_keeps_its_bar_at_extreme_gradient_magnitudes(ops, lib, dev, p):
    """the direct f16x3 forward kernel on the gradient's own scale: dx finite and within 2e-5 of max|dx| (test_conv3d_bwd_data's bar)"""
    n, ci, co, d, h, w = BWD_DATA_SHAPE
    assert lib.mphip_conv3d_kernel_variant(n, co, ci, d, h, w, 3, 1) == 1
    dy, wt, dx1 = _bwd_data_case()
    two_p = 2.0 ** p
    want = dx1 * two_p
    assert bool(torch.isfinite(want.float()).all()) and want.abs().max().item() > 2.0 ** -120     # far from the end of the normal range
    dyd = (dy.double() * two_p).float().to(dev)
    _, scale = ops.grad_prep(dyd, want_bias=False)
    dx = ops.conv3d_bwd_data(dyd, ops.PackedConv(wt.to(dev), None, transposed=True), scale, precision=1)
    assert bool(torch.isfinite(dx).all())
    err = (dx.cpu().double() - want).abs().max().item() / want.abs().max().item()
    print(f"conv3d_bwd_data at dy * 2^{p}: {err:.2e} of max|dx| (bar 2e-5)")
    assert err < 2e-5, err


# ---------------------------------------------------------------------------------------------------------------- d. rounding
def _split_f16(t):
    """(hi, lo) of t at its power-of-two operand scale, unscaled, float64: what the three-product kernels multiply"""
    s = R.pow2_operand_scale(t.abs().max().item(), 14)
    v = t.float() * s
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi.double() / s, lo.double() / s


@functools.lru_cache(maxsize=None)
def rounding_case(k, shape):
    """Gaussian-class seeded data, its float64 gradient, the bar, and the CPU evidence that the bar separates one product from three"""
    n, ci, co, d, h, w = shape
    x, dy = R.seeded_tensor((n, ci, d, h, w), 2301, scale=1.5), R.seeded_tensor((n, co, d, h, w), 2302)
    t64 = dw_ref(x, dy, k)
    e32 = (dw_aten32(x, dy, k).double() - t64).abs().max().item()
    A = dw_ref(x.abs(), dy.abs(), k).max().item()
    bar = 4 * e32 + 2.0 ** -21 * A
    xh, xl = _split_f16(x)
    dh, dl = _split_f16(dy)
    one = dw_ref(xh, dh, k)
    three = one + dw_ref(xl, dh, k) + dw_ref(xh, dl, k)
    assert torch.equal(xh, R.round_f16_at_scale(x)) and torch.equal(dh, R.round_f16_at_scale(dy))
    e1, e3 = (one - t64).abs().max().item(), (three - t64).abs().max().item()
    return x, dy, t64, one, bar, e1, e3


@pytest.mark.parametrize("row", ROUNDING_CASES, ids=case_id)
def test_rounding_bar(ops, lib, dev, row):
    """max|got - t64| <= 4 * max|t32 - t64| + 2^-21 * A on Gaussian-class data; the bar can fail: the one-product contract, emulated in
    float64, misses it by more than 10x, the three-product one keeps a tenth of it (no wrong kernel is involved)."""
    k, shape, claimed = row
    claim_holds(lib, row)
    x, dy, t64, _, bar, e1, e3 = rounding_case(k, shape)
    print(f"{case_id(row)}: CPU emulation, one product {e1 / bar:.1f} x bar, three products {e3 / bar:.4f} x bar")
    assert e1 >= 10 * bar, (e1, bar)
    assert e3 <= 0.1 * bar, (e3, bar)
    xd, dyd = x.to(dev), dy.to(dev)
    _, scale = ops.grad_prep(dyd, want_bias=False)
    dw = ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1)
    err = (dw.cpu().double() - t64).abs().max().item()
    print(f"{case_id(row)}: err {err:.3e}, bar {bar:.3e}, err / bar {err / bar:.4f}")
    _note("test_rounding_bar", case_id(row), err / bar)
    assert err <= bar, (err, bar)


def test_half_products_keep_the_autocast_contract_at_the_ragged_shape(ops, lib, dev):
    """ops.half_products(True) -> conv_bwd_weight_f16x3_kernel<true> at ragged channels, odd D, ragged H: 1e-4 of max|dW| against the
    f16-operand reference (the existing bar of test_conv3d_bwd_weight_half_products_follow_the_autocast_contract)"""
    row = ROUNDING_CASES[0]
    k, shape, claimed = row
    plan = claim_holds(lib, row)
    for e in ("ci%32", "co%96", "odd-d", "ragged-h"):
        assert edge_holds(e, k, shape, plan)
    x, dy, t64, one, bar, _, _ = rounding_case(k, shape)
    xd, dyd = x.to(dev), dy.to(dev)
    _, scale = ops.grad_prep(dyd, want_bias=False)
    with ops.half_products(True):
        half = ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1)
    full = ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1)
    top = one.abs().max().item()
    err = (half.cpu().double() - one).abs().max().item() / top
    print(f"{case_id(row)}: half products vs the f16-operand contract {err:.2e} of max|dW| (gate 1e-4), err / gate {err / 1e-4:.4f}")
    _note("test_half_products_keep_the_autocast_contract_at_the_ragged_shape", case_id(row), err / 1e-4)
    assert err < 1e-4, err
    assert not torch.equal(half, full)
    assert (full.cpu().double() - t64).abs().max().item() <= bar


# ---------------------------------------------------------------------------------------------------------------- e. grad_prep alone
@pytest.mark.parametrize("ncs,what", GRAD_PREP_CASES, ids=[f"{n}x{c}x{s}" for (n, c, s), _ in GRAD_PREP_CASES])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset-dy"])
def test_grad_prep_is_exact_on_integers(ops, dev, ncs, what, aligned):
    """dbias = sum dy and scale[2] = max|dy| exactly, over one and several 8192-float chunks, both loops, both finalize blocks, and with dy
    4 bytes past a 16-byte boundary (the scalar loop whatever S)"""
    n, c, s = ncs
    assert n * s * 4 < EXACT
    gen = torch.Generator().manual_seed(80260 + s)
    dy = torch.randint(-4, 5, (n, c, s), generator=gen).float()
    dy[0, 0, 0] = 1.0
    dy[-1, -1, -1] = -4.0            # the maximum sits in the last element of the last chunk of the last plane
    assert dy.abs().max().item() == 4
    dyd = dy.to(dev) if aligned else _offset_view(dy, dev)
    db, scale = ops.grad_prep(dyd)
    assert torch.equal(db.cpu().double(), dy.double().sum(dim=(0, 2)))
    assert scale.cpu().tolist()[:3] == [2.0 ** 11, 2.0 ** -11, 4.0]
    none, scale2 = ops.grad_prep(dyd, want_bias=False)
    assert none is None and torch.equal(scale2[:3], scale[:3])


def test_grad_prep_of_an_all_zero_gradient(ops, lib, dev):
    """scale 1, and dW exactly 0 from both kernels"""
    for k, (shape, claimed) in MAGNITUDE_SHAPES.items():
        claim_holds(lib, (k, shape, claimed))
        x, _, _ = int_case(k, shape, 62260 + k)
        n, ci, co, d, h, w = shape
        dyd = torch.zeros((n, co, d, h, w), device=dev)
        db, scale = ops.grad_prep(dyd)
        assert scale.cpu().tolist()[:3] == [1.0, 1.0, 0.0] and not bool(db.any())
        dw = ops.conv3d_bwd_weight(x.to(dev), dyd, k, scale, precision=1)
        assert tuple(dw.shape) == (co, ci, k, k, k) and not bool(dw.any())
