"""The backward of the 2-D 3x3 conv on the matrix cores (csrc/conv2d_bwd_f16x3.hip, ops.conv2d_bwd_weight / conv2d_bwd_data,
ag.Conv2dFn), after tests/test_gpu_bwd_weight_f16x3_branches.py.

Each integer case first asserts that the library (mphip_debug_conv2d_bwd_weight_plan: the launcher's own decision) reports the kernel,
the splits, the tiles per split and the pixel tiles the case claims, and that every edge its id names holds for the shape.

Why no tolerance (integer cases): x, dy are integers in [-4, 4] and both contain a 4, so both operand scales are 2^11 (max * scale =
2^13).  Every scaled operand is an exact f16, every `lo` half is 0, every product an integer times 2^22 and every partial sum an integer
below N*H*W*16 < 2^24 times 2^22: exact in fp32 in any order, over any split and through the slab reduce.  The float64 gradient is THE
answer and dW must be torch.equal to it.  Each case asserts the bound, and that ATen's fp32 CPU gradient equals the float64 one, before
it touches the GPU.

Edges (`edge_holds`): ci%64 / co%64 (ragged channel blocks; the tile is 64 x 64), ci+16 / co+32 (one channel chunk past a block),
ragged-h, ragged-w (against the 8 x 8 pixel tile: the masked kernel, id 2), w<8 (a map narrower than one K group), h1 (the kh = 0 and
kh = 2 taps see only padding), w1, cols1 / cols2 / cols3 (tile columns: with three a middle tile has both side halos), tps>1,
uneven-last, cross-sample, single (N = 1, one tile, one split).

Rounding (Gaussian data): the project's rule of tests/test_gpu_conv2d_f16x3.py, max|got - t64| <= 4 * max|t32 - t64| + 2^-21 * A,
t32 = ATen's fp32 CPU gradient, A = max over outputs of sum |dy||x|.  Each case shows on the CPU that the bar can fail: a float64
emulation of a one-product kernel must exceed it tenfold, the three-product emulation must stay under a tenth of it.  err, bar and
ratio are printed; with MPHIP_PARITY_JSON=<file> the worst ratios go to that file (profiles/conv2d_bwd_parity.json holds one MI355X run).

Magnitudes: a 128-pixel integer case with x and dy scaled by 2^e.  The result is the integer gradient times 2^(2e), rounded once to fp32
(0 below the subnormals, Inf above the range).  The unscale must be two factors applied in turn: with their single product an exact 0
of dW becomes NaN at e >= 97 (0 * Inf), and at (x, dy) * (2^-100, 2^-30) every element becomes 0 (2^-111 * 2^-41 = 0 in fp32)."""
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
VEC, MASKED = 1, 2           # kernel ids of mphip_debug_conv2d_bwd_weight_plan (0: refused)
RANGE_FLOATS = 4100
WS_HEAD = RANGE_FLOATS * 4 + 256

# ((N, Ci, Co, H, W), claimed (kernel, splits, tiles per split, tiles), edges)
INT_CASES = [
    ((2, 16, 32, 12, 20), (MASKED, 12, 1, 12), ("ci%64", "co%64", "ragged-h", "ragged-w", "cols3")),
    ((1, 48, 96, 9, 16), (VEC, 4, 1, 4), ("ci%64", "co%64", "co+32", "ragged-h", "cols2")),
    ((1, 80, 160, 8, 8), (VEC, 1, 1, 1), ("ci+16", "co+32", "cols1", "single")),
    ((2, 16, 32, 5, 3), (MASKED, 2, 1, 2), ("w<8", "ragged-h", "ragged-w", "cols1")),
    ((3, 16, 32, 1, 1), (MASKED, 3, 1, 3), ("h1", "w1", "w<8")),
    ((1, 16, 32, 1, 24), (VEC, 3, 1, 3), ("h1", "cols3")),
    ((1, 256, 256, 40, 72), (VEC, 23, 2, 45), ("tps>1", "uneven-last")),
    ((2, 256, 256, 24, 56), (VEC, 21, 2, 42), ("tps>1", "cross-sample")),
]
OUTSIDE_CASES = [(1, 24, 32, 8, 8), (1, 16, 16, 8, 8), (1, 8, 32, 8, 8)]     # Ci = 24, Co = 16, Ci = 8
# Gaussian data: a ragged one, one with several tiles per split (and Ci >= 128), one with Ci >= 128 on whole tiles
ROUNDING_CASES = [
    ((2, 48, 96, 12, 20), (MASKED, 12, 1, 12)),
    ((2, 256, 256, 24, 56), (VEC, 21, 2, 42)),
    ((1, 128, 64, 16, 16), (VEC, 4, 1, 4)),
]
MAGNITUDE_CASE = ((1, 48, 96, 8, 16), (VEC, 2, 1, 2))      # 128 pixels
MAGNITUDE_EXPONENTS = (-126, -118, -116, -60, 0, 60, 97, 99, 112)
BWD_DATA_CASES = [(2, 32, 64, 12, 20), (1, 64, 32, 9, 16)]     # the conv Ci -> Co whose dx is computed
FN_SHAPE = (2, 32, 64, 12, 20)


def case_id(row):
    (n, ci, co, h, w), (kern, splits, tps, ntiles), *rest = row
    edges = rest[0] if rest else ()
    return f"{n}x{ci}x{co}@{h}x{w}-k{kern}-t{ntiles}-s{splits}-tps{tps}" + "".join(f"-{e}" for e in edges)


def bwd_plan(lib, shape):
    out = (ctypes.c_int * 4)()
    assert lib.mphip_debug_conv2d_bwd_weight_plan(*shape, out) == 1
    return tuple(out)


def splits_of_tiles(plan):
    _, splits, tps, ntiles = plan
    return [(s * tps, min(ntiles, (s + 1) * tps)) for s in range(splits)]


def edge_holds(edge, shape, plan):
    n, ci, co, h, w = shape
    kern, splits, tps, ntiles = plan
    cols = (w + 7) // 8
    if edge == "ci%64":
        return ci % 64 != 0
    if edge == "co%64":
        return co % 64 != 0
    if edge == "ci+16":
        return ci % 64 == 16 and ci > 64
    if edge == "co+32":
        return co % 64 == 32 and co > 64
    if edge == "ragged-h":
        return h % 8 != 0
    if edge == "ragged-w":
        return w % 8 != 0 and kern == MASKED
    if edge == "w<8":
        return w < 8
    if edge == "h1":
        return h == 1
    if edge == "w1":
        return w == 1
    if edge in ("cols1", "cols2", "cols3"):
        return cols == int(edge[-1])
    if edge == "tps>1":
        return tps > 1
    if edge == "uneven-last":
        return splits > 1 and 0 < ntiles - (splits - 1) * tps < tps
    if edge == "cross-sample":
        per_sample = ntiles // n
        return n > 1 and ntiles == n * per_sample and any(b // per_sample != (e - 1) // per_sample for b, e in splits_of_tiles(plan))
    if edge == "single":
        return n == 1 and ntiles == 1 and splits == 1
    raise AssertionError(f"unknown edge {edge}")


def claim_holds(lib, row):
    """the library reports the plan the row claims, the shape is supported, and every edge the id names holds"""
    shape, claimed, *rest = row
    n, ci, co, h, w = shape
    plan = bwd_plan(lib, shape)
    assert plan == claimed, (case_id(row), plan)
    assert lib.mphip_conv2d_bwd_weight_supported(*shape) == 1
    assert plan[0] == (VEC if w % 8 == 0 else MASKED)
    assert plan[3] == n * ((h + 7) // 8) * ((w + 7) // 8)
    assert plan[1] * plan[2] >= plan[3] > (plan[1] - 1) * plan[2]
    for e in (rest[0] if rest else ()):
        assert edge_holds(e, shape, plan), (case_id(row), e, plan)
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
def dw_ref(x, dy):
    """dW[co][ci][kh][kw] = sum dy[n][co][h][w] * x[n][ci][h+kh-1][w+kw-1] (zero padding), one float64 matrix product per tap"""
    x, dy = x.double(), dy.double()
    n, ci, h, w = x.shape
    co = dy.shape[1]
    a = dy.transpose(0, 1).reshape(co, -1)
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.empty(co, ci, 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            out[:, :, kh, kw] = a @ xp[:, :, kh:kh + h, kw:kw + w].transpose(0, 1).reshape(ci, -1).t()
    return out


def dw_aten32(x, dy):
    """ATen's own fp32 CPU gradient (autograd of F.conv2d)"""
    wt = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=torch.float32, requires_grad=True)
    F.conv2d(x.float(), wt, None, padding=1).backward(dy.float())
    return wt.grad


def _ints(shape, gen):
    t = torch.randint(-4, 5, shape, generator=gen).float()
    t.view(-1)[0] = 4.0      # the maximum is 4 whatever the draw: the operand scale is 2^11
    return t


@functools.lru_cache(maxsize=None)
def int_case(shape, seed):
    """(x, dy, float64 dW) of an integer case, computed once and left unchanged; asserts that fp32 is exact on it"""
    n, ci, co, h, w = shape
    assert n * h * w * 16 < EXACT
    gen = torch.Generator().manual_seed(seed)
    x, dy = _ints((n, ci, h, w), gen), _ints((n, co, h, w), gen)
    assert x.abs().max().item() == 4 and dy.abs().max().item() == 4
    want = dw_ref(x, dy)
    assert torch.equal(dw_aten32(x, dy).double(), want)      # a condition on the inputs: ATen's fp32 gradient is exact on them
    assert want.abs().max().item() < EXACT
    return x, dy, want


def _offset_view(t, dev):
    """A contiguous device copy of `t` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


_RECORD = {}


def note(test, case, ratio):
    """worst err / bar per test; rewritten on every call when MPHIP_PARITY_JSON names a file (shared with test_gpu_g2d_body_train.py)"""
    cur = _RECORD.setdefault(test, {"worst_err_over_bar": -1.0, "at": None, "checks": 0})
    cur["checks"] += 1
    if ratio > cur["worst_err_over_bar"]:
        cur["worst_err_over_bar"], cur["at"] = float(f"{ratio:.4g}"), case
    out = os.environ.get("MPHIP_PARITY_JSON")
    if out:
        with open(out, "w") as f:
            json.dump({"what": "tests/test_gpu_conv2d_bwd.py and tests/test_gpu_g2d_body_train.py: worst max|got - t64| / bar per test and the "
                               "case it occurred at (kernel level: bar = 4 * max|t32 - t64| + 2^-21 * max sum |dy||x|; Conv2dFn and module "
                               "level: bar = 4 * max|t32 - t64| + 2^-21 * max|t64| per tensor)",
                       "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "tests": _RECORD}, f, indent=1)
            f.write("\n")


# ---------------------------------------------------------------------------------------------------------------- a. integer cases
@pytest.mark.parametrize("row", INT_CASES, ids=case_id)
def test_bwd_weight_bit_exact(ops, lib, dev, row):
    shape, claimed, edges = row
    claim_holds(lib, row)
    x, dy, want = int_case(shape, 90260 + 7 * INT_CASES.index(row))
    want = want.float()
    xd, dyd = x.to(dev), dy.to(dev)
    assert xd.data_ptr() % 16 == 0 and dyd.data_ptr() % 16 == 0 and ops.tensor_range(xd) is None
    db, scale = ops.grad_prep(dyd)                                    # S = H * W
    assert scale.cpu().tolist()[:3] == [2.0 ** 11, 2.0 ** -11, 4.0]
    assert torch.equal(db.cpu().double(), dy.double().sum(dim=(0, 2, 3)))
    first = ops.conv2d_bwd_weight(xd, dyd, scale)                     # x_range left to the library
    assert tuple(first.shape) == (shape[2], shape[1], 3, 3)
    assert torch.equal(first.cpu(), want), "library-measured x range"
    assert torch.equal(ops.conv2d_bwd_weight(xd, dyd, scale), first), "second launch: the same bits"
    loose = torch.zeros(RANGE_FLOATS, dtype=torch.float32)
    loose[2] = 1000.0 * 4.0                                           # derive mode, a rigorous but loose bound: scale 2^2
    assert torch.equal(ops.conv2d_bwd_weight(xd, dyd, scale, x_range=loose.to(dev)).cpu(), want), "explicit loose x bound"
    assert torch.equal(ops.conv2d_bwd_weight(xd, dyd, scale, x_range=ops.absmax_range(xd)).cpu(), want), "x range of absmax_range"
    # pointers the 16-byte loads cannot take: the wrapper copies them once, the result stays exact
    assert torch.equal(ops.conv2d_bwd_weight(_offset_view(x, dev), _offset_view(dy, dev), scale).cpu(), want), "offset views"


@pytest.mark.parametrize("shape", OUTSIDE_CASES, ids=lambda s: "x".join(map(str, s)))
def test_outside_the_rule_is_refused(ops, lib, dev, shape):
    n, ci, co, h, w = shape
    assert bwd_plan(lib, shape) == (0, 0, 0, 0) and lib.mphip_conv2d_bwd_weight_supported(*shape) == 0
    assert not ops.conv2d_bwd_weight_supported(*shape) and not ops.conv2d_bwd_supported(*shape, False)
    x, dy = torch.ones((n, ci, h, w), device=dev), torch.ones((n, co, h, w), device=dev)
    _, scale = ops.grad_prep(dy, want_bias=False)
    with pytest.raises(RuntimeError, match="conv2d_bwd_weight: unsupported shape"):
        ops.conv2d_bwd_weight(x, dy, scale)
    ws = torch.empty(1 << 16, device=dev)
    dw = torch.empty((co, ci, 3, 3), device=dev)
    rc = lib.mphip_conv2d_bwd_weight(x.data_ptr(), None, dy.data_ptr(), scale.data_ptr(), dw.data_ptr(), n, ci, co, h, w, ws.data_ptr(),
                                     ws.numel() * 4, None)
    assert rc == -1 and b"conv2d_bwd_weight: unsupported shape" in lib.mphip_last_error()


def test_the_entry_refuses_pointers_off_16_bytes_when_rows_are_vector_loads(ops, lib, dev):
    shape = (1, 48, 96, 8, 16)
    assert bwd_plan(lib, shape)[0] == VEC
    x, dy, _ = int_case(shape, 91260)
    n, ci, co, h, w = shape
    xd, dyd = _offset_view(x, dev), dy.to(dev)
    _, scale = ops.grad_prep(dyd, want_bias=False)
    nbytes = lib.mphip_conv2d_bwd_weight_workspace_bytes(*shape)
    ws = torch.empty(nbytes // 4, device=dev)
    dw = torch.empty((co, ci, 3, 3), device=dev)
    rc = lib.mphip_conv2d_bwd_weight(xd.data_ptr(), None, dyd.data_ptr(), scale.data_ptr(), dw.data_ptr(), n, ci, co, h, w, ws.data_ptr(),
                                     nbytes, None)
    assert rc == -1 and b"16-byte aligned" in lib.mphip_last_error()


# ---------------------------------------------------------------------------------------------------------------- b. backward-data
@pytest.mark.parametrize("shape", BWD_DATA_CASES, ids=lambda s: "x".join(map(str, s)))
def test_bwd_data_bit_exact(ops, dev, shape):
    """integer dy and weight: dx equals float64 conv_transpose2d and the autograd dx; the transposed pack is the flipped transpose"""
    n, ci, co, h, w = shape
    assert ops.conv2d_bwd_supported(n, ci, co, h, w, True)
    gen = torch.Generator().manual_seed(92260 + ci)
    dy, wt = _ints((n, co, h, w), gen), _ints((co, ci, 3, 3), gen)
    assert co * 9 * 16 < EXACT
    want = F.conv_transpose2d(dy.double(), wt.double(), padding=1)
    x = torch.zeros((n, ci, h, w), dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wt.double(), None, padding=1).backward(dy.double())
    assert torch.equal(x.grad, want)
    x32 = torch.zeros((n, ci, h, w), requires_grad=True)
    F.conv2d(x32, wt, None, padding=1).backward(dy)
    assert torch.equal(x32.grad.double(), want)
    dyd = dy.to(dev)
    _, scale = ops.grad_prep(dyd, want_bias=False)
    pack_t = ops.PackedConv2d(wt.to(dev), None, transposed=True)
    assert (pack_t.co, pack_t.ci) == (ci, co) and pack_t.transposed and not bool(pack_t.bias.any())
    dx = ops.conv2d_bwd_data(dyd, pack_t, scale)
    assert torch.equal(dx.cpu().double(), want)
    # the same pack through the ordinary entry on the flipped, transposed weight built with torch ops
    flipped = ops.PackedConv2d(wt.flip(2, 3).transpose(0, 1).contiguous().to(dev), torch.zeros(ci, device=dev))
    assert torch.equal(pack_t.packed().view(torch.int32), flipped.packed().view(torch.int32))
    with pytest.raises(RuntimeError, match="transposed=True"):
        ops.conv2d_bwd_data(dyd, flipped, scale)


def test_transposed_pack_rule(ops, dev):
    """the roles swap: the weight's Co % 16 == 0 and Ci % 32 == 0"""
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.PackedConv2d(torch.ones((32, 16, 3, 3), device=dev), None, transposed=True)
    assert ops.conv2d_bwd_supported(1, 16, 32, 8, 8, False) and not ops.conv2d_bwd_supported(1, 16, 32, 8, 8, True)
    p = ops.PackedConv2d(torch.ones((16, 32, 3, 3), device=dev), None, transposed=True)     # Co = 16 is fine for the pack alone
    assert (p.co, p.ci) == (32, 16)


# ---------------------------------------------------------------------------------------------------------------- c. magnitudes
def _pow2_scale_pair(m):
    """scale_from_bits of csrc/mphip_common.h on a maximum m > 0: (scale, 1 / scale), the exponent clamped to +-120"""
    e = min(max(14 - math.frexp(m)[1], -120), 120)
    return 2.0 ** e, 2.0 ** -e


@functools.lru_cache(maxsize=None)
def _magnitude_case():
    shape, _ = MAGNITUDE_CASE
    x, dy, _ = int_case(shape, 93260)
    dy = dy.clone()
    dy[:, -1] = 0.0                       # a whole output channel of exact zeros in dW: 0 * Inf = NaN shows a single-product unscale
    assert dy.abs().max().item() == 4
    truth = dw_ref(x, dy)
    assert torch.equal(dw_aten32(x, dy).double(), truth) and not bool(truth[-1].any()) and bool(truth[:-1].any())
    return x, dy, truth


def _scaled(t, p):
    out = (t.double() * 2.0 ** p).float()
    assert torch.equal(out.double(), t.double() * 2.0 ** p)
    return out


def _check_magnitude(ops, lib, dev, p, q):
    """x * 2^p, dy * 2^q: dW is truth * 2^(p+q) rounded once to fp32; returns what the two unscales would give on the CPU"""
    claim_holds(lib, MAGNITUDE_CASE)
    x, dy, truth = _magnitude_case()
    want = (truth * 2.0 ** (p + q)).float()            # float64 holds truth * 2^(p+q) exactly; one rounding to fp32 (0 / Inf outside)
    xp, dyp = _scaled(x, p), _scaled(dy, q)
    # CPU emulation of the kernel's arithmetic from the reduce on: the exact accumulator in the scaled domain, then the unscale
    (sx, ix), (sd, idy) = _pow2_scale_pair(4 * 2.0 ** p), _pow2_scale_pair(4 * 2.0 ** q)
    acc = (truth * (2.0 ** p * sx) * (2.0 ** q * sd)).float()
    assert bool(torch.isfinite(acc).all()) and torch.equal(acc.double(), truth * (2.0 ** p * sx) * (2.0 ** q * sd))
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    two = (acc * f32(idy)) * f32(ix)
    one = acc * (f32(idy) * f32(ix))
    assert torch.equal(torch.nan_to_num(two, nan=-1.0), torch.nan_to_num(want, nan=-1.0)) and not bool(torch.isnan(two).any())
    xd, dyd = xp.to(dev), dyp.to(dev)
    db, scale = ops.grad_prep(dyd)
    s0, s1, s2 = scale.cpu().tolist()[:3]
    assert (s0, s1, s2) == (sd, idy, 4 * 2.0 ** q)
    assert torch.equal(db.cpu().double(), dy.double().sum(dim=(0, 2, 3)) * 2.0 ** q)
    dw = ops.conv2d_bwd_weight(xd, dyd, scale)
    assert not bool(torch.isnan(dw).any())
    assert torch.equal(dw.cpu(), want)
    return one, want


@pytest.mark.parametrize("e", MAGNITUDE_EXPONENTS, ids=lambda e: f"2^{e}")
def test_magnitude_sweep_is_exact_or_correctly_flushed(ops, lib, dev, e):
    one, want = _check_magnitude(ops, lib, dev, e, e)
    if e >= 97:     # 1/scale_dy * 1/scale_x overflows: the single product turns the exact zeros of dW into NaN
        assert bool(torch.isinf(want[:-1]).any()) and not bool(want[-1].any()) and bool(torch.isnan(one[-1]).all())
    if e <= -116:   # far below the subnormals: flushed
        assert not bool(want.any())
    if e in (-60, 0):
        assert bool(torch.isfinite(want).all()) and bool(want.any())
    if e == 60:     # 2^120 times the integers: some elements finite, the largest already Inf
        assert bool(torch.isfinite(want[:-1]).any()) and bool(want.any())


def test_unscale_is_two_factors_not_their_product(ops, lib, dev):
    """(x, dy) * (2^-100, 2^-30): 1/scale_x = 2^-111 and 1/scale_dy = 2^-41, their product 2^-152 is 0 in fp32, the results (up to 2^-119)
    are not"""
    one, want = _check_magnitude(ops, lib, dev, -100, -30)
    assert not bool(one.any()) and want.abs().max().item() > 2.0 ** -126


# ---------------------------------------------------------------------------------------------------------------- d. rounding
def _split_f16(t):
    """(hi, lo) of t at its power-of-two operand scale, unscaled, float64: what the three-product kernels multiply"""
    s = R.pow2_operand_scale(t.abs().max().item(), 14)
    v = t.float() * s
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi.double() / s, lo.double() / s


@functools.lru_cache(maxsize=None)
def rounding_case(shape):
    n, ci, co, h, w = shape
    x, dy = R.seeded_tensor((n, ci, h, w), 2401, scale=1.5), R.seeded_tensor((n, co, h, w), 2402)
    t64 = dw_ref(x, dy)
    e32 = (dw_aten32(x, dy).double() - t64).abs().max().item()
    A = dw_ref(x.abs(), dy.abs()).max().item()
    bar = 4 * e32 + 2.0 ** -21 * A
    xh, xl = _split_f16(x)
    dh, dl = _split_f16(dy)
    one = dw_ref(xh, dh)
    three = one + dw_ref(xl, dh) + dw_ref(xh, dl)
    e1, e3 = (one - t64).abs().max().item(), (three - t64).abs().max().item()
    return x, dy, t64, bar, e1, e3


@pytest.mark.parametrize("row", ROUNDING_CASES, ids=case_id)
def test_rounding_bar(ops, lib, dev, row):
    shape, claimed = row
    claim_holds(lib, row)
    x, dy, t64, bar, e1, e3 = rounding_case(shape)
    print(f"{case_id(row)}: CPU emulation, one product {e1 / bar:.1f} x bar, three products {e3 / bar:.4f} x bar")
    assert e1 >= 10 * bar, (e1, bar)
    assert e3 <= 0.1 * bar, (e3, bar)
    xd, dyd = x.to(dev), dy.to(dev)
    _, scale = ops.grad_prep(dyd, want_bias=False)
    dw = ops.conv2d_bwd_weight(xd, dyd, scale)
    err = (dw.cpu().double() - t64).abs().max().item()
    print(f"{case_id(row)}: err {err:.3e}, bar {bar:.3e}, err / bar {err / bar:.4f}")
    note("test_rounding_bar", case_id(row), err / bar)
    assert err <= bar, (err, bar)
    assert torch.equal(ops.conv2d_bwd_weight(xd, dyd, scale), dw), "two launches on the same inputs give equal bits"


# ---------------------------------------------------------------------------------------------------------------- e. Conv2dFn
def tensor_bar(got, t64, t32):
    """(err, bar) of the module-level rule: max|got - t64| <= 4 * max|t32 - t64| + 2^-21 * max|t64|"""
    err = (got.detach().cpu().double() - t64).abs().max().item()
    return err, 4 * (t32.double() - t64).abs().max().item() + 2.0 ** -21 * t64.abs().max().item()


@functools.lru_cache(maxsize=None)
def _fn_case():
    n, ci, co, h, w = FN_SHAPE
    x, wt, b, r, dy = (R.seeded_tensor(s, 2500 + i, scale=sc) for i, (s, sc) in enumerate(
        (((n, ci, h, w), 1.5), ((co, ci, 3, 3), 0.08), ((co,), 0.5), ((n, co, h, w), 1.0), ((n, co, h, w), 1.0))))
    out = {}
    for dt in (torch.float64, torch.float32):
        leaves = [t.to(dt).clone().requires_grad_(True) for t in (x, wt, b, r)]
        y = F.relu(F.conv2d(leaves[0], leaves[1], leaves[2], padding=1) + leaves[3])
        y.backward(dy.to(dt))
        out[dt] = [y.detach()] + [t.grad for t in leaves]
    return (x, wt, b, r, dy), out[torch.float64], out[torch.float32]


def _fn_run(ops, dev, x_requires_grad):
    from megaportrait_hack_amd import autograd as ag

    (x, wt, b, r, dy), t64, t32 = _fn_case()
    xd = x.to(dev).requires_grad_(x_requires_grad)
    wd, bd, rd = (t.to(dev).requires_grad_(True) for t in (wt, b, r))
    y = ag.conv2d(xd, wd, bd, ops.PackedConv2d(wd, bd), None, residual=rd, relu=True)
    return y, (xd, wd, bd, rd), dy.to(dev), t64, t32


def test_conv2d_fn_matches_float64_autograd(ops, dev):
    y, leaves, dyd, t64, t32 = _fn_run(ops, dev, True)
    assert type(y.grad_fn).__name__ == "Conv2dFnBackward"
    y.backward(dyd)
    for name, got, a, b in zip(("y", "dx", "dW", "db", "dresidual"), [y] + [t.grad for t in leaves], t64, t32):
        err, bar = tensor_bar(got, a, b)
        print(f"Conv2dFn {name}: err {err:.3e}, bar {bar:.3e}, err / bar {err / bar:.4f}")
        note("test_conv2d_fn_matches_float64_autograd", name, err / bar)
        assert err <= bar, (name, err, bar)
    with pytest.raises(RuntimeError):
        y.backward(dyd)            # a second backward through the same graph


def test_conv2d_fn_without_dx_makes_no_backward_data_launch(ops, dev, monkeypatch):
    y, leaves, dyd, t64, t32 = _fn_run(ops, dev, False)
    calls = []
    real = ops.conv2d_bwd_data
    monkeypatch.setattr(ops, "conv2d_bwd_data", lambda *a, **k: calls.append(1) or real(*a, **k))
    y.backward(dyd)
    assert not calls and leaves[0].grad is None
    for name, got, a, b in zip(("dW", "db", "dresidual"), [t.grad for t in leaves[1:]], t64[2:], t32[2:]):
        err, bar = tensor_bar(got, a, b)
        assert err <= bar, (name, err, bar)
    y2, leaves2, _, _, _ = _fn_run(ops, dev, True)
    y2.backward(dyd)
    assert calls == [1] and leaves2[0].grad is not None
