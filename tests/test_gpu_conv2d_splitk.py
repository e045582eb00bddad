"""The split-K form of the 2-D 3x3 convs on the matrix cores (csrc/conv2d_splitk_f16x3.hip: mphip_conv2d_split_supported, mphip_conv2d_splits,
mphip_conv2d_split_workspace_bytes, mphip_conv2d_split_fwd; the `splits` keyword of ops.conv2d / ops.conv2d_grouped), with the conventions
of tests/test_gpu_conv2d_grouped.py.

Integer data makes every product, partial sum and sum of partial maps an exact fp32 value (|sum| <= 9*256*8 + 16 < 2^24, power-of-two scales,
every lo half 0): those cases are compared with torch.equal against the fp64 oracle.  The contract that pins the arithmetic on random data:
with one descriptor of the whole x and one header scale (the same +-max|w| planted in every K range of the weight), the launch writes the
bits of  act(((y_0 + y_1) + ... + y_{S-1}) + bias (+ residual))  evaluated with fp32 torch ops in that order, y_s = mphip_conv2d_fwd on the
input channels and the weight columns of K range s with a zero bias (for groups: each group's range, assembled into the dense weight of the
grouped test).  Power-of-two scales commute with fp32 rounding away from underflow, so y_s carries the bits of partial map s times the
unscale.  Random data is also held to the project's conv bar 4*e_torch + 2^-21*A (A = max over outputs of sum |w||x| + |bias| + |residual|,
as defined in tests/test_gpu_conv2d_grouped.py) against torch's fp32 conv on the same GPU."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANGE_FLOATS = 4100

# (N, Ci, Co, H, W, groups, S): one chunk per split and half a channel tile; a ragged tile smaller than one tile, two channel tiles and an odd
# H*W (the scalar finish path); a split that is no power of two across tile rows and columns; whole tiles (the 16-byte finish path, 96
# finish workgroups); grouped with Cig = 32; the nets' own channel counts, grouped; sixteen splits of one chunk each
SHAPES = [(1, 32, 32, 1, 1, 1, 2), (2, 64, 96, 5, 7, 1, 4), (1, 96, 64, 17, 19, 1, 3), (3, 64, 128, 16, 16, 1, 2), (1, 64, 128, 9, 33, 2, 2),
          (1, 512, 512, 4, 4, 2, 8), (1, 256, 256, 8, 8, 1, 16)]
OFFSET_SHAPES = [SHAPES[3], SHAPES[5]]      # H*W % 4 == 0: aligned they take the 16-byte finish path, 4 bytes off the scalar one
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("plus4bytes" if v else "aligned")


def _lib():
    from megaportrait_hack_amd import _lib as L

    return L.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _oracle(x, w, b, res, relu, groups):
    y = F.conv2d(x.double(), w.double(), b.double(), padding=1, groups=groups)
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu else y


def _misaligned(t):
    """The same values at a base pointer 4 bytes past a 16-byte boundary."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = big[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _dense(w, groups):
    """[Co, Ci/groups, 3, 3] -> [Co, Ci, 3, 3]: the group blocks on the diagonal, exact zeros elsewhere."""
    co, cig = w.shape[:2]
    cog = co // groups
    d = torch.zeros(co, cig * groups, 3, 3, dtype=w.dtype, device=w.device)
    for g in range(groups):
        d[g * cog:(g + 1) * cog, g * cig:(g + 1) * cig] = w[g * cog:(g + 1) * cog]
    return d


def _pack(w):
    lib = _lib()
    co, ci = w.shape[:2]
    nb = lib.mphip_conv2d_packed_weight_bytes(co, ci)
    assert nb > 0
    wp = torch.empty((nb + 3) // 4, device=w.device)
    assert lib.mphip_pack_conv2d_weight(_p(w.contiguous()), _p(wp), co, ci, _stream()) == 0, lib.mphip_last_error()
    return wp


def _split(groups, splits, x, wp, bias, co, res=None, relu=False, x_range=None, out_range=None, y=None):
    """mphip_conv2d_split_fwd called directly (no descriptor is looked up on the tensors); y: write into this tensor."""
    lib = _lib()
    n, ci, h, w = x.shape
    y = torch.empty((n, co, h, w), device=x.device) if y is None else y
    nb = lib.mphip_conv2d_split_workspace_bytes(n, ci, co, h, w, groups, splits)
    assert nb > 0
    ws = torch.empty((nb + 3) // 4, device=x.device)
    rc = lib.mphip_conv2d_split_fwd(_p(x), _p(x_range), _p(wp), _p(bias), _p(res), _p(y), _p(out_range), n, ci, co, h, w, groups, splits,
                                    int(relu), _p(ws), nb, _stream())
    assert rc == 0, lib.mphip_last_error()
    return y


def _unsplit(groups, x, wp, bias, co, res=None, relu=False, x_range=None, out_range=None):
    """mphip_conv2d_grouped_fwd (groups >= 1) or mphip_conv2d_fwd (groups None) called directly."""
    lib = _lib()
    n, ci, h, w = x.shape
    y = torch.empty((n, co, h, w), device=x.device)
    g = () if groups is None else (groups,)
    fn, wsfn = ((lib.mphip_conv2d_fwd, lib.mphip_conv2d_workspace_bytes) if groups is None
                else (lib.mphip_conv2d_grouped_fwd, lib.mphip_conv2d_grouped_workspace_bytes))
    nb = wsfn(n, ci, co, h, w, *g)
    ws = torch.empty((nb + 3) // 4, device=x.device)
    rc = fn(_p(x), _p(x_range), _p(wp), _p(bias), _p(res), _p(y), _p(out_range), n, ci, co, h, w, *g, int(relu), _p(ws), nb, _stream())
    assert rc == 0, lib.mphip_last_error()
    return y


def _range_max(rng):
    r = rng.view(torch.int32)
    n = int(r[3].item())
    assert rng[0].item() == 0.0 and 0 < n <= RANGE_FLOATS - 4
    return torch.cat([r[2:3], r[4:4 + n]]).max().view(1).view(torch.float32).item()


def _random_case(shape, seed):
    """x, weight (|w| <= 0.4 with +-0.5 planted in every K range), bias, residual on the GPU."""
    n, ci, co, h, w, g, s = shape
    cig = ci // g
    x, b, res = _rand((n, ci, h, w), seed, 2.0), _rand((co,), seed + 2), _rand((n, co, h, w), seed + 3)
    wt = _rand((co, cig, 3, 3), seed + 1, 0.1).clamp_(-0.4, 0.4)
    for k in range(s):
        wt[0, k * cig // s, 0, 0] = 0.5 if k % 2 == 0 else -0.5
    return x.to(DEV), wt.to(DEV), b.to(DEV), res.to(DEV)


@pytest.mark.parametrize("shape,offset", [(s, False) for s in SHAPES] + [(s, True) for s in OFFSET_SHAPES], ids=_ids)
def test_integer_data_is_bit_exact(shape, offset):
    from megaportrait_hack_amd import ops

    lib = _lib()
    n, ci, co, h, w, g, s = shape
    assert lib.mphip_conv2d_split_supported(*shape) == 1 and ops.conv2d_split_supported(*shape)
    x, wt = _ints((n, ci, h, w), -4, 4, 1), _ints((co, ci // g, 3, 3), -2, 2, 2)
    b, res = _ints((co,), -8, 8, 3), _ints((n, co, h, w), -8, 8, 4)
    xg, rg, bg = x.to(DEV), res.to(DEV), b.to(DEV)
    y = torch.full((n, co, h, w), float("nan"), device=DEV)
    if offset:
        xg, rg, y = _misaligned(xg), _misaligned(rg), _misaligned(y)
    wp = _pack(wt.to(DEV))
    ops.f16x3_saturation_count(reset=True)
    for relu in (False, True):
        for with_res in (False, True):
            want = _oracle(x, wt, b, res if with_res else None, relu, g).float()
            assert want.abs().max() < 2 ** 24
            got = _split(g, s, xg, wp, bg, co, res=rg if with_res else None, relu=relu, y=y)
            assert got.data_ptr() % 16 == (4 if offset else 0)
            assert torch.equal(got.cpu(), want), (shape, relu, with_res, (got.cpu() - want).abs().max().item())
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_split_writes_the_bits_of_the_ordered_sum_of_its_ranges(shape):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w, g, s = shape
    cig, per = ci // g, ci // g // s
    x, wt, b, res = _random_case(shape, 51)
    assert wt.abs().max().item() == 0.5
    wp = _pack(wt)
    desc = ops.absmax_range(x.clone())                   # one descriptor of the whole x, for every call
    zero = torch.zeros(co, device=DEV)
    parts = []
    for k in range(s):
        cols = slice(k * per, (k + 1) * per)
        xs = torch.cat([x[:, q * cig + cols.start:q * cig + cols.stop] for q in range(g)], dim=1).contiguous()
        ws = _dense(wt[:, cols].contiguous(), g)
        assert ws.abs().max().item() == 0.5 and xs.shape[1] == ws.shape[1] == ci // s
        wps = _pack(ws)
        assert torch.equal(wps[:4], wp[:4])              # the same header: one scale
        parts.append(_unsplit(None, xs, wps, zero, co, x_range=desc))
    acc = parts[0]
    for k in range(1, s):
        acc = acc + parts[k]
    acc = acc + b.view(1, -1, 1, 1)
    desc_before = desc.clone()
    for relu, r in ((False, None), (True, None), (False, res), (True, res)):
        want = acc if r is None else acc + r
        want = torch.relu(want) if relu else want
        got = _split(g, s, x, wp, b, co, res=r, relu=relu, x_range=desc)
        assert torch.equal(got, want), (shape, relu, r is not None, (got - want).abs().max().item())
    assert torch.equal(desc, desc_before)


_PARITY = []


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_random_data_accuracy(shape):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w, g, s = shape
    x, wt = _rand((n, ci, h, w), 11), _rand((co, ci // g, 3, 3), 12, 0.05)
    b, res = _rand((co,), 13), _rand((n, co, h, w), 14)
    y64 = _oracle(x, wt, b, res, True, g)
    A = (F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), padding=1, groups=g) + res.double().abs()).max().item()
    xg, wg, bg, rg = x.to(DEV), wt.to(DEV), b.to(DEV), res.to(DEV)
    cudnn = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        yt = F.relu(F.conv2d(xg, wg, bg, padding=1, groups=g) + rg)
    finally:
        torch.backends.cudnn.allow_tf32 = cudnn
    ops.f16x3_saturation_count(reset=True)
    pack = ops.PackedConv2d(wg, bg, g)
    yh = (ops.conv2d if g == 1 else ops.conv2d_grouped)(xg, pack, residual=rg, relu=True, splits=s)
    e_torch = (yt.cpu().double() - y64).abs().max().item()
    e_hip = (yh.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -21 * A
    print(f"conv2d_split parity {shape}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} A={A:.3e} bound={bound:.3e} ratio={e_hip / bound:.3f}")
    _PARITY.append({"shape_N_Ci_Co_H_W_groups_splits": list(shape), "e_hip": float(f"{e_hip:.4g}"), "e_torch": float(f"{e_torch:.4g}"),
                    "A": float(f"{A:.4g}"), "bound": float(f"{bound:.4g}"), "e_hip_over_bound": float(f"{e_hip / bound:.4g}")})
    out = os.environ.get("MPHIP_PARITY_JSON")      # the measured values, for profiles/conv2d_splitk_parity.json
    if out and len(_PARITY) == len(SHAPES):
        with open(out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "cases": _PARITY}, f, indent=1)
    assert e_hip <= bound
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_ranges_descriptors_repeats_and_one_split(shape):
    """out_range folds to the bits of max|y|; a call that scans x and one given the descriptor, and two calls on the same inputs, write
    the same bits; splits = 1 writes the bits of the plain / grouped entry."""
    from megaportrait_hack_amd import ops

    n, ci, co, h, w, g, s = shape
    x, wt, b, res = _random_case(shape, 21)
    wp = _pack(wt)
    out_range = torch.full((RANGE_FLOATS,), 1.0e30, device=DEV)                # poisoned: the launch must initialise what it uses
    y = _split(g, s, x, wp, b, co, res=res, relu=False, out_range=out_range)
    assert _range_max(out_range) == y.abs().max().item()
    y_relu = _split(g, s, x, wp, b, co, relu=True, out_range=out_range)         # the same tensor again: initialised again
    assert _range_max(out_range) == y_relu.abs().max().item()
    desc = ops.absmax_range(x.clone())
    assert torch.equal(_split(g, s, x, wp, b, co, res=res, x_range=desc), y)   # the scan and the descriptor
    assert torch.equal(_split(g, s, x, wp, b, co, res=res), y)                 # a second call
    for relu in (False, True):
        one = _split(g, 1, x, wp, b, co, res=res, relu=relu)
        assert torch.equal(one, _unsplit(g, x, wp, b, co, res=res, relu=relu))
        if g == 1:
            assert torch.equal(one, _unsplit(None, x, wp, b, co, res=res, relu=relu))
    # the next conv reads y with the split launch's descriptor as with its own scan
    w2, b2 = _rand((32, co, 3, 3), 24, 0.1).to(DEV), _rand((32,), 25).to(DEV)
    wp2 = _pack(w2)
    y = _split(g, s, x, wp, b, co, res=res, out_range=out_range)
    assert torch.equal(_unsplit(None, y, wp2, b2, 32, x_range=out_range), _unsplit(None, y, wp2, b2, 32))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[5]], ids=_ids)
def test_python_keyword(shape):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w, g, s = shape
    x, wt, b, res = _random_case(shape, 31)
    pack = ops.PackedConv2d(wt, b, g)
    conv = ops.conv2d if g == 1 else ops.conv2d_grouped
    base = conv(x, pack, residual=res, relu=True)
    assert torch.equal(conv(x, pack, residual=res, relu=True, splits=None), base)
    assert torch.equal(conv(x, pack, residual=res, relu=True, splits=1), base)
    explicit = conv(x, pack, residual=res, relu=True, splits=s, want_range=True)
    assert torch.equal(explicit, _split(g, s, x, pack.packed(), b, co, res=res, relu=True))
    assert _range_max(ops.current_range(explicit)) == explicit.abs().max().item()
    assert ops.current_range(conv(x, pack, splits=s)) is None
    auto = ops.conv2d_splits(n, ci, co, h, w, g)
    assert auto == _lib().mphip_conv2d_splits(n, ci, co, h, w, g) and auto >= 1
    assert torch.equal(conv(x, pack, residual=res, relu=True, splits="auto"), conv(x, pack, residual=res, relu=True, splits=auto))
    if auto > 1:
        assert torch.equal(conv(x, pack, residual=res, relu=True, splits="auto"),
                           _split(g, auto, x, pack.packed(), b, co, res=res, relu=True))


def test_python_refusals():
    from megaportrait_hack_amd import ops

    z = lambda *s: torch.zeros(*s, device=DEV)
    p1, p2 = ops.PackedConv2d(z(64, 64, 3, 3), z(64)), ops.PackedConv2d(z(128, 32, 3, 3), z(128), 2)
    x = z(1, 64, 8, 8)
    for kw in (dict(out_dtype=torch.float16), dict(products=3), dict(products=1)):
        for splits in (2, "auto"):
            with pytest.raises(RuntimeError, match="typed map, out_dtype or products"):
                ops.conv2d(x, p1, splits=splits, **kw)
    with pytest.raises(RuntimeError, match="typed map, out_dtype or products"):
        ops.conv2d(x.half(), p1, splits=2)
    assert ops.conv2d(x, p1, splits=1, products=1).shape == (1, 64, 8, 8)      # one split: today's typed path
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.conv2d(x, p1, splits=3)
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.conv2d_grouped(x, p2, splits=4)      # 4 divides Ci / 16, not (Ci / groups) / 16
    with pytest.raises(RuntimeError, match="splits"):
        ops.conv2d(x, p1, splits="always")
    with pytest.raises(RuntimeError, match="grouped"):
        ops.conv2d(x, p2, splits=2)
    with pytest.raises(RuntimeError, match="residual"):
        ops.conv2d(x, p1, residual=z(1, 64, 4, 4), splits=2)
    torch.cuda.synchronize()
