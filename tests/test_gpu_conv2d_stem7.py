"""The 7x7 stem conv from a 3-channel image at stride 1 and 2 on the matrix cores, with the optional ReLU and 3x3/2 max-pool in the same
launch (csrc/conv2d_stem7_f16x3.hip: mphip_conv2d_stem7_supported, mphip_conv2d_stem7_packed_weight_bytes,
mphip_pack_conv2d_stem7_weight, mphip_conv2d_stem7_workspace_bytes, mphip_conv2d_stem7_fwd), with the conventions of
tests/test_gpu_conv2d_pw.py.

Integer data makes every product and partial sum an exact fp32 value (|sum| <= 147*8 + 8 < 2^24, power-of-two scales, every lo half 0), so
those cases are compared with torch.equal against the fp64 oracle.  Three identities pin the arithmetic on random data, all with one
explicit descriptor: the stride-2 launch writes the bits of the stride-1 launch at the even rows and columns; the pooled launch writes
F.max_pool2d(3, 2, 1) of the flat launch's bits (NaN and +-Inf enter through the bias, so the operand scaling is not involved); and an
image placed in a zero canvas gives the translated bits of the image alone.  Random data is also held to the project's bar
4*e_torch + 2^-21*A (A = max over outputs of sum |w||x| + |bias|) against torch's fp32 conv on the same GPU with TF32 off; the measured
values are printed and, when MPHIP_PARITY_JSON names a file, written there (profiles/conv2d_stem7_parity.json holds one MI355X run)."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANGE_FLOATS = 4100
EINVAL, EWORKSPACE = -1, -3


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


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _y_shape(n, co, h, w, s, pool):
    ho, wo = (h + s - 1) // s, (w + s - 1) // s
    return (n, co, (ho + 1) // 2, (wo + 1) // 2) if pool else (n, co, ho, wo)


def _oracle(x, w, b, s, relu, pool):
    y = F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=3)
    if relu:
        y = F.relu(y)
    return F.max_pool2d(y, 3, 2, 1) if pool else y


def _misaligned(t):
    """The same values at a base pointer 4 bytes past a 16-byte boundary."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = big[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _pack(w):
    lib = _lib()
    nb = lib.mphip_conv2d_stem7_packed_weight_bytes(w.shape[0])
    assert nb > 0
    wp = torch.empty((nb + 3) // 4, device=w.device)
    assert lib.mphip_pack_conv2d_stem7_weight(_p(w), _p(wp), w.shape[0], _stream()) == 0, lib.mphip_last_error()
    return wp


def _fwd(x, wp, bias, co, stride=1, relu=False, pool=False, x_range=None, out_range=None, ws="auto"):
    """mphip_conv2d_stem7_fwd called directly (no descriptor is looked up on the tensors)."""
    lib = _lib()
    n, ci, h, w = x.shape
    y = torch.empty(_y_shape(n, co, h, w, stride, pool), device=x.device)
    nb = lib.mphip_conv2d_stem7_workspace_bytes(n, ci, co, h, w, stride, int(pool))
    wsb = torch.empty((nb + 3) // 4, device=x.device) if ws == "auto" else ws
    rc = lib.mphip_conv2d_stem7_fwd(_p(x), _p(x_range), _p(wp), _p(bias), _p(y), _p(out_range), n, ci, co, h, w, stride, int(relu), int(pool),
                                    _p(wsb), 0 if wsb is None else wsb.numel() * 4, _stream())
    assert rc == 0, lib.mphip_last_error()
    return y


def _range_max(rng):
    r = rng.view(torch.int32)
    n = int(r[3].item())
    assert rng[0].item() == 0.0 and 0 < n <= RANGE_FLOATS - 4
    return torch.cat([r[2:3], r[4:4 + n]]).max().view(1).view(torch.float32).item()


def _bits(t):
    return t.contiguous().view(torch.int32)


# (N, Co, H, W).  1x1: every tap but one is padding; 5x7: narrower than the window; 17x19: crosses a tile, ragged, odd Ho and Wo at stride 2
# (a ragged pool); 16x20 with 48 channels: a partial channel tile; 33x35: three tiles each way, two images
INT_CASES = [(1, 16, 1, 1), (2, 32, 5, 7), (1, 64, 17, 19), (1, 48, 16, 20), (2, 64, 33, 35)]


@pytest.mark.parametrize("stride", [1, 2], ids=["s1", "s2"])
@pytest.mark.parametrize("shape,offset", [(s, False) for s in INT_CASES] + [(s, True) for s in INT_CASES[1:3]],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else ("plus4bytes" if v else "aligned"))
def test_integer_data_is_bit_exact(shape, offset, stride):
    from megaportrait_hack_amd import ops

    lib = _lib()
    n, co, h, w = shape
    x, wt, b = _ints((n, 3, h, w), -4, 4, 1), _ints((co, 3, 7, 7), -2, 2, 2), _ints((co,), -8, 8, 3)
    xg = _misaligned(x.to(DEV)) if offset else x.to(DEV)
    pack = ops.PackedConv2dStem7(wt.to(DEV), b.to(DEV))
    ops.f16x3_saturation_count(reset=True)
    for relu in (False, True):
        for pool in (False, True):
            assert lib.mphip_conv2d_stem7_supported(n, 3, co, h, w, stride, int(pool)) == 1
            assert ops.conv2d_stem7_supported(n, 3, co, h, w, stride, pool)
            want = _oracle(x, wt, b, stride, relu, pool).float()
            assert want.abs().max() < 2 ** 24
            got = ops.conv2d_stem7(xg, pack, stride=stride, relu=relu, pool=pool)
            assert got.shape == want.shape == _y_shape(n, co, h, w, stride, pool) and got.dtype == torch.float32
            assert torch.equal(got.cpu(), want), (shape, stride, relu, pool, (got.cpu() - want).abs().max().item())
    assert ops.f16x3_saturation_count() == 0


IDENTITY_CASES = [(2, 64, 19, 35), (1, 32, 33, 32), (2, 16, 5, 7)]


def _random_case(shape, seed):
    n, co, h, w = shape
    return (_rand((n, 3, h, w), seed, 2.0).to(DEV), _rand((co, 3, 7, 7), seed + 1, 0.1).to(DEV), _rand((co,), seed + 2).to(DEV))


@pytest.mark.parametrize("shape", IDENTITY_CASES, ids=_ids)
def test_stride2_is_the_even_subsample_of_stride1_bitwise(shape):
    from megaportrait_hack_amd import ops

    x, wt, b = _random_case(shape, 61)
    pack = ops.PackedConv2dStem7(wt, b)
    desc = ops.absmax_range(x.clone())
    for relu in (False, True):
        s1 = ops.conv2d_stem7(x, pack, stride=1, relu=relu, x_range=desc)
        s2 = ops.conv2d_stem7(x, pack, stride=2, relu=relu, x_range=desc)
        assert torch.equal(_bits(s2), _bits(s1[:, :, ::2, ::2])), (shape, relu)


@pytest.mark.parametrize("stride", [1, 2], ids=["s1", "s2"])
@pytest.mark.parametrize("shape", IDENTITY_CASES, ids=_ids)
def test_the_pool_is_max_pool2d_bitwise(shape, stride):
    from megaportrait_hack_amd import ops

    x, wt, b = _random_case(shape, 71)
    desc = ops.absmax_range(x.clone())
    special = b.clone()      # NaN and +-Inf through the bias: whole channels, the operand scaling is not involved
    special[1], special[2], special[3] = float("nan"), float("inf"), float("-inf")
    for bias in (b, special):
        pack = ops.PackedConv2dStem7(wt, bias)
        for relu in (False, True):
            flat = ops.conv2d_stem7(x, pack, stride=stride, relu=relu, x_range=desc)
            if not relu:
                assert not bool((flat == 0).any())      # no zero sums: the sign of a pooled zero is left open without ReLU
            want = F.max_pool2d(flat, 3, 2, 1)
            got = ops.conv2d_stem7(x, pack, stride=stride, relu=relu, pool=True, x_range=desc)
            assert got.shape == want.shape
            nan = torch.isnan(want)
            assert torch.equal(torch.isnan(got), nan), (shape, stride, relu)
            assert bool(nan[:, 1].all()) == (bias is special)
            assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), (shape, stride, relu)


@pytest.mark.parametrize("stride", [1, 2], ids=["s1", "s2"])
def test_translation(stride):
    """An h x w image in a zero canvas, moved across tile boundaries: zero padding and canvas zeros stage the same operands."""
    from megaportrait_hack_amd import ops

    n, co, h, w = 2, 32, 9, 11
    x, wt, b = _random_case((n, co, h, w), 81)
    pack = ops.PackedConv2dStem7(wt, b)
    desc = ops.absmax_range(x.clone())
    small = ops.conv2d_stem7(x, pack, stride=stride, x_range=desc)
    # a window that leaves the image sees the canvas's zeros where the small image had padding: the same operands, so the WHOLE small map
    # is compared; the offsets put the image inside one tile, across a tile corner, and one tile further (even ones at stride 2)
    for oy, ox in ((0, 0), (3, 5), (13, 16)) if stride == 1 else ((0, 0), (4, 6), (14, 16)):
        canvas = torch.zeros(n, 3, 40, 44, device=DEV)
        canvas[:, :, oy:oy + h, ox:ox + w] = x
        big = ops.conv2d_stem7(canvas, pack, stride=stride, x_range=desc)
        sy, sx = oy // stride, ox // stride
        assert torch.equal(_bits(big[:, :, sy:sy + small.shape[2], sx:sx + small.shape[3]]), _bits(small)), (stride, oy, ox)


ACC_CASES = [((2, 64, 40, 56), 1, False, False), ((2, 64, 40, 56), 2, False, False), ((1, 64, 33, 35), 2, True, True)]
_PARITY = []


@pytest.mark.parametrize("xscale", [1.0, 1e4, 1e-4])
@pytest.mark.parametrize("shape,stride,relu,pool", ACC_CASES, ids=lambda v: _ids(v) if isinstance(v, tuple) else str(int(v)))
def test_random_data_accuracy(shape, stride, relu, pool, xscale):
    from megaportrait_hack_amd import ops

    n, co, h, w = shape
    x, wt, b = _rand((n, 3, h, w), 11, xscale), _rand((co, 3, 7, 7), 12, 0.05), _rand((co,), 13, xscale)
    y64 = _oracle(x, wt, b, stride, relu, pool)
    A = F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), stride=stride, padding=3).max().item()
    xg, wg, bg = x.to(DEV), wt.to(DEV), b.to(DEV)
    cudnn, mm = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        yt = F.conv2d(xg, wg, bg, stride=stride, padding=3)
        if relu:
            yt = F.relu(yt)
        if pool:
            yt = F.max_pool2d(yt, 3, 2, 1)
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = cudnn, mm
    ops.f16x3_saturation_count(reset=True)
    yh = ops.conv2d_stem7(xg, ops.PackedConv2dStem7(wg, bg), stride=stride, relu=relu, pool=pool)
    e_torch = (yt.cpu().double() - y64).abs().max().item()
    e_hip = (yh.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -21 * A
    print(f"conv2d_stem7 parity {shape} stride {stride} relu {relu} pool {pool} x*{xscale:g}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} "
          f"A={A:.3e} bound={bound:.3e} ratio={e_hip / bound:.3f}")
    _PARITY.append({"shape_N_Co_H_W": list(shape), "stride": stride, "relu": relu, "pool": pool, "x_scale": xscale,
                    "e_hip": float(f"{e_hip:.4g}"), "e_torch": float(f"{e_torch:.4g}"), "A": float(f"{A:.4g}"),
                    "bound": float(f"{bound:.4g}"), "e_hip_over_bound": float(f"{e_hip / bound:.4g}")})
    out = os.environ.get("MPHIP_PARITY_JSON")      # the measured values, for profiles/conv2d_stem7_parity.json
    if out and len(_PARITY) == 3 * len(ACC_CASES):
        with open(out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "bar": "e_hip <= 4 * e_torch + 2^-21 * A", "cases": _PARITY}, f, indent=1)
    assert e_hip <= bound
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("stride,pool", [(1, False), (2, True)], ids=["s1", "s2pool"])
def test_ranges_are_exact_and_interchangeable(stride, pool):
    from megaportrait_hack_amd import ops

    n, co, h, w = 2, 64, 37, 50
    x, wt, b = _random_case((n, co, h, w), 21)
    w2, b2 = _rand((32, co, 3, 3), 24, 0.1).to(DEV), _rand((32,), 25).to(DEV)
    wp = _pack(wt)
    desc = ops.absmax_range(x.clone())
    y_null = _fwd(x, wp, b, co, stride, True, pool)                                  # the library scans x into the workspace
    y_desc = _fwd(x, wp, b, co, stride, True, pool, x_range=desc, ws=None)           # no workspace needed with a descriptor
    assert torch.equal(y_null, y_desc)
    out_range = torch.full((RANGE_FLOATS,), 1.0e30, device=DEV)                      # poisoned: the launch must initialise what it uses
    y = _fwd(x, wp, b, co, stride, False, pool, out_range=out_range)
    assert torch.equal(y, _fwd(x, wp, b, co, stride, False, pool))
    assert _range_max(out_range) == y.abs().max().item()
    # ops.conv2d_stem7: a scan tags x, want_range tags the result, the next conv2d picks the tag up
    p1, p2 = ops.PackedConv2dStem7(wt, b), ops.PackedConv2d(w2, b2)
    x2 = x.clone()
    assert ops.tensor_range(x2) is None
    yt = ops.conv2d_stem7(x2, p1, stride=stride, pool=pool, want_range=True)
    assert ops.tensor_range(x2) is not None      # the second stem of the same image does not scan it again
    assert ops.tensor_range(yt) is not None and torch.equal(yt, y)
    assert torch.equal(ops.conv2d(yt, p2), ops.conv2d(y.clone(), p2))
    assert ops.tensor_range(ops.conv2d_stem7(x2, p1, stride=stride, pool=pool)) is None


def test_argument_rules():
    """Each refusal returns its code before anything is launched: y, pre-filled with a sentinel, is untouched.  The order is the 2-D
    entries': null pointer, shape, alignment, aliasing, then the workspace."""
    from megaportrait_hack_amd import ops

    lib = _lib()
    t = torch.zeros(1 << 16, device=DEV)
    y = torch.full((1 << 14,), 7.0, device=DEV)
    args = lambda n, ci, co, h, w, s, pool, x=t, wp=t, b=t, y=y, ws=t, wsb=1 << 18: (
        _p(x), None, _p(wp), _p(b), _p(y), None, n, ci, co, h, w, s, 0, pool, _p(ws), wsb, _stream())
    for shape in [(1, 4, 32, 8, 8, 1, 0), (1, 3, 24, 8, 8, 1, 0), (1, 3, 80, 8, 8, 1, 0), (1, 3, 0, 8, 8, 1, 0), (1, 3, 32, 0, 8, 2, 1),
                  (0, 3, 32, 8, 8, 1, 0), (1, 3, 16, 1 << 15, 1 << 16, 2, 1), (1, 3, 32, 8, 8, 0, 0), (1, 3, 32, 8, 8, 3, 0)]:
        assert lib.mphip_conv2d_stem7_supported(*shape) == 0 and lib.mphip_conv2d_stem7_workspace_bytes(*shape) == 0
        assert not ops.conv2d_stem7_supported(*shape)
        assert lib.mphip_conv2d_stem7_fwd(*args(*shape)) == EINVAL
        assert b"conv2d_stem7_fwd: unsupported shape" in lib.mphip_last_error()
    ok = (1, 3, 32, 8, 8, 2, 0)      # x: 192 elements, y: 32 x 4 x 4 = 512
    assert lib.mphip_conv2d_stem7_supported(*ok) == 1
    for missing in ("x", "wp", "b", "y"):
        assert lib.mphip_conv2d_stem7_fwd(*args(*ok, **{missing: None})) == EINVAL and b"conv2d_stem7_fwd: null" in lib.mphip_last_error()
    assert lib.mphip_conv2d_stem7_fwd(*args(1, 3, 32, 8, 8, 3, 0, b=None)) == EINVAL and b"conv2d_stem7_fwd: null" in lib.mphip_last_error()
    assert lib.mphip_conv2d_stem7_fwd(*args(1, 3, 24, 8, 8, 1, 0, wp=t[1:])) == EINVAL and b"unsupported shape" in lib.mphip_last_error()
    assert lib.mphip_conv2d_stem7_fwd(*args(*ok, wp=t[1:])) == EINVAL and b"16-byte aligned" in lib.mphip_last_error()
    assert lib.mphip_conv2d_stem7_fwd(*args(*ok, wp=t[1:], x=y)) == EINVAL and b"16-byte aligned" in lib.mphip_last_error()   # before aliasing
    assert lib.mphip_conv2d_stem7_fwd(*args(*ok, x=y)) == EINVAL and b"must not alias" in lib.mphip_last_error()             # y is x
    assert lib.mphip_conv2d_stem7_fwd(*args(*ok, x=y[511:])) == EINVAL and b"must not alias" in lib.mphip_last_error()       # one element shared
    assert lib.mphip_conv2d_stem7_fwd(*args(*ok, x=y[512:])) == 0, lib.mphip_last_error()      # extents from Ho*Wo: these only touch
    y[:512] = 7.0
    pooled = (1, 3, 32, 8, 8, 2, 1)  # pooled y is 32 x 2 x 2 = 128 elements
    assert lib.mphip_conv2d_stem7_fwd(*args(*pooled, x=y[127:])) == EINVAL and b"must not alias" in lib.mphip_last_error()
    need = lib.mphip_conv2d_stem7_workspace_bytes(*ok)
    assert need >= RANGE_FLOATS * 4
    assert lib.mphip_conv2d_stem7_fwd(*args(*ok, wsb=need - 4)) == EWORKSPACE and b"conv2d_stem7_fwd: workspace" in lib.mphip_last_error()
    assert lib.mphip_conv2d_stem7_fwd(*args(*ok, ws=None, wsb=0)) == EWORKSPACE
    assert lib.mphip_conv2d_stem7_fwd(*args(*ok, b=None, wsb=need - 4)) == EINVAL      # the argument error wins
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    pk = ops.PackedConv2dStem7(torch.zeros(32, 3, 7, 7, device=DEV), torch.zeros(32, device=DEV))
    with pytest.raises(RuntimeError, match="image"):
        ops.conv2d_stem7(torch.zeros(1, 4, 8, 8, device=DEV), pk)
    with pytest.raises(RuntimeError, match="stride"):
        ops.conv2d_stem7(torch.zeros(1, 3, 8, 8, device=DEV), pk, stride=3)
    with pytest.raises(RuntimeError, match="PackedConv2dStem7"):
        ops.conv2d_stem7(torch.zeros(1, 3, 8, 8, device=DEV), ops.PackedConv2d(torch.zeros(32, 16, 3, 3, device=DEV), torch.zeros(32, device=DEV)))
    with pytest.raises(RuntimeError):
        ops.PackedConv2dStem7(torch.zeros(80, 3, 7, 7, device=DEV), torch.zeros(80, device=DEV))
    torch.cuda.synchronize()
