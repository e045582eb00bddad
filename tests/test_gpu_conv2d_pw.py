"""The 2-D pointwise (1x1) conv at stride 1 and 2 on the matrix cores (csrc/conv2d_pw_f16x3.hip: mphip_conv2d_pw_supported,
mphip_conv2d_pw_packed_weight_bytes, mphip_pack_conv2d_pw_weight, mphip_conv2d_pw_workspace_bytes, mphip_conv2d_pw_fwd), with the
conventions of tests/test_gpu_conv2d_s2.py.

Integer data makes every product and partial sum an exact fp32 value (|sum| <= 64*8 + 16 < 2^24, power-of-two scales, every lo half 0),
so those cases are compared with torch.equal against the fp64 oracle F.conv2d(..., stride=s).  Two contracts pin the arithmetic on random
data: with the same x, descriptor and bias the launch writes the bits of the 3x3 kernels fed the weight whose only non-zero tap is the
centre (mphip_conv2d_fwd at stride 1, mphip_conv2d_s2_fwd at stride 2), and the stride-2 launch writes the bits of the stride-1 launch at
the even rows and columns.  Random data is also held to the project's bar 4*e_torch + 2^-21*A (A = max over outputs of sum |w||x| +
|bias| + |residual|) against torch's fp32 conv on the same GPU with TF32 off."""
import ctypes

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


def _out(h, w, s):
    return (h + s - 1) // s, (w + s - 1) // s


def _oracle(x, w, b, res, relu, s):
    y = F.conv2d(x.double(), w.double(), b.double(), stride=s)
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


def _centre(w):
    """The 3x3 weight whose only non-zero tap is the centre: the same max|w|, so the same pack scale."""
    w3 = torch.zeros(*w.shape[:2], 3, 3, device=w.device)
    w3[:, :, 1, 1] = w[:, :, 0, 0]
    return w3


def _pack(w):
    """mphip_pack_conv2d_pw_weight of a [Co,Ci,1,1] weight, mphip_pack_conv2d_weight of a [Co,Ci,3,3] one."""
    lib = _lib()
    co, ci = w.shape[:2]
    size, pack = ((lib.mphip_conv2d_pw_packed_weight_bytes, lib.mphip_pack_conv2d_pw_weight) if w.shape[2] == 1 else
                  (lib.mphip_conv2d_packed_weight_bytes, lib.mphip_pack_conv2d_weight))
    nb = size(co, ci)
    assert nb > 0
    wp = torch.empty((nb + 3) // 4, device=w.device)
    assert pack(_p(w), _p(wp), co, ci, _stream()) == 0, lib.mphip_last_error()
    return wp


def _fwd(entry, x, wp, bias, co, res=None, relu=False, x_range=None, out_range=None, ws="auto", stride=1):
    """mphip_conv2d_pw_fwd (entry "pw") or mphip_conv2d_fwd ("k3") called directly (no descriptor is looked up on the tensors)."""
    lib = _lib()
    n, ci, h, w = x.shape
    if entry == "pw":
        y = torch.empty((n, co, *_out(h, w, stride)), device=x.device)
        nb = lib.mphip_conv2d_pw_workspace_bytes(n, ci, co, h, w, stride)
        wsb = torch.empty((nb + 3) // 4, device=x.device) if ws == "auto" else ws
        rc = lib.mphip_conv2d_pw_fwd(_p(x), _p(x_range), _p(wp), _p(bias), _p(res), _p(y), _p(out_range), n, ci, co, h, w, stride, int(relu),
                                     _p(wsb), 0 if wsb is None else wsb.numel() * 4, _stream())
    else:
        y = torch.empty((n, co, h, w), device=x.device)
        nb = lib.mphip_conv2d_workspace_bytes(n, ci, co, h, w)
        wsb = torch.empty((nb + 3) // 4, device=x.device) if ws == "auto" else ws
        rc = lib.mphip_conv2d_fwd(_p(x), _p(x_range), _p(wp), _p(bias), _p(res), _p(y), _p(out_range), n, ci, co, h, w, int(relu), _p(wsb),
                                  0 if wsb is None else wsb.numel() * 4, _stream())
    assert rc == 0, lib.mphip_last_error()
    return y


def _range_max(rng):
    r = rng.view(torch.int32)
    n = int(r[3].item())
    assert rng[0].item() == 0.0 and 0 < n <= RANGE_FLOATS - 4
    return torch.cat([r[2:3], r[4:4 + n]]).max().view(1).view(torch.float32).item()


# (1,1): one pixel, a half-empty channel tile; (5,7): H*W = 35, the 4-byte path, ragged; 17x19: 323 pixels cross a 256-pixel tile, two
# chunks, a partial second channel tile; 16x20: the 16-byte path with a partial second pixel tile; 16x16: full tiles
INT_CASES = [(1, 16, 32, 1, 1), (2, 16, 32, 5, 7), (1, 32, 96, 17, 19), (1, 48, 64, 16, 20), (2, 64, 128, 16, 16)]


@pytest.mark.parametrize("stride", [1, 2], ids=["s1", "s2"])
@pytest.mark.parametrize("shape,offset", [(s, False) for s in INT_CASES] + [(s, True) for s in INT_CASES[:2]],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("plus4bytes" if v else "aligned"))
def test_integer_data_is_bit_exact(shape, offset, stride):
    from megaportrait_hack_amd import ops

    lib = _lib()
    n, ci, co, h, w = shape
    ho, wo = _out(h, w, stride)
    assert lib.mphip_conv2d_pw_supported(*shape, stride) == 1 and ops.conv2d_pw_supported(*shape, stride)
    x, wt = _ints((n, ci, h, w), -4, 4, 1), _ints((co, ci, 1, 1), -2, 2, 2)
    b, res = _ints((co,), -8, 8, 3), _ints((n, co, ho, wo), -8, 8, 4)
    xg, rg = x.to(DEV), res.to(DEV)
    if offset:
        xg, rg = _misaligned(xg), _misaligned(rg)
    pack = ops.PackedConv2dPW(wt.to(DEV), b.to(DEV))
    ops.f16x3_saturation_count(reset=True)
    for relu in (False, True):
        for with_res in (False, True):
            want = _oracle(x, wt, b, res if with_res else None, relu, stride).float()
            assert want.abs().max() < 2 ** 24
            got = ops.conv2d_pw(xg, pack, residual=rg if with_res else None, relu=relu, stride=stride)
            assert got.shape == want.shape == (n, co, ho, wo) and got.dtype == torch.float32
            assert torch.equal(got.cpu(), want), (shape, stride, relu, with_res, (got.cpu() - want).abs().max().item())
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("shape", [(2, 32, 64, 19, 35), (1, 64, 128, 33, 32)], ids=lambda s: "x".join(map(str, s)))
def test_centre_tap_of_the_3x3_kernels_bitwise(shape):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = shape
    x, wt, b = _rand((n, ci, h, w), 51, 2.0).to(DEV), _rand((co, ci, 1, 1), 52, 0.1).to(DEV), _rand((co,), 53).to(DEV)
    res = _rand((n, co, h, w), 54).to(DEV)
    sub = res[:, :, ::2, ::2].contiguous()
    p1, p3 = ops.PackedConv2dPW(wt, b), ops.PackedConv2d(_centre(wt), b)
    assert p1.pointwise and not p3.pointwise
    assert torch.equal(p1.packed()[:4], p3.packed()[:4])     # the header: the same function of the same max|w|
    for relu in (False, True):      # both calls scan x
        assert torch.equal(ops.conv2d_pw(x, p1, relu=relu), ops.conv2d(x, p3, relu=relu))
        assert torch.equal(ops.conv2d_pw(x, p1, relu=relu, stride=2), ops.conv2d_s2(x, p3, relu=relu))
    assert torch.equal(ops.conv2d_pw(x, p1, residual=res, relu=True), ops.conv2d(x, p3, residual=res, relu=True))
    assert torch.equal(ops.conv2d_pw(x, p1, residual=sub, relu=True, stride=2), ops.conv2d_s2(x, p3, residual=sub, relu=True))
    desc = ops.absmax_range(x.clone())      # one explicit descriptor for all
    a = ops.conv2d_pw(x, p1, relu=True, x_range=desc)
    assert torch.equal(a, ops.conv2d(x, p3, relu=True, x_range=desc)) and torch.equal(a, ops.conv2d_pw(x, p1, relu=True))
    a2 = ops.conv2d_pw(x, p1, relu=True, stride=2, x_range=desc)
    assert torch.equal(a2, ops.conv2d_s2(x, p3, relu=True, x_range=desc)) and torch.equal(a2, ops.conv2d_pw(x, p1, relu=True, stride=2))
    with pytest.raises(RuntimeError, match="1x1"):      # the layouts differ: neither wrapper takes the other's pack
        ops.conv2d(x, p1)
    with pytest.raises(RuntimeError, match="3x3"):
        ops.conv2d_pw(x, p3)


@pytest.mark.parametrize("shape", [(2, 32, 64, 19, 35), (1, 64, 128, 33, 32), (2, 16, 32, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_stride2_is_the_even_subsample_of_stride1_bitwise(shape):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = shape
    x, wt, b = _rand((n, ci, h, w), 61, 2.0).to(DEV), _rand((co, ci, 1, 1), 62, 0.1).to(DEV), _rand((co,), 63).to(DEV)
    res = _rand((n, co, h, w), 64).to(DEV)
    pack = ops.PackedConv2dPW(wt, b)
    for relu in (False, True):
        assert torch.equal(ops.conv2d_pw(x, pack, relu=relu, stride=2), ops.conv2d_pw(x, pack, relu=relu)[:, :, ::2, ::2])
    sub = res[:, :, ::2, ::2].contiguous()
    assert torch.equal(ops.conv2d_pw(x, pack, residual=sub, relu=True, stride=2),
                       ops.conv2d_pw(x, pack, residual=res, relu=True)[:, :, ::2, ::2])
    # the 16-byte and the 4-byte staging of the stride-1 launch give the same bits
    assert torch.equal(ops.conv2d_pw(_misaligned(x), pack, residual=res, relu=True), ops.conv2d_pw(x, pack, residual=res, relu=True))


# 64 -> 256 on 32x32: layer1's widening conv; 1024 -> 256 on 8x8: 64 chunks; 256 -> 512 at stride 2: layer2's downsample
ACC_CASES = [((2, 64, 256, 32, 32), 1), ((1, 1024, 256, 8, 8), 1), ((1, 256, 512, 16, 16), 2)]


@pytest.mark.parametrize("xscale", [1.0, 1e4, 1e-4])
@pytest.mark.parametrize("shape,stride", ACC_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"s{v}")
def test_random_data_accuracy(shape, stride, xscale):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = shape
    x, wt = _rand((n, ci, h, w), 11, xscale), _rand((co, ci, 1, 1), 12, 0.05)
    b, res = _rand((co,), 13, xscale), _rand((n, co, *_out(h, w, stride)), 14, xscale)
    y64 = _oracle(x, wt, b, res, True, stride)
    A = (F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), stride=stride) + res.double().abs()).max().item()
    xg, wg, bg, rg = x.to(DEV), wt.to(DEV), b.to(DEV), res.to(DEV)
    cudnn, mm = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        yt = F.relu(F.conv2d(xg, wg, bg, stride=stride) + rg)
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = cudnn, mm
    ops.f16x3_saturation_count(reset=True)
    yh = ops.conv2d_pw(xg, ops.PackedConv2dPW(wg, bg), residual=rg, relu=True, stride=stride)
    e_torch = (yt.cpu().double() - y64).abs().max().item()
    e_hip = (yh.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -21 * A
    print(f"conv2d_pw parity {shape} stride {stride} x*{xscale:g}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} A={A:.3e} bound={bound:.3e}")
    assert e_hip <= bound
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("stride", [1, 2], ids=["s1", "s2"])
def test_ranges_are_exact_and_interchangeable(stride):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = 2, 32, 64, 37, 50
    x, wt, b = _rand((n, ci, h, w), 21, 3.0).to(DEV), _rand((co, ci, 1, 1), 22, 0.1).to(DEV), _rand((co,), 23).to(DEV)
    w2, b2 = _rand((32, co, 3, 3), 24, 0.1).to(DEV), _rand((32,), 25).to(DEV)
    wp, wp2 = _pack(wt), _pack(w2)
    desc = ops.absmax_range(x.clone())
    y_null = _fwd("pw", x, wp, b, co, relu=True, stride=stride)
    y_desc = _fwd("pw", x, wp, b, co, relu=True, x_range=desc, ws=None, stride=stride)      # no workspace needed with a descriptor
    assert torch.equal(y_null, y_desc)
    out_range = torch.full((RANGE_FLOATS,), 1.0e30, device=DEV)                   # poisoned: the launch must initialise what it uses
    y = _fwd("pw", x, wp, b, co, relu=False, out_range=out_range, stride=stride)
    assert torch.equal(y, _fwd("pw", x, wp, b, co, relu=False, stride=stride))
    assert _range_max(out_range) == y.abs().max().item()
    z_fed = _fwd("k3", y, wp2, b2, 32, x_range=out_range, ws=None)
    z_null = _fwd("k3", y, wp2, b2, 32)
    assert torch.equal(z_fed, z_null)
    # ops.conv2d_pw: want_range tags the result, the next conv2d picks the tag up
    p1, p2 = ops.PackedConv2dPW(wt, b), ops.PackedConv2d(w2, b2)
    yt = ops.conv2d_pw(x, p1, stride=stride, want_range=True)
    assert ops.tensor_range(yt) is not None and torch.equal(yt, y) and torch.equal(ops.conv2d(yt, p2), z_null)
    assert ops.tensor_range(ops.conv2d_pw(x, p1, stride=stride)) is None


def test_argument_rules():
    """Each refusal returns its code before anything is launched: y, pre-filled with a sentinel, is untouched."""
    from megaportrait_hack_amd import ops

    lib = _lib()
    t = torch.zeros(1 << 16, device=DEV)
    y = torch.full((1 << 14,), 7.0, device=DEV)
    args = lambda n, ci, co, h, w, s, x=t, wp=t, b=t, res=None, y=y, ws=t, wsb=1 << 18: (
        _p(x), None, _p(wp), _p(b), _p(res), _p(y), None, n, ci, co, h, w, s, 0, _p(ws), wsb, _stream())
    for shape in [(1, 8, 32, 8, 8, 1), (1, 16, 48, 8, 8, 1), (1, 16, 32, 0, 8, 2), (0, 16, 32, 8, 8, 1), (1, 16, 32, 1 << 15, 1 << 16, 2),
                  (1, 16, 32, 8, 8, 0), (1, 16, 32, 8, 8, 3), (1, 16, 32, 8, 8, -1)]:
        assert lib.mphip_conv2d_pw_supported(*shape) == 0 and lib.mphip_conv2d_pw_workspace_bytes(*shape) == 0
        assert not ops.conv2d_pw_supported(*shape)
        assert lib.mphip_conv2d_pw_fwd(*args(*shape)) == EINVAL
        assert b"conv2d_pw_fwd: unsupported shape" in lib.mphip_last_error()
    ok = (1, 16, 32, 8, 8, 2)      # x: 1024 elements, y: 32 x 4 x 4 = 512
    assert lib.mphip_conv2d_pw_supported(*ok) == 1
    for missing in ("x", "wp", "b", "y"):
        assert lib.mphip_conv2d_pw_fwd(*args(*ok, **{missing: None})) == EINVAL and b"conv2d_pw_fwd: null" in lib.mphip_last_error()
    assert lib.mphip_conv2d_pw_fwd(*args(1, 16, 32, 8, 8, 3, b=None)) == EINVAL and b"conv2d_pw_fwd: null" in lib.mphip_last_error()   # the shared order
    assert lib.mphip_conv2d_pw_fwd(*args(*ok, wp=t[1:])) == EINVAL and b"16-byte aligned" in lib.mphip_last_error()
    assert lib.mphip_conv2d_pw_fwd(*args(*ok, x=y)) == EINVAL and b"must not alias" in lib.mphip_last_error()           # y is x
    assert lib.mphip_conv2d_pw_fwd(*args(*ok, res=y[511:])) == EINVAL and b"must not alias" in lib.mphip_last_error()   # one element shared
    assert lib.mphip_conv2d_pw_fwd(*args(*ok, x=y[512:], res=y[1536:])) == 0, lib.mphip_last_error()   # extents from Ho*Wo: these only touch
    y[:512] = 7.0
    s1 = (1, 16, 32, 8, 8, 1)      # at stride 1 y is 2048 elements: the same residual now overlaps it
    assert lib.mphip_conv2d_pw_fwd(*args(*s1, res=y[1536:])) == EINVAL and b"must not alias" in lib.mphip_last_error()
    need = lib.mphip_conv2d_pw_workspace_bytes(*ok)
    assert need >= RANGE_FLOATS * 4
    assert lib.mphip_conv2d_pw_fwd(*args(*ok, wsb=need - 4)) == EWORKSPACE and b"conv2d_pw_fwd: workspace" in lib.mphip_last_error()
    assert lib.mphip_conv2d_pw_fwd(*args(*ok, ws=None, wsb=0)) == EWORKSPACE
    assert lib.mphip_conv2d_pw_fwd(*args(*ok, b=None, wsb=need - 4)) == EINVAL      # the argument error wins
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    pw = ops.PackedConv2dPW(torch.zeros(32, 16, 1, 1, device=DEV), torch.zeros(32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.conv2d_pw(torch.zeros(1, 32, 8, 8, device=DEV), pw)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.conv2d_pw(torch.zeros(1, 16, 8, 8, device=DEV), pw, stride=3)
    with pytest.raises(RuntimeError, match="residual"):
        ops.conv2d_pw(torch.zeros(1, 16, 8, 8, device=DEV), pw, residual=torch.zeros(1, 32, 8, 8, device=DEV), stride=2)
    torch.cuda.synchronize()
