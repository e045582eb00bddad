"""The 2-D 3x3 conv at stride 2 on the matrix cores (csrc/conv2d_s2_f16x3.hip: mphip_conv2d_s2_supported,
mphip_conv2d_s2_workspace_bytes, mphip_conv2d_s2_fwd), with the conventions of tests/test_gpu_conv2d_f16x3.py.

Integer data makes every product and partial sum an exact fp32 value (|sum| <= 9*64*8 + 16 < 2^24, power-of-two scales, every lo half 0),
so those cases are compared with torch.equal against the fp64 oracle F.conv2d(..., stride=2, padding=1).  The contract that pins the
arithmetic on random data: with the same x, descriptor, pack and bias the launch writes the bits of mphip_conv2d_fwd's output at the even
rows and columns.  Random data is also held to the project's bar 4*e_torch + 2^-21*A (A = max over outputs of sum |w||x| + |bias| +
|residual|) against torch's fp32 stride-2 conv on the same GPU."""
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


def _out(h, w):
    return (h + 1) // 2, (w + 1) // 2


def _oracle(x, w, b, res, relu):
    y = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)
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


def _pack(w):
    lib = _lib()
    co, ci = w.shape[:2]
    nb = lib.mphip_conv2d_packed_weight_bytes(co, ci)
    assert nb > 0
    wp = torch.empty((nb + 3) // 4, device=w.device)
    assert lib.mphip_pack_conv2d_weight(_p(w), _p(wp), co, ci, _stream()) == 0, lib.mphip_last_error()
    return wp


def _fwd(entry, x, wp, bias, co, res=None, relu=False, x_range=None, out_range=None, ws="auto"):
    """mphip_conv2d_s2_fwd (entry "s2") or mphip_conv2d_fwd ("s1") called directly (no descriptor is looked up on the tensors)."""
    lib = _lib()
    n, ci, h, w = x.shape
    ho, wo = _out(h, w) if entry == "s2" else (h, w)
    y = torch.empty((n, co, ho, wo), device=x.device)
    fn, wsfn = (lib.mphip_conv2d_s2_fwd, lib.mphip_conv2d_s2_workspace_bytes) if entry == "s2" else (lib.mphip_conv2d_fwd, lib.mphip_conv2d_workspace_bytes)
    nb = wsfn(n, ci, co, h, w)
    wsb = torch.empty((nb + 3) // 4, device=x.device) if ws == "auto" else ws
    rc = fn(_p(x), _p(x_range), _p(wp), _p(bias), _p(res), _p(y), _p(out_range), n, ci, co, h, w, int(relu), _p(wsb),
            0 if wsb is None else wsb.numel() * 4, _stream())
    assert rc == 0, lib.mphip_last_error()
    return y


def _range_max(rng):
    r = rng.view(torch.int32)
    n = int(r[3].item())
    assert rng[0].item() == 0.0 and 0 < n <= RANGE_FLOATS - 4
    return torch.cat([r[2:3], r[4:4 + n]]).max().view(1).view(torch.float32).item()


# (1,1) and (2,2): one output pixel; (5,7): the last output row and column read the padding; (4,6): they do not; 33x31: Ho = 17 crosses
# a tile row, two chunks, a half-empty second co tile; 34x70: Wo = 35, three tile columns
INT_CASES = [(1, 16, 32, 1, 1), (1, 16, 32, 2, 2), (2, 16, 32, 5, 7), (1, 16, 32, 4, 6), (1, 32, 96, 33, 31), (1, 48, 64, 34, 70),
             (1, 64, 128, 16, 16)]


@pytest.mark.parametrize("shape,offset", [(s, False) for s in INT_CASES] + [(s, True) for s in INT_CASES[:2]],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("plus4bytes" if v else "aligned"))
def test_integer_data_is_bit_exact(shape, offset):
    from megaportrait_hack_amd import ops

    lib = _lib()
    n, ci, co, h, w = shape
    ho, wo = _out(h, w)
    assert lib.mphip_conv2d_s2_supported(*shape) == 1 and ops.conv2d_s2_supported(*shape)
    x, wt = _ints((n, ci, h, w), -4, 4, 1), _ints((co, ci, 3, 3), -2, 2, 2)
    b, res = _ints((co,), -8, 8, 3), _ints((n, co, ho, wo), -8, 8, 4)
    xg, rg = x.to(DEV), res.to(DEV)
    if offset:
        xg, rg = _misaligned(xg), _misaligned(rg)
    pack = ops.PackedConv2d(wt.to(DEV), b.to(DEV))
    ops.f16x3_saturation_count(reset=True)
    for relu in (False, True):
        for with_res in (False, True):
            want = _oracle(x, wt, b, res if with_res else None, relu).float()
            assert want.abs().max() < 2 ** 24
            got = ops.conv2d_s2(xg, pack, residual=rg if with_res else None, relu=relu)
            assert got.shape == want.shape == (n, co, ho, wo) and got.dtype == torch.float32
            assert torch.equal(got.cpu(), want), (shape, relu, with_res, (got.cpu() - want).abs().max().item())
    assert ops.f16x3_saturation_count() == 0


def test_zero_padding_counts_the_taps():
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = 1, 16, 32, 19, 35      # 10 x 18 outputs: two tile rows, two tile columns; odd sizes: padding on every side
    pack = ops.PackedConv2d(torch.ones(co, ci, 3, 3, device=DEV), torch.zeros(co, device=DEV))
    y = ops.conv2d_s2(torch.ones(n, ci, h, w, device=DEV), pack).cpu()
    taps = F.conv2d(torch.ones(1, 1, h, w), torch.ones(1, 1, 3, 3), stride=2, padding=1)
    assert taps[0, 0, 0, 0] == 4 and taps[0, 0, 0, 1] == 6 and taps[0, 0, 5, 5] == 9 and taps[0, 0, 9, 17] == 4
    assert torch.equal(y, (ci * taps).expand(n, co, *_out(h, w)))


@pytest.mark.parametrize("shape", [(2, 32, 64, 19, 35), (1, 64, 128, 33, 32)], ids=lambda s: "x".join(map(str, s)))
def test_stride2_is_the_even_subsample_of_stride1_bitwise(shape):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = shape
    x, wt, b = _rand((n, ci, h, w), 51, 2.0).to(DEV), _rand((co, ci, 3, 3), 52, 0.1).to(DEV), _rand((co,), 53).to(DEV)
    res = _rand((n, co, h, w), 54).to(DEV)
    pack = ops.PackedConv2d(wt, b)
    for relu in (False, True):      # both calls scan x
        assert torch.equal(ops.conv2d_s2(x, pack, relu=relu), ops.conv2d(x, pack, relu=relu)[:, :, ::2, ::2])
    sub = res[:, :, ::2, ::2].contiguous()
    assert torch.equal(ops.conv2d_s2(x, pack, residual=sub, relu=True), ops.conv2d(x, pack, residual=res, relu=True)[:, :, ::2, ::2])
    desc = ops.absmax_range(x.clone())      # one explicit descriptor for both
    a, c = ops.conv2d_s2(x, pack, relu=True, x_range=desc), ops.conv2d(x, pack, relu=True, x_range=desc)[:, :, ::2, ::2]
    assert torch.equal(a, c) and torch.equal(a, ops.conv2d_s2(x, pack, relu=True))


@pytest.mark.parametrize("xscale", [1.0, 1e4, 1e-4])
@pytest.mark.parametrize("shape", [(2, 64, 128, 32, 32), (1, 256, 512, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_random_data_accuracy(shape, xscale):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = shape
    x, wt = _rand((n, ci, h, w), 11, xscale), _rand((co, ci, 3, 3), 12, 0.05)
    b, res = _rand((co,), 13, xscale), _rand((n, co, *_out(h, w)), 14, xscale)
    y64 = _oracle(x, wt, b, res, True)
    A = (F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), stride=2, padding=1) + res.double().abs()).max().item()
    xg, wg, bg, rg = x.to(DEV), wt.to(DEV), b.to(DEV), res.to(DEV)
    cudnn = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        yt = F.relu(F.conv2d(xg, wg, bg, stride=2, padding=1) + rg)
    finally:
        torch.backends.cudnn.allow_tf32 = cudnn
    ops.f16x3_saturation_count(reset=True)
    yh = ops.conv2d_s2(xg, ops.PackedConv2d(wg, bg), residual=rg, relu=True)
    e_torch = (yt.cpu().double() - y64).abs().max().item()
    e_hip = (yh.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -21 * A
    print(f"conv2d_s2 parity {shape} x*{xscale:g}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} A={A:.3e} bound={bound:.3e}")
    assert e_hip <= bound
    assert ops.f16x3_saturation_count() == 0


def test_ranges_are_exact_and_interchangeable():
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = 2, 32, 64, 37, 50
    x, wt, b = _rand((n, ci, h, w), 21, 3.0).to(DEV), _rand((co, ci, 3, 3), 22, 0.1).to(DEV), _rand((co,), 23).to(DEV)
    w2, b2 = _rand((32, co, 3, 3), 24, 0.1).to(DEV), _rand((32,), 25).to(DEV)
    wp, wp2 = _pack(wt), _pack(w2)
    desc = ops.absmax_range(x.clone())
    y_null = _fwd("s2", x, wp, b, co, relu=True)
    y_desc = _fwd("s2", x, wp, b, co, relu=True, x_range=desc, ws=None)            # no workspace needed with a descriptor
    assert torch.equal(y_null, y_desc)
    out_range = torch.full((RANGE_FLOATS,), 1.0e30, device=DEV)                   # poisoned: the launch must initialise what it uses
    y = _fwd("s2", x, wp, b, co, relu=False, out_range=out_range)
    assert torch.equal(y, _fwd("s2", x, wp, b, co, relu=False))
    assert _range_max(out_range) == y.abs().max().item()
    z_fed = _fwd("s1", y, wp2, b2, 32, x_range=out_range, ws=None)
    z_null = _fwd("s1", y, wp2, b2, 32)
    assert torch.equal(z_fed, z_null)
    # ops.conv2d_s2: want_range tags the result, the next conv2d picks the tag up
    p1, p2 = ops.PackedConv2d(wt, b), ops.PackedConv2d(w2, b2)
    yt = ops.conv2d_s2(x, p1, want_range=True)
    assert ops.tensor_range(yt) is not None and torch.equal(yt, y) and torch.equal(ops.conv2d(yt, p2), z_null)


def test_argument_rules():
    """Each refusal returns its code before anything is launched: y, pre-filled with a sentinel, is untouched."""
    from megaportrait_hack_amd import ops

    lib = _lib()
    t = torch.zeros(1 << 16, device=DEV)
    y = torch.full((1 << 14,), 7.0, device=DEV)
    args = lambda n, ci, co, h, w, x=t, wp=t, b=t, res=None, y=y, ws=t, wsb=1 << 18: (
        _p(x), None, _p(wp), _p(b), _p(res), _p(y), None, n, ci, co, h, w, 0, _p(ws), wsb, _stream())
    for shape in [(1, 8, 32, 8, 8), (1, 16, 48, 8, 8), (1, 16, 32, 0, 8), (0, 16, 32, 8, 8), (1, 16, 32, 1 << 15, 1 << 16)]:
        assert lib.mphip_conv2d_s2_supported(*shape) == 0 and lib.mphip_conv2d_s2_workspace_bytes(*shape) == 0
        assert not ops.conv2d_s2_supported(*shape)
        assert lib.mphip_conv2d_s2_fwd(*args(*shape)) == EINVAL and b"conv2d_s2_fwd" in lib.mphip_last_error()
    ok = (1, 16, 32, 8, 8)      # x: 1024 elements, y: 32 x 4 x 4 = 512
    assert lib.mphip_conv2d_s2_supported(*ok) == 1
    for missing in ("x", "wp", "b", "y"):
        assert lib.mphip_conv2d_s2_fwd(*args(*ok, **{missing: None})) == EINVAL and b"conv2d_s2_fwd: null" in lib.mphip_last_error()
    assert lib.mphip_conv2d_s2_fwd(*args(*ok, x=y)) == EINVAL and b"must not alias" in lib.mphip_last_error()           # y is x
    assert lib.mphip_conv2d_s2_fwd(*args(*ok, res=y[511:])) == EINVAL and b"must not alias" in lib.mphip_last_error()   # one element shared
    assert lib.mphip_conv2d_s2_fwd(*args(*ok, x=y[512:], res=y[1536:])) == 0, lib.mphip_last_error()   # extents from Ho*Wo: these only touch
    y[:512] = 7.0
    need = lib.mphip_conv2d_s2_workspace_bytes(*ok)
    assert need >= RANGE_FLOATS * 4
    assert lib.mphip_conv2d_s2_fwd(*args(*ok, wsb=need - 4)) == EWORKSPACE and b"conv2d_s2_fwd: workspace" in lib.mphip_last_error()
    assert lib.mphip_conv2d_s2_fwd(*args(*ok, ws=None, wsb=0)) == EWORKSPACE
    assert lib.mphip_conv2d_s2_fwd(*args(*ok, b=None, wsb=need - 4)) == EINVAL      # the argument error wins
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    with pytest.raises(RuntimeError):
        ops.conv2d_s2(torch.zeros(1, 32, 8, 8, device=DEV), ops.PackedConv2d(torch.zeros(32, 16, 3, 3, device=DEV), torch.zeros(32, device=DEV)))
    with pytest.raises(RuntimeError, match="residual"):
        ops.conv2d_s2(torch.zeros(1, 16, 8, 8, device=DEV), ops.PackedConv2d(torch.zeros(32, 16, 3, 3, device=DEV), torch.zeros(32, device=DEV)),
                      residual=torch.zeros(1, 32, 8, 8, device=DEV))
    torch.cuda.synchronize()
