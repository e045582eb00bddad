"""The 2-D 3x3 conv on the matrix cores (csrc/conv2d_f16x3.hip: mphip_conv2d_supported, mphip_conv2d_packed_weight_bytes,
mphip_pack_conv2d_weight, mphip_conv2d_workspace_bytes, mphip_conv2d_fwd) against an fp64 CPU oracle.

Integer data makes every product and partial sum an exact fp32 value (|sum| <= 9*512*8 < 2^24, power-of-two scales, every lo half 0),
so those cases are compared with torch.equal; random data is held to 4*e_torch + 2^-21*A (A = max over outputs of sum |w||x| + |bias| +
|residual|): 4 is the project's rule for a different summation order, 2^-21 per term the f16x3 contract of conv3d_f16x3.hip.
A one-product kernel (hi*hi only) cannot meet that bound: emulating the split on the CPU with exact accumulation gives, on the two
shapes of test_random_data_accuracy, errors of 1.5e-3 and 4.5e-3 against bounds of about 2e-5 and 1e-4 (the three products: 4e-7, 1e-6)."""
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


def _oracle(x, w, b, res, relu):
    y = F.conv2d(x.double(), w.double(), b.double(), padding=1)
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


def _fwd(x, wp, bias, co, res=None, relu=False, x_range=None, out_range=None, ws="auto"):
    """mphip_conv2d_fwd called directly (no descriptor is looked up on the tensors)."""
    lib = _lib()
    n, ci, h, w = x.shape
    y = torch.empty((n, co, h, w), device=x.device)
    nb = lib.mphip_conv2d_workspace_bytes(n, ci, co, h, w)
    wsb = torch.empty((nb + 3) // 4, device=x.device) if ws == "auto" else ws
    rc = lib.mphip_conv2d_fwd(_p(x), _p(x_range), _p(wp), _p(bias), _p(res), _p(y), _p(out_range), n, ci, co, h, w, int(relu), _p(wsb),
                              0 if wsb is None else wsb.numel() * 4, _stream())
    assert rc == 0, lib.mphip_last_error()
    return y


def _pack(w):
    lib = _lib()
    co, ci = w.shape[:2]
    nb = lib.mphip_conv2d_packed_weight_bytes(co, ci)
    assert nb > 0
    wp = torch.empty((nb + 3) // 4, device=w.device)
    assert lib.mphip_pack_conv2d_weight(_p(w), _p(wp), co, ci, _stream()) == 0, lib.mphip_last_error()
    return wp


def _range_max(rng):
    r = rng.view(torch.int32)
    n = int(r[3].item())
    assert rng[0].item() == 0.0 and 0 < n <= RANGE_FLOATS - 4
    return torch.cat([r[2:3], r[4:4 + n]]).max().view(1).view(torch.float32).item()


INT_CASES = [(2, 16, 32, 8, 16), (1, 48, 64, 13, 19), (2, 32, 96, 24, 40), (1, 512, 512, 8, 8), (1, 64, 32, 1, 1), (1, 16, 32, 3, 70)]


# (the kernel has no vector path that depends on the base pointer's alignment; the first two cases still run 4 bytes off a 16-byte boundary)
@pytest.mark.parametrize("shape,offset", [(s, False) for s in INT_CASES] + [(s, True) for s in INT_CASES[:2]],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("plus4bytes" if v else "aligned"))
def test_integer_data_is_bit_exact(shape, offset):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = shape
    x, wt = _ints((n, ci, h, w), -4, 4, 1), _ints((co, ci, 3, 3), -2, 2, 2)
    b, res = _ints((co,), -8, 8, 3), _ints((n, co, h, w), -8, 8, 4)
    xg, rg = x.to(DEV), res.to(DEV)
    if offset:
        xg, rg = _misaligned(xg), _misaligned(rg)
    pack = ops.PackedConv2d(wt.to(DEV), b.to(DEV))
    ops.f16x3_saturation_count(reset=True)
    for relu in (False, True):
        for with_res in (False, True):
            want = _oracle(x, wt, b, res if with_res else None, relu).float()
            assert want.abs().max() < 2 ** 24
            got = ops.conv2d(xg, pack, residual=rg if with_res else None, relu=relu)
            assert got.shape == want.shape and got.dtype == torch.float32
            assert torch.equal(got.cpu(), want), (shape, relu, with_res, (got.cpu() - want).abs().max().item())
    assert ops.f16x3_saturation_count() == 0


def test_zero_padding_counts_the_taps():
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = 1, 16, 32, 19, 35      # ragged: two tile rows, three tile columns
    pack = ops.PackedConv2d(torch.ones(co, ci, 3, 3, device=DEV), torch.zeros(co, device=DEV))
    y = ops.conv2d(torch.ones(n, ci, h, w, device=DEV), pack).cpu()
    taps = F.conv2d(torch.ones(1, 1, h, w), torch.ones(1, 1, 3, 3), padding=1)      # 9 inside, 6 on an edge, 4 in a corner
    assert taps[0, 0, 0, 0] == 4 and taps[0, 0, 0, 1] == 6 and taps[0, 0, 5, 5] == 9
    assert torch.equal(y, (ci * taps).expand(n, co, h, w))


@pytest.mark.parametrize("xscale", [1.0, 1e4, 1e-4])
@pytest.mark.parametrize("shape", [(2, 64, 64, 16, 32), (1, 512, 256, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_random_data_accuracy(shape, xscale):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = shape
    x, wt = _rand((n, ci, h, w), 11, xscale), _rand((co, ci, 3, 3), 12, 0.05)
    b, res = _rand((co,), 13, xscale), _rand((n, co, h, w), 14, xscale)
    y64 = _oracle(x, wt, b, res, True)
    A = (F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), padding=1) + res.double().abs()).max().item()
    xg, wg, bg, rg = x.to(DEV), wt.to(DEV), b.to(DEV), res.to(DEV)
    cudnn = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        yt = F.relu(F.conv2d(xg, wg, bg, padding=1) + rg)
    finally:
        torch.backends.cudnn.allow_tf32 = cudnn
    ops.f16x3_saturation_count(reset=True)
    yh = ops.conv2d(xg, ops.PackedConv2d(wg, bg), residual=rg, relu=True)
    e_torch = (yt.cpu().double() - y64).abs().max().item()
    e_hip = (yh.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -21 * A
    print(f"conv2d parity {shape} x*{xscale:g}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} A={A:.3e} bound={bound:.3e}")
    assert e_hip <= bound
    assert ops.f16x3_saturation_count() == 0


def test_ranges_are_exact_and_interchangeable():
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = 2, 32, 64, 24, 40
    x, wt, b = _rand((n, ci, h, w), 21, 3.0).to(DEV), _rand((co, ci, 3, 3), 22, 0.1).to(DEV), _rand((co,), 23).to(DEV)
    w2, b2 = _rand((32, co, 3, 3), 24, 0.1).to(DEV), _rand((32,), 25).to(DEV)
    wp, wp2 = _pack(wt), _pack(w2)
    desc = ops.absmax_range(x.clone())
    y_null = _fwd(x, wp, b, co, relu=True)
    y_desc = _fwd(x, wp, b, co, relu=True, x_range=desc, ws=None)            # no workspace needed with a descriptor
    assert torch.equal(y_null, y_desc)
    out_range = torch.full((RANGE_FLOATS,), 1.0e30, device=DEV)             # poisoned: the launch must initialise what it uses
    y = _fwd(x, wp, b, co, relu=False, out_range=out_range)
    assert torch.equal(y, _fwd(x, wp, b, co, relu=False))
    assert _range_max(out_range) == y.abs().max().item()
    z_fed = _fwd(y, wp2, b2, 32, x_range=out_range, ws=None)
    z_null = _fwd(y, wp2, b2, 32)
    assert torch.equal(z_fed, z_null)
    # ops.conv2d: want_range tags the result, the next conv2d picks the tag up
    p1, p2 = ops.PackedConv2d(wt, b), ops.PackedConv2d(w2, b2)
    yt = ops.conv2d(x, p1, want_range=True)
    assert ops.tensor_range(yt) is not None and torch.equal(yt, y) and torch.equal(ops.conv2d(yt, p2), z_null)


def test_out_range_folds_more_tiles_than_slots():
    """65 x 65 tiles = 4225 workgroups share the descriptor's 4096 partial maxima."""
    n, ci, co, h, w = 1, 16, 32, 1030, 1030
    x, wt, b = _rand((n, ci, h, w), 31).to(DEV), _rand((co, ci, 3, 3), 32, 0.1).to(DEV), _rand((co,), 33).to(DEV)
    out_range = torch.full((RANGE_FLOATS,), 1.0e30, device=DEV)
    y = _fwd(x, _pack(wt), b, co, out_range=out_range)
    assert int(out_range.view(torch.int32)[3].item()) == RANGE_FLOATS - 4
    assert _range_max(out_range) == y.abs().max().item()
    want = F.conv2d(x, wt, b, padding=1)
    assert (y - want).abs().max().item() <= 1e-4 * want.abs().max().item()


def test_two_calls_give_the_same_bits():
    from megaportrait_hack_amd import ops

    x, wt, b = _rand((2, 48, 24, 40), 41).to(DEV), _rand((96, 48, 3, 3), 42, 0.1).to(DEV), _rand((96,), 43).to(DEV)
    res = _rand((2, 96, 24, 40), 44).to(DEV)
    pack = ops.PackedConv2d(wt, b)
    a = ops.conv2d(x, pack, residual=res, relu=True, want_range=True)
    c = ops.conv2d(x, ops.PackedConv2d(wt, b), residual=res, relu=True, want_range=True)
    assert torch.equal(a, c) and torch.equal(ops.tensor_range(a)[:4 + 24], ops.tensor_range(c)[:4 + 24])   # 12 tiles x 2 co tiles


def test_non_finite_inputs_are_counted_not_clamped():
    from megaportrait_hack_amd import ops

    x = torch.ones(1, 16, 8, 8, device=DEV)
    x[0, 3, 4, 4] = float("inf")
    pack = ops.PackedConv2d(torch.ones(32, 16, 3, 3, device=DEV), torch.zeros(32, device=DEV))
    ops.f16x3_saturation_count(reset=True)
    y = ops.conv2d(x, pack)
    assert not torch.isfinite(y[0, :, 3:6, 3:6]).any() and torch.isfinite(y[0, :, 0, 0]).all()
    assert ops.f16x3_saturation_count(reset=True) > 0


def test_refusals():
    from megaportrait_hack_amd import ops

    lib = _lib()
    t = torch.zeros(1 << 16, device=DEV)
    args = lambda n, ci, co, h, w, x=t, wp=t, b=t, y=t[1 << 15:], ws=t, wsb=1 << 18: (      # (y apart from x: an in-place call is refused)
        _p(x), None, _p(wp), _p(b), None, _p(y), None, n, ci, co, h, w, 0, _p(ws), wsb, _stream())
    for shape in [(1, 8, 32, 8, 8), (1, 16, 16, 8, 8), (1, 16, 32, 0, 8), (1, 24, 32, 8, 8), (1, 16, 48, 8, 8), (0, 16, 32, 8, 8),
                  (1, 16, 32, 1 << 15, 1 << 15)]:
        assert lib.mphip_conv2d_supported(*shape) == 0 and lib.mphip_conv2d_workspace_bytes(*shape) == 0
        assert lib.mphip_conv2d_fwd(*args(*shape)) == EINVAL and b"conv2d_fwd" in lib.mphip_last_error()
    ok = (1, 16, 32, 8, 8)
    assert lib.mphip_conv2d_supported(*ok) == 1
    for missing in ("x", "wp", "b", "y"):
        assert lib.mphip_conv2d_fwd(*args(*ok, **{missing: None})) == EINVAL and b"null" in lib.mphip_last_error()
    assert lib.mphip_conv2d_fwd(*args(*ok, y=t)) == EINVAL and b"must not alias" in lib.mphip_last_error()
    need = lib.mphip_conv2d_workspace_bytes(*ok)
    assert need >= RANGE_FLOATS * 4
    assert lib.mphip_conv2d_fwd(*args(*ok, wsb=need - 4)) == EWORKSPACE and b"workspace" in lib.mphip_last_error()
    assert lib.mphip_conv2d_fwd(*args(*ok, ws=None, wsb=0)) == EWORKSPACE
    assert lib.mphip_conv2d_packed_weight_bytes(32, 8) == 0 and lib.mphip_conv2d_packed_weight_bytes(16, 16) == 0
    assert lib.mphip_pack_conv2d_weight(_p(t), _p(t), 16, 16, _stream()) == EINVAL
    assert lib.mphip_pack_conv2d_weight(None, _p(t), 32, 16, _stream()) == EINVAL
    with pytest.raises(RuntimeError):
        ops.PackedConv2d(torch.zeros(32, 8, 3, 3, device=DEV), torch.zeros(32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.conv2d(torch.zeros(1, 32, 8, 8, device=DEV), ops.PackedConv2d(torch.zeros(32, 16, 3, 3, device=DEV), torch.zeros(32, device=DEV)))
    torch.cuda.synchronize()
