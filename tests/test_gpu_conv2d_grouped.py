"""The grouped 2-D 3x3 conv on the matrix cores (csrc/conv2d_grp_f16x3.hip: mphip_conv2d_grouped_supported,
mphip_conv2d_grouped_workspace_bytes, mphip_conv2d_grouped_fwd), with the conventions of tests/test_gpu_conv2d_s2.py.

Integer data makes every product and partial sum an exact fp32 value (|sum| <= 9*256*8 + 16 < 2^24, power-of-two scales, every lo half 0),
so those cases are compared with torch.equal against the fp64 oracle F.conv2d(..., padding=1, groups=g).  The contract that pins the
arithmetic on random data: with the same x, descriptor and bias the launch writes the bits of mphip_conv2d_fwd on the dense [Co,Ci,3,3]
weight that holds the group blocks on its diagonal and exact zeros elsewhere (same max|w|, so the same pack scale): the chunks a group
skips are the ones that add exact zeros in the dense launch.  Random data is also held to the project's bar 4*e_torch + 2^-21*A (A = max
over outputs of sum |w||x| + |bias| + |residual|) against torch's fp32 grouped conv on the same GPU."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANGE_FLOATS = 4100

# (N, Ci, Co, H, W, groups): one pixel, one chunk and one channel tile per group; the image stride is Ci, not Cig (N = 2); two chunks and two
# channel tiles per group, ragged tiles on both axes; four groups; a group count that is no power of two; the net's own channel counts
SHAPES = [(1, 32, 128, 1, 1, 2), (2, 32, 128, 5, 7, 2), (1, 64, 256, 17, 19, 2), (1, 64, 256, 16, 16, 4), (1, 96, 192, 33, 18, 3),
          (1, 128, 128, 8, 8, 2), (1, 512, 512, 4, 4, 2)]
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
    assert lib.mphip_pack_conv2d_weight(_p(w), _p(wp), co, ci, _stream()) == 0, lib.mphip_last_error()
    return wp


def _fwd(groups, x, wp, bias, co, res=None, relu=False, x_range=None, out_range=None, ws="auto"):
    """mphip_conv2d_grouped_fwd (groups >= 1) or mphip_conv2d_fwd (groups None) called directly (no descriptor is looked up on the tensors)."""
    lib = _lib()
    n, ci, h, w = x.shape
    y = torch.empty((n, co, h, w), device=x.device)
    g = () if groups is None else (groups,)
    fn, wsfn = ((lib.mphip_conv2d_fwd, lib.mphip_conv2d_workspace_bytes) if groups is None
                else (lib.mphip_conv2d_grouped_fwd, lib.mphip_conv2d_grouped_workspace_bytes))
    nb = wsfn(n, ci, co, h, w, *g)
    wsb = torch.empty((nb + 3) // 4, device=x.device) if ws == "auto" else ws
    rc = fn(_p(x), _p(x_range), _p(wp), _p(bias), _p(res), _p(y), _p(out_range), n, ci, co, h, w, *g, int(relu), _p(wsb),
            0 if wsb is None else wsb.numel() * 4, _stream())
    assert rc == 0, lib.mphip_last_error()
    return y


def _range_max(rng):
    r = rng.view(torch.int32)
    n = int(r[3].item())
    assert rng[0].item() == 0.0 and 0 < n <= RANGE_FLOATS - 4
    return torch.cat([r[2:3], r[4:4 + n]]).max().view(1).view(torch.float32).item()


@pytest.mark.parametrize("shape,offset", [(s, False) for s in SHAPES] + [(s, True) for s in SHAPES[:2]], ids=_ids)
def test_integer_data_is_bit_exact(shape, offset):
    from megaportrait_hack_amd import ops

    lib = _lib()
    n, ci, co, h, w, g = shape
    assert lib.mphip_conv2d_grouped_supported(*shape) == 1 and ops.conv2d_grouped_supported(*shape)
    x, wt = _ints((n, ci, h, w), -4, 4, 1), _ints((co, ci // g, 3, 3), -2, 2, 2)
    b, res = _ints((co,), -8, 8, 3), _ints((n, co, h, w), -8, 8, 4)
    xg, rg = x.to(DEV), res.to(DEV)
    if offset:
        xg, rg = _misaligned(xg), _misaligned(rg)
    pack = ops.PackedConv2d(wt.to(DEV), b.to(DEV), g)
    assert (pack.ci, pack.co, pack.groups) == (ci, co, g)
    ops.f16x3_saturation_count(reset=True)
    for relu in (False, True):
        for with_res in (False, True):
            want = _oracle(x, wt, b, res if with_res else None, relu, g).float()
            assert want.abs().max() < 2 ** 24
            got = ops.conv2d_grouped(xg, pack, residual=rg if with_res else None, relu=relu)
            assert got.shape == want.shape == (n, co, h, w) and got.dtype == torch.float32
            assert torch.equal(got.cpu(), want), (shape, relu, with_res, (got.cpu() - want).abs().max().item())
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_grouped_writes_the_bits_of_the_dense_conv(shape):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w, g = shape
    x, wt, b = _rand((n, ci, h, w), 51, 2.0).to(DEV), _rand((co, ci // g, 3, 3), 52, 0.1).to(DEV), _rand((co,), 53).to(DEV)
    res = _rand((n, co, h, w), 54).to(DEV)
    wd = _dense(wt, g)
    assert wd.abs().max().item() == wt.abs().max().item()
    wp, wpd = _pack(wt), _pack(wd)
    assert torch.equal(wp[:4], wpd[:4])                  # the same header: one scale
    desc = ops.absmax_range(x.clone())                   # one explicit descriptor for both
    rng_g, rng_d = (torch.full((RANGE_FLOATS,), 1.0e30, device=DEV) for _ in range(2))
    for relu, r in ((False, None), (True, None), (False, res), (True, res)):
        got = _fwd(g, x, wp, b, co, res=r, relu=relu, x_range=desc, out_range=rng_g, ws=None)
        want = _fwd(None, x, wpd, b, co, res=r, relu=relu, x_range=desc, out_range=rng_d, ws=None)
        assert torch.equal(got, want), (shape, relu, r is not None, (got - want).abs().max().item())
        assert _range_max(rng_g) == _range_max(rng_d) == got.abs().max().item()


@pytest.mark.parametrize("shape", [(2, 32, 64, 19, 35), (1, 64, 96, 8, 8)], ids=_ids)
def test_one_group_is_the_plain_entry(shape):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = shape
    x, wt, b = _rand((n, ci, h, w), 61, 2.0).to(DEV), _rand((co, ci, 3, 3), 62, 0.1).to(DEV), _rand((co,), 63).to(DEV)
    res = _rand((n, co, h, w), 64).to(DEV)
    wp = _pack(wt)
    for relu in (False, True):      # both calls scan x
        assert torch.equal(_fwd(1, x, wp, b, co, res=res, relu=relu), _fwd(None, x, wp, b, co, res=res, relu=relu))
    p1 = ops.PackedConv2d(wt, b, 1)
    assert torch.equal(ops.conv2d_grouped(x, p1, relu=True), ops.conv2d(x, ops.PackedConv2d(wt, b), relu=True))


_PARITY = []


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_random_data_accuracy(shape):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w, g = shape
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
    yh = ops.conv2d_grouped(xg, ops.PackedConv2d(wg, bg, g), residual=rg, relu=True)
    e_torch = (yt.cpu().double() - y64).abs().max().item()
    e_hip = (yh.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -21 * A
    print(f"conv2d_grouped parity {shape}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} A={A:.3e} bound={bound:.3e}")
    _PARITY.append({"shape_N_Ci_Co_H_W_groups": list(shape), "e_hip": float(f"{e_hip:.4g}"), "e_torch": float(f"{e_torch:.4g}"),
                    "A": float(f"{A:.4g}"), "bound": float(f"{bound:.4g}")})
    out = os.environ.get("MPHIP_PARITY_JSON")      # the measured values, for profiles/conv2d_grouped_parity.json
    if out and len(_PARITY) == len(SHAPES):
        with open(out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "cases": _PARITY}, f, indent=1)
    assert e_hip <= bound
    assert ops.f16x3_saturation_count() == 0


def test_ranges_are_exact_and_interchangeable():
    from megaportrait_hack_amd import ops

    n, ci, co, h, w, g = 2, 64, 128, 21, 18, 2
    x, wt, b = _rand((n, ci, h, w), 21, 3.0).to(DEV), _rand((co, ci // g, 3, 3), 22, 0.1).to(DEV), _rand((co,), 23).to(DEV)
    w2, b2 = _rand((32, co, 3, 3), 24, 0.1).to(DEV), _rand((32,), 25).to(DEV)
    wp, wp2 = _pack(wt), _pack(w2)
    desc = ops.absmax_range(x.clone())
    y_null = _fwd(g, x, wp, b, co, relu=True)
    y_desc = _fwd(g, x, wp, b, co, relu=True, x_range=desc, ws=None)            # no workspace needed with a descriptor
    assert torch.equal(y_null, y_desc)
    out_range = torch.full((RANGE_FLOATS,), 1.0e30, device=DEV)                # poisoned: the launch must initialise what it uses
    y = _fwd(g, x, wp, b, co, relu=False, out_range=out_range)
    assert torch.equal(y, _fwd(g, x, wp, b, co, relu=False))
    assert _range_max(out_range) == y.abs().max().item()
    z_fed = _fwd(None, y, wp2, b2, 32, x_range=out_range, ws=None)
    z_null = _fwd(None, y, wp2, b2, 32)
    assert torch.equal(z_fed, z_null)
    # ops.conv2d_grouped: want_range tags the result, the next conv2d picks the tag up
    p1, p2 = ops.PackedConv2d(wt, b, g), ops.PackedConv2d(w2, b2)
    yt = ops.conv2d_grouped(x, p1, want_range=True)
    assert ops.tensor_range(yt) is not None and ops.current_range(yt) is not None and torch.equal(yt, y)
    assert _range_max(ops.current_range(yt)) == y.abs().max().item()
    assert ops.current_range(ops.conv2d_grouped(x, p1)) is None
    assert torch.equal(ops.conv2d(yt, p2), z_null)


def test_python_refusals():
    from megaportrait_hack_amd import ops

    z = lambda *s: torch.zeros(*s, device=DEV)
    p2 = ops.PackedConv2d(z(128, 16, 3, 3), z(128), 2)
    with pytest.raises(RuntimeError, match="grouped"):      # a grouped pack holds Ci / groups channels per slab row: no other kernel reads it
        ops.conv2d(z(1, 32, 8, 8), p2)
    with pytest.raises(RuntimeError, match="grouped"):
        ops.conv2d_s2(z(1, 32, 8, 8), p2)
    with pytest.raises(RuntimeError, match="does not match"):
        ops.conv2d_grouped(z(1, 16, 8, 8), p2)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.conv2d_grouped(z(1, 64, 8, 8), ops.PackedConv2d(z(64, 32, 3, 3), z(64), 2))      # Cog = 32
    with pytest.raises(RuntimeError, match="residual"):
        ops.conv2d_grouped(z(1, 32, 8, 8), p2, residual=z(1, 128, 4, 4))
    with pytest.raises(RuntimeError):
        ops.PackedConv2d(z(128, 8, 3, 3), z(128), 2)      # Cig = 8
    torch.cuda.synchronize()
