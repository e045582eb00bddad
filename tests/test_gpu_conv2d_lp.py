"""The typed, one-product form of the 2-D 3x3 convs (csrc/conv2d_lp.hip: mphip_conv2d_fwd_typed, mphip_conv2d_cat_fwd_typed) on the GPU.

One launch with products = 1 computes
    y = narrow_Y( act( unscale * sum round_f16(w * s_w) * round_f16(x * s_x)  + bias + widen(residual) ) )
with fp32 accumulation and one rounding at the store.

Integer data (the method of tests/test_gpu_conv_f32_branches.py): x in [-4, 4], w in [-3, 3], bias and residual in [-8, 8].  Every product
and partial sum is an exact integer below 2^24 (|sum| <= 9 * 48 * 12 + 16), every lo half is zero, so the fp32 value before the store is
exact and the result must be torch.equal to the float64 conv cast ONCE to the output dtype, for one product and for three.

Gaussian data: the yardstick is y64, the float64 conv of the operands rounded to f16 at their power-of-two scales
(oracle.hotpath_ref.round_f16_at_scale).  Bar: e_hip <= 4 * e_torch + 2^-22 * max|y64|, e_torch = the error of torch's fp32 conv of the
same rounded operands on the GPU: 4 is the project's rule for a different summation order, 2^-22 * max|y64| two fp32 ulps at the largest
output as the floor where torch happens to be exact.  Each test prints its pair (lines starting with `conv2d_lp_parity`, run with -s) and,
when MPHIP_PARITY_OUT names a file, appends it there: profiles/conv2d_lp_parity.json holds one MI355X run's pairs."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANGE_FLOATS = 4100
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# (x dtype, y dtype, products): every combination mphip_conv2d_typed_supported reports for the plain form
PLAIN = [(F32, F32, 1), (F16, F32, 1), (BF16, F32, 1), (F32, F16, 1), (F32, BF16, 1), (F32, F32, 3)]
NAME = {F32: "f32", F16: "f16", BF16: "bf16"}


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _oracle(x, w, b, res=None, relu=False):
    y = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu else y


def _range_max(rng):
    r = rng.view(torch.int32)
    n = int(r[3].item())
    assert rng[0].item() == 0.0 and 0 < n <= RANGE_FLOATS - 4
    return torch.cat([r[2:3], r[4:4 + n]]).max().view(1).view(torch.float32).item()


def record(case, **figures):
    line = {"case": case, **figures}
    print("conv2d_lp_parity " + json.dumps(line))
    out = os.environ.get("MPHIP_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")


def test_the_table_of_combinations_is_the_one_tested_here():
    from megaportrait_hack_amd import ops

    built = [(x, y, p) for p in (1, 3) for x in (F32, F16, BF16) for y in (F32, F16, BF16) if ops.conv2d_typed_supported(False, x, F32, y, p)]
    assert sorted(built, key=str) == sorted(PLAIN, key=str)
    assert [y for y in (F32, F16, BF16) if ops.conv2d_typed_supported(True, F32, F32, y, 1)] == [F32, F16, BF16]
    assert [y for y in (F32, F16, BF16) if ops.conv2d_typed_supported(True, F32, F32, y, 3)] == [F32]


@pytest.mark.parametrize("combo", PLAIN, ids=lambda c: f"{NAME[c[0]]}-{NAME[c[1]]}-p{c[2]}")
@pytest.mark.parametrize("shape", [(2, 16, 32, 1, 1), (2, 32, 96, 13, 19), (1, 48, 64, 16, 16), (1, 16, 32, 17, 33)], ids=lambda s: "x".join(map(str, s)))
def test_integer_data_is_bit_exact(shape, combo):
    from megaportrait_hack_amd import ops

    n, ci, co, h, w = shape
    xdt, ydt, products = combo
    x, wt = _ints((n, ci, h, w), -4, 4, 1), _ints((co, ci, 3, 3), -3, 3, 2)
    b, res = _ints((co,), -8, 8, 3), _ints((n, co, h, w), -8, 8, 4)
    big = torch.empty(x.numel() + 1, dtype=xdt, device=DEV)         # one element past an aligned base: a half map then starts on a
    big[1:].copy_(x.view(-1))                                       # 2-byte, not 4-byte boundary (small integers are exact in f16 / bf16)
    xg = big[1:].view(n, ci, h, w)
    assert xg.is_contiguous() and xg.data_ptr() % 4 == (0 if xdt == F32 else 2)
    pack = ops.PackedConv2d(wt.to(DEV), b.to(DEV))
    ops.f16x3_saturation_count(reset=True)
    for relu in (False, True):
        for rdt in (None, F32) + ((ydt,) if ydt != F32 else ()):
            want64 = _oracle(x, wt, b, None if rdt is None else res, relu)
            assert want64.abs().max() < 2 ** 24
            want = want64.to(ydt)                                   # the one rounding
            rg = None if rdt is None else res.to(DEV).to(rdt)
            got = ops.conv2d(xg, pack, residual=rg, relu=relu, want_range=True, out_dtype=ydt, products=products)
            assert got.shape == want.shape and got.dtype == ydt and got.is_contiguous()
            assert torch.equal(got.cpu(), want), (shape, combo, relu, rdt, (got.cpu().double() - want.double()).abs().max().item())
            assert _range_max(ops.tensor_range(got)) == want.float().abs().max().item()      # the exact max|y| of the ROUNDED output
            if products == 1 and xdt == F32 and ydt == F32 and rdt in (None, F32):
                assert torch.equal(got, ops.conv2d(xg, pack, residual=rg, relu=relu))           # the lo halves are zero: three products agree
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("ydt", [F32, F16, BF16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("tables", ["both", "first", "none"])
def test_two_source_integer_data_is_bit_exact(tables, ydt):
    """(C1, C2) = (16, 32) at 13 x 19.  A table entry (scale, shift) with small integers keeps the staged values integers:
    relu(x * s + t) in [0, 4 * 2 + 3]; sums stay below 2^24."""
    from megaportrait_hack_amd import ops

    n, c1, c2, co, h, w = 2, 16, 32, 64, 13, 19
    x1, x2, wt = _ints((n, c1, h, w), -4, 4, 5), _ints((n, c2, h, w), -4, 4, 6), _ints((co, c1 + c2, 3, 3), -3, 3, 7)
    b, res = _ints((co,), -8, 8, 8), _ints((n, co, h, w), -8, 8, 9)
    t1 = torch.stack([_ints((n, c1), 1, 2, 10), _ints((n, c1), -3, 3, 11)], dim=-1).contiguous()
    t2 = torch.stack([_ints((n, c2), 1, 2, 12), _ints((n, c2), -3, 3, 13)], dim=-1).contiguous()
    use1, use2 = tables in ("both", "first"), tables == "both"
    s1 = F.relu(x1 * t1[..., 0, None, None] + t1[..., 1, None, None]) if use1 else x1
    s2 = (x2 * t2[..., 0, None, None] + t2[..., 1, None, None]) if use2 else x2       # (no ReLU on the second source)
    pack = ops.PackedConv2d(wt.to(DEV), b.to(DEV))
    bound = lambda: ops.absmax_range(torch.full((4,), 11.0, device=DEV))               # a descriptor that bounds a normalised source
    ops.f16x3_saturation_count(reset=True)
    for rdt in (None, F32) + ((ydt,) if ydt != F32 else ()):
        for relu in (False, True):
            want64 = _oracle(torch.cat([s1, s2], 1), wt, b, None if rdt is None else res, relu)
            assert want64.abs().max() < 2 ** 24
            want = want64.to(ydt)
            kw = dict(x2=x2.to(DEV), affine1=t1.to(DEV) if use1 else None, relu1=use1, x1_range=bound() if use1 else None,
                      affine2=t2.to(DEV) if use2 else None, x2_range=bound() if use2 else None,
                      residual=None if rdt is None else res.to(DEV).to(rdt), relu=relu, want_range=True)
            got = ops.conv2d_cat(x1.to(DEV), pack, out_dtype=ydt, products=1, **kw)
            assert got.dtype == ydt and torch.equal(got.cpu(), want), (tables, ydt, rdt, relu)
            assert _range_max(ops.tensor_range(got)) == want.float().abs().max().item()
            if ydt == F32:
                assert torch.equal(got, ops.conv2d_cat(x1.to(DEV), pack, **kw))       # three products: the same integers
                assert torch.equal(got, ops.conv2d_cat(x1.to(DEV), pack, out_dtype=F32, products=3, **kw))
    assert ops.f16x3_saturation_count() == 0
    with pytest.raises(RuntimeError, match="typed source"):
        ops.conv2d_cat(x1.to(DEV).half(), pack, x2=x2.to(DEV).half(), products=1)
    with pytest.raises(RuntimeError, match="no kernel"):
        ops.conv2d_cat(x1.to(DEV), pack, x2=x2.to(DEV), out_dtype=F16, products=3)


@pytest.mark.parametrize("shape", [(2, 32, 96, 13, 19), (1, 512, 64, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_gaussian_data_follows_the_one_product_contract(shape):
    from megaportrait_hack_amd import ops
    from oracle.hotpath_ref import round_f16_at_scale

    n, ci, co, h, w = shape
    x, wt, b = _rand((n, ci, h, w), 51), _rand((co, ci, 3, 3), 52, 0.05), _rand((co,), 53)
    xr, wr = round_f16_at_scale(x), round_f16_at_scale(wt, top=15)            # (weights scale to below 2^15: csrc/mphip_f16x3.h)
    y64 = _oracle(xr, wr, b)
    y64_unrounded = _oracle(x, wt, b)
    xg, wg, bg = x.to(DEV), wt.to(DEV), b.to(DEV)
    tf32 = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        yt = F.conv2d(xr.float().to(DEV), wr.float().to(DEV), bg, padding=1)
    finally:
        torch.backends.cudnn.allow_tf32 = tf32
    pack = ops.PackedConv2d(wg, bg)
    ops.f16x3_saturation_count(reset=True)
    y1 = ops.conv2d(xg, pack, products=1)
    y3 = ops.conv2d(xg, pack, products=3)
    e_hip = (y1.cpu().double() - y64).abs().max().item()
    e_torch = (yt.cpu().double() - y64).abs().max().item()
    bar = 4 * e_torch + 2.0 ** -22 * y64.abs().max().item()
    e1 = (y1.cpu().double() - y64_unrounded).abs().max().item()
    e3 = (y3.cpu().double() - y64_unrounded).abs().max().item()
    record("conv2d one product " + "x".join(map(str, shape)), e_hip=e_hip, e_torch=e_torch, bar=bar, e_one_vs_unrounded=e1, e_three_vs_unrounded=e3)
    assert e_hip <= bar
    assert not torch.equal(y1, y3) and e1 > e3                                  # the mode was really taken
    assert torch.equal(y3, ops.conv2d(xg, pack))                                # three products through the typed entry: the fp32 entry
    # typed x gives the bits of its widened copy
    for dt in (F16, BF16):
        xt = xg.to(dt)
        assert torch.equal(ops.conv2d(xt, pack, products=1), ops.conv2d(xt.float(), pack, products=1)), dt
    # typed y equals the fp32 result .to(dtype); the residual in either dtype
    res = _rand((n, co, h, w), 54).to(DEV)
    for dt in (F16, BF16):
        assert torch.equal(ops.conv2d(xg, pack, out_dtype=dt, products=1), y1.to(dt)), dt
        a = ops.conv2d(xg, pack, residual=res.to(dt), relu=True, out_dtype=dt, products=1)
        assert torch.equal(a, ops.conv2d(xg, pack, residual=res.to(dt).float(), relu=True, products=1).to(dt)), dt
    # products = 0 follows the thread's policy; the old entry does not
    old = ops.conv2d(xg, pack)
    assert torch.equal(ops.conv2d(xg, pack, products=0), y3)
    with ops.half_products(True):
        assert torch.equal(ops.conv2d(xg, pack, products=0), y1)
        assert torch.equal(ops.conv2d(xg, pack), old)                           # its old bits: fp32 and three products
        assert torch.equal(ops.conv2d(xg, pack, products=3), y3)
    assert torch.equal(ops.conv2d(xg, pack, products=0), y3)
    assert ops.f16x3_saturation_count() == 0


def test_two_source_one_product_matches_the_plain_form_and_the_concatenation():
    """Without tables the two-source launch computes the plain launch of the concatenated map, bit for bit, in one product too; with
    typed y it is that result rounded once; products = 0 follows the policy."""
    from megaportrait_hack_amd import ops

    n, c1, c2, co, h, w = 2, 16, 32, 64, 13, 19
    x1, x2 = _rand((n, c1, h, w), 61).to(DEV), _rand((n, c2, h, w), 62, 0.5).to(DEV)
    pack = ops.PackedConv2d(_rand((co, c1 + c2, 3, 3), 63, 0.05).to(DEV), _rand((co,), 64).to(DEV))
    xcat = torch.cat([x1, x2], 1)
    y1 = ops.conv2d_cat(x1, pack, x2=x2, products=1)
    assert torch.equal(y1, ops.conv2d(xcat, pack, products=1)) and not torch.equal(y1, ops.conv2d_cat(x1, pack, x2=x2))
    for dt in (F16, BF16):
        assert torch.equal(ops.conv2d_cat(x1, pack, x2=x2, out_dtype=dt, products=1), y1.to(dt))
    with ops.half_products(True):
        assert torch.equal(ops.conv2d_cat(x1, pack, x2=x2, products=0), y1)
        assert torch.equal(ops.conv2d_cat(x1, pack, x2=x2), ops.conv2d(xcat, pack))
    assert torch.equal(ops.conv2d_cat(x1, pack, x2=x2, products=0), ops.conv2d(xcat, pack))
