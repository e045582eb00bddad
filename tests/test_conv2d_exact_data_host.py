"""CPU test of the data behind tests/test_gpu_conv2d_exact.py: for every case of its tables, that the "xlo" / "wlo" operands do what the
file claims (one operand needs hi + lo, the other has lo = 0, every partial sum is exact in fp32), that the float64 conv is what a correct
three-product kernel must return bit for bit, and that the cases can fail: a float64 emulation of the contract
(oracle.hotpath_ref.conv_f16x3_contract) that drops the lo products, or swaps hi and lo of either operand, is wrong on more than 90 % of
the outputs.  Nothing here touches a GPU or the library."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_conv2d_exact as gpu  # noqa: E402

from oracle import hotpath_ref as R  # noqa: E402

EXACT = 2 ** 24
THREE_PRODUCT = [(c, k) for c in gpu.LO_CASES + gpu.UP2_CASES for k in gpu.KINDS if c.form != "typed"]
ONE_PRODUCT = [(c, k) for c in gpu.LO_CASES for k in gpu.KINDS if c.form == "typed"]
IDS = lambda rows: [f"{gpu.case_id(c)}-{k}" for c, k in rows]


def _exact_f32(t64):
    return torch.equal(t64.float().double(), t64)


def _pow2_unit(t):
    """the largest power of two (down to 2^-40) that divides every element of t"""
    for k in range(-8, 41):
        v = t * 2.0 ** k
        if torch.equal(v, v.round()):
            return 2.0 ** -k
    raise AssertionError("not a dyadic tensor")


def _share(mask):
    return mask.double().mean().item()


def test_the_tables_cover_every_form_and_every_id_is_unique():
    from megaportrait_hack_amd import ops

    forms = {c.form for c in gpu.LO_CASES + gpu.UP2_CASES}
    assert forms == (set(ops._CONV2D_FORMS) | {"stem7", "typed"})
    assert {c.form for c in gpu.MAG_CASES + gpu.MAG_UP2_CASES} == forms
    for table in (gpu.LO_CASES + gpu.UP2_CASES, gpu.MAG_CASES + gpu.MAG_UP2_CASES):
        ids = [gpu.case_id(c) for c in table]
        assert len(set(ids)) == len(ids)
    # the shapes: more than one ragged tile each way (16x16; stride 2: 8x16 outputs; pointwise: 256 pixels), two K chunks, Co = 96
    for c in gpu.LO_CASES:
        n, ci, co, h, w = c.shape
        o = dict(c.opt)
        assert n == 2
        if c.form == "pw":
            pix = ((h + o["stride"] - 1) // o["stride"]) * ((w + o["stride"] - 1) // o["stride"])
            assert pix > 256 and pix % 256
        elif c.form == "s2":
            assert h % 2 and w % 2 and (h + 1) // 2 > 8 and ((h + 1) // 2) % 8 and (w + 1) // 2 > 16 and ((w + 1) // 2) % 16
        else:
            assert h > 16 and w > 32 and h % 16 and w % 16
        if c.form not in ("stem7", "grouped"):
            assert ci // o.get("groups", 1) >= 32
        if c.form == "split":
            chunks = ci // o["groups"] // 16
            assert chunks % o["splits"] == 0 and 1 < o["splits"] <= chunks
        if c.form not in ("stem7", "grouped", "split") or o.get("groups", 1) == 1:
            assert co % 64 == 32 or c.form == "stem7"
    splits = {(dict(c.opt)["groups"], dict(c.opt)["splits"]) for c in gpu.LO_CASES if c.form == "split"}
    assert splits == {(1, 4), (1, 2), (2, 4), (2, 2)}               # the chunk count and a proper divisor of it, plain and grouped
    for table in (gpu.LO_CASES, gpu.MAG_CASES):                     # both bodies of the finish kernel: H * W % 4 == 0 and not
        assert {c.shape[3] * c.shape[4] % 4 == 0 for c in table if c.form == "split"} == {True, False}


@pytest.mark.parametrize("case,kind", THREE_PRODUCT, ids=IDS(THREE_PRODUCT))
def test_three_product_cases_are_exact_and_can_fail(case, kind):
    d = gpu.lo_data(case, kind)
    assert _exact_f32(d.staged)                                     # what the kernel stages (a table's x * scale + shift included) is fp32
    xh, xl, sx = R.split_f16_at_scale(d.staged, 14, d.x_scale)
    wh, wl, sw = R.split_f16_at_scale(d.w, 15)
    assert sx == d.x_scale and (d.staged.abs().max().item() * sx < 2 ** 14) and (d.w.abs().max().item() * sw < 2 ** 15)
    if kind == "wlo":
        assert sw == 2.0 ** 12
    elif case.form != "cat":
        assert sx == 2.0 ** 11
    # hi + lo holds the operand exactly; the operand with fractional bits needs its lo half, the other has none
    assert torch.equal(xh + xl, d.staged) and torch.equal(wh + wl, d.w.double())
    frac_lo, other_lo = (xl, wl) if kind == "xlo" else (wl, xl)
    assert not bool(other_lo.any())
    assert _share(frac_lo != 0) >= 0.40, _share(frac_lo != 0)
    # every partial sum, in any order, of any subset of the three products is bounded by the sum of their magnitudes: below 2^24 units
    unit = _pow2_unit(torch.cat([xh.flatten(), xl.flatten()])) * _pow2_unit(torch.cat([wh.flatten(), wl.flatten()]))
    assert unit == (2.0 ** -11 if kind == "xlo" else 2.0 ** -12)    # every product is a whole number of units
    worst = d.conv(xh.abs() + xl.abs(), wh.abs() + wl.abs()).max().item() / unit
    assert worst < EXACT, worst
    # the contract's three products are the float64 conv, which survives fp32; so do bias, residual and the activation
    y3 = R.conv_f16x3_contract(d.staged, d.w, d.conv, 3, d.x_scale)
    assert torch.equal(y3, d.lin) and torch.equal(y3.float().double(), d.lin)
    step = d.lin + d.b.double().view(1, -1, 1, 1)
    assert _exact_f32(step) and (d.res is None or _exact_f32(step + d.res.double())) and _exact_f32(d.want64)
    # the case can fail: one product is wrong nearly everywhere, and so is a swap of the hi and lo halves of the operand WITHOUT fractional
    # bits (its lo = 0 then multiplies what matters); a swap inside the other operand is the same sum here and is seen by the other kind
    y1 = R.conv_f16x3_contract(d.staged, d.w, d.conv, 1, d.x_scale)
    assert _share(y1 != d.lin) >= 0.90
    swapped_x = d.conv(xl, wl) + d.conv(xl, wh) + d.conv(xh, wh)    # Wlo*Xlo + Whi*Xlo + Whi*Xhi
    swapped_w = d.conv(xh, wh) + d.conv(xh, wl) + d.conv(xl, wl)    # Whi*Xhi + Wlo*Xhi + Wlo*Xlo
    wrong, same = (swapped_w, swapped_x) if kind == "xlo" else (swapped_x, swapped_w)
    assert _share(wrong != d.lin) >= 0.90 and torch.equal(same, d.lin)
    # a lo fragment misplaced by one pixel for ONE tap of one chunk shows as well
    lo_op = xl if kind == "xlo" else xh
    shifted = lo_op.clone()
    shifted[:, :16] = torch.roll(lo_op[:, :16], 1, dims=-1)
    w_tap = torch.zeros_like(wh)
    w_tap[:, :16, :1, :1] = (wh if kind == "xlo" else wl)[:, :16, :1, :1]
    moved = d.lin - d.conv(lo_op, w_tap) + d.conv(shifted, w_tap)
    assert _share(moved != d.lin) >= 0.40


@pytest.mark.parametrize("case,kind", ONE_PRODUCT, ids=IDS(ONE_PRODUCT))
def test_one_product_cases_are_exact_and_can_fail(case, kind):
    d = gpu.lo_data(case, kind)
    o = dict(case.opt)
    assert _exact_f32(d.staged)
    xr, wr = R.round_f16_at_scale(d.staged.float()), R.round_f16_at_scale(d.w, top=15)
    xh, xl, sx = R.split_f16_at_scale(d.staged, 14, d.x_scale)
    wh, wl, sw = R.split_f16_at_scale(d.w, 15)
    assert torch.equal(xr, xh) and torch.equal(wr, wh)              # the one rounding IS the hi half
    if o["xdt"] != gpu.F32:
        assert not bool(xl.any())                                    # a half x is its own hi half
    unit = _pow2_unit(xh) * _pow2_unit(wh)
    assert d.conv(xh.abs(), wh.abs()).max().item() / unit < EXACT
    assert torch.equal(R.conv_f16x3_contract(d.staged, d.w, d.conv, 1, d.x_scale), d.lin) and _exact_f32(d.lin)
    step = d.lin + d.b.double().view(1, -1, 1, 1)
    assert _exact_f32(step) and _exact_f32(step + d.res.double()) and _exact_f32(d.want64)
    # can fail: the three-product result (fp32 x), or the conv of the unrounded weight, differs nearly everywhere
    other = d.conv(d.staged, d.w.double())
    if o["xdt"] == gpu.F32 or kind == "wlo":
        assert _share(other != d.lin) >= 0.90
    else:
        assert torch.equal(other, d.lin)                             # (a half x with an integer w: nothing is rounded away)
        assert _share(d.conv(d.x.double(), d.w.double()) != d.lin) >= 0.90    # ... but the rounding to the dtype is seen


@pytest.mark.parametrize("case", gpu.MAG_CASES + gpu.MAG_UP2_CASES, ids=gpu.case_id)
def test_magnitude_cases_are_representable(case):
    d = gpu.mag_data(case)
    assert d.x.abs().max() == 4 and d.w.abs().max() == 4 and d.truth.abs().max() < EXACT
    o = dict(case.opt)
    for p in gpu.X_EXPONENTS:
        for q in gpu.W_EXPONENTS:
            xs, ws, want = gpu.mag_operands(d, p, q)
            if o.get("xdt", gpu.F32) != gpu.F32:
                assert torch.equal(xs.to(o["xdt"]).float(), xs)      # integers * 2^p are bf16 values
            if abs(p + q) < 120:
                assert torch.equal(want.double(), d.truth * 2.0 ** (p + q)) and bool(torch.isfinite(want).all())
            # the single factor 1/scale_w * 1/scale_x, in fp32: 0 at (-100, -30) alone
            uw, ux = 1.0 / R.pow2_operand_scale(ws.abs().max().item(), 15), 1.0 / R.pow2_operand_scale(xs.abs().max().item(), 14)
            one = torch.tensor(uw, dtype=torch.float32) * torch.tensor(ux, dtype=torch.float32)
            assert (one.item() == 0.0) == ((p, q) == (-100, -30))
            if (p, q) == (-100, -30):
                assert want.abs().max() > 0                          # normal or subnormal fp32 numbers the single product loses
