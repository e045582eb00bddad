"""CPU test of the data behind tests/test_gpu_f16x3_lo_planes.py: for every (case, kind) that file runs, from the case's own data and not
from a formula, that hi + lo holds every scaled operand exactly (x, w, dy; t and u of the F(2,3) cases), that the fractional operand's lo
plane is non-zero on at least 40 % of its elements and the ternary operand's is zero, that a float64 emulation of the three-product
contract equals the float64 conv or gradient bit for bit and that value is an fp32 number, that the largest possible partial sum stays
below 2^24 units of the products' common lsb, and that the case can fail: an emulation with one product, or with hi and lo swapped, is
wrong on more than 90 % of the outputs that receive at least one non-zero product.  It also bounds the GPU file's EXCLUDED table.
Nothing here touches a GPU; the plan claims of the tables are checked by the host tests of the three source files."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_f16x3_lo_planes as gpu  # noqa: E402

from oracle import hotpath_ref as R  # noqa: E402

EXACT = 2 ** 24
CASES = gpu.all_cases()
IDS = [f"{t}:{cid}-{k}" for t, cid, k, _ in CASES]


def _exact_f32(t64):
    return torch.equal(t64.float().double(), t64)


def _pow2_unit(*ts):
    """the largest power of two (down to 2^-40) that divides every element of the tensors"""
    for k in range(-20, 41):
        if all(torch.equal(t * 2.0 ** k, (t * 2.0 ** k).round()) for t in ts):
            return 2.0 ** -k
    raise AssertionError("not dyadic tensors")


def _share(mask, among=None):
    if among is None:
        return mask.double().mean().item()
    return (mask & among).double().sum().item() / among.double().sum().item()


def _bilinear(f, like):
    """f(a, b) that does not spend a conv on an operand that is all zero (the ternary operand's lo plane): the result is 0"""
    return lambda a, b: f(a, b) if bool(a.any()) and bool(b.any()) else torch.zeros_like(like)


def _lo_share(lo, frac, d):
    """share of the fractional operand's elements with a non-zero lo half; where a ReLU or a dy box zeroes part of the operand, of the
    elements it leaves"""
    masked = bool(d.relu) if hasattr(d, "relu") else False
    return _share(lo != 0, (frac != 0) if (masked or d.boxes is not None) else None)


def _support(f, a, b):
    """outputs that receive at least one non-zero product (counted in fp32: the counts are small integers)"""
    return f((a != 0).float(), (b != 0).float()) > 0


def _check_can_fail(lin, one, swapped_same, swapped_wrong, support):
    assert bool(support.any())
    assert _share(one != lin, support) > 0.90, _share(one != lin, support)
    assert _share(swapped_wrong != lin, support) > 0.90
    assert torch.equal(swapped_same, lin)


def _conv_direct(d):
    """direct-domain conv cases: the 3x3x3 direct kernels, the 1x1x1 kernels, the 2-D bwd-data launch"""
    assert _exact_f32(d.staged)
    xh, xl, sx = R.split_f16_at_scale(d.staged, 14, d.x_scale)
    wh, wl, sw = R.split_f16_at_scale(d.w_eq, 15)
    assert sx == d.x_scale and d.staged.abs().max().item() * sx < 2 ** 14 and d.w_eq.abs().max().item() * sw < 2 ** 15
    assert torch.equal(xh + xl, d.staged) and torch.equal(wh + wl, d.w_eq.double())
    frac_lo, other_lo, frac = (wl, xl, d.w_eq) if d.kind == "wlo" else (xl, wl, d.staged)
    assert not bool(other_lo.any())
    assert _lo_share(frac_lo, frac, d) >= 0.40, _lo_share(frac_lo, frac, d)
    unit = _pow2_unit(xh, xl) * _pow2_unit(wh, wl)
    worst = d.conv(xh.abs() + xl.abs(), wh.abs() + wl.abs()).max().item() / unit
    assert worst < EXACT, worst
    hh = d.conv(xh, wh)
    conv = _bilinear(d.conv, hh)
    assert torch.equal(hh, R.conv_f16x3_contract(d.staged, d.w_eq, conv, 1, d.x_scale))
    three = conv(xh, wl) + hh + conv(xl, wh)
    assert torch.equal(three, d.lin) and _exact_f32(d.lin) and torch.equal(d.want.double(), d.lin if d.bias is None else
                                                                           d.lin + d.bias.double().view((1, -1) + (1,) * d.dims))
    swapped_x = conv(xl, wl) + conv(xl, wh) + hh      # Wlo*Xlo + Whi*Xlo + Whi*Xhi
    swapped_w = hh + conv(xh, wl) + conv(xl, wl)      # Whi*Xhi + Wlo*Xhi + Wlo*Xlo
    wrong, same = (swapped_x, swapped_w) if d.kind == "wlo" else (swapped_w, swapped_x)
    _check_can_fail(d.lin, hh, same, wrong, _support(d.conv, d.staged.float(), d.w_eq))
    return worst


def _conv_wino(d):
    """F(2,3) cases: what is split is the transformed pair"""
    assert _exact_f32(d.staged)
    th, tl, uh, ul, t, u, unit = R.wino_f16x3_operands(d.staged.float(), d.w_eq, d.x_scale)
    sx = d.x_scale
    sw = R.pow2_operand_scale(d.w_eq.abs().max().item(), 15)
    assert unit == sx * sw
    # the fp32 transform is exact on this data: t and u are the float64 transforms of the scaled operands
    xp = torch.nn.functional.pad(d.staged * sx, (1, 1))
    W = d.staged.shape[-1]
    dd = [xp[..., i:i + W:2] for i in range(4)]
    g = d.w_eq.double() * sw
    for got, want in zip(t, [dd[0] - dd[2], dd[1] + dd[2], dd[2] - dd[1], dd[1] - dd[3]]):
        assert torch.equal(got, want)
    for got, want in zip(u, [g[..., 0], 0.5 * (g[..., 0] + g[..., 1] + g[..., 2]), 0.5 * (g[..., 0] - g[..., 1] + g[..., 2]), g[..., 2]]):
        assert torch.equal(got, want)
    for hi, lo, v in zip(th + uh, tl + ul, t + u):
        assert torch.equal(hi + lo, v) and hi.abs().max().item() < 65504
    frac_lo, other_lo, frac = (ul, tl, u) if d.kind == "wlo" else (tl, ul, t)
    assert not any(bool(v.any()) for v in other_lo)
    lo_share = _lo_share(torch.stack(frac_lo), torch.stack(frac), d)
    assert lo_share >= 0.40, lo_share
    lsb = _pow2_unit(*th, *tl) * _pow2_unit(*uh, *ul)
    M = R.wino_position_sums([a.abs() + b.abs() for a, b in zip(th, tl)], [a.abs() + b.abs() for a, b in zip(uh, ul)])
    worst = max((M[0] + M[1] + M[2]).max().item(), (M[1] + M[2] + M[3]).max().item()) / lsb
    assert worst < EXACT, worst
    three = R.conv3d_wino_f16_contract(d.staged.float(), d.w_eq, products=3, x_scale=d.x_scale)
    assert torch.equal(three, d.lin) and _exact_f32(d.lin)
    assert torch.equal(d.want.double(), d.lin if d.bias is None else d.lin + d.bias.double().view(1, -1, 1, 1, 1))
    one = R.conv3d_wino_f16_contract(d.staged.float(), d.w_eq, products=1, x_scale=d.x_scale)
    # hi and lo swapped inside the operand WITHOUT fractional bits: its lo = 0 then multiplies what matters; swapped inside the other
    # operand the three products are the same sum (seen by the other kind)
    hh = R.wino_position_sums(th, uh)
    assert torch.equal(R.wino_output(hh, unit), one)
    live = lambda vs: any(bool(v.any()) for v in vs)                                                               # noqa: E731
    pos = lambda a, b: R.wino_position_sums(a, b) if live(a) and live(b) else [torch.zeros_like(m) for m in hh]     # noqa: E731
    out = lambda *ms: R.wino_output([sum(vs) for vs in zip(*ms)], unit)                                            # noqa: E731
    swapped_t = out(pos(tl, ul), pos(tl, uh), hh)      # Ulo*Tlo + Uhi*Tlo + Uhi*Thi
    swapped_u = out(hh, pos(th, ul), pos(tl, ul))      # Uhi*Thi + Ulo*Thi + Ulo*Tlo
    wrong, same = (swapped_t, swapped_u) if d.kind == "wlo" else (swapped_u, swapped_t)
    _check_can_fail(d.lin, one, same, wrong, _support(d.conv, d.staged.float(), d.w_eq))
    return worst


def _dw(d):
    xh, xl, sx = R.split_f16_at_scale(d.x, 14)
    dh, dl, sd = R.split_f16_at_scale(d.dy, 14)
    assert d.x.abs().max().item() * sx < 2 ** 14 and d.dy.abs().max().item() * sd < 2 ** 14
    assert torch.equal(xh + xl, d.x.double()) and torch.equal(dh + dl, d.dy.double())
    frac_lo, other_lo, frac = (xl, dl, d.x) if d.kind == "xlo" else (dl, xl, d.dy)
    assert not bool(other_lo.any())
    assert _lo_share(frac_lo, frac, d) >= 0.40, _lo_share(frac_lo, frac, d)
    unit = _pow2_unit(xh, xl) * _pow2_unit(dh, dl)
    worst = d.grad(xh.abs() + xl.abs(), dh.abs() + dl.abs()).max().item() / unit
    assert worst < EXACT, worst
    hh = d.grad(xh, dh)
    grad = _bilinear(d.grad, hh)
    three = hh + grad(xh, dl) + grad(xl, dh)
    assert torch.equal(three, d.lin) and torch.equal(three, R.bwd_weight_f16x3_contract(d.x, d.dy, grad, 3))
    assert _exact_f32(d.lin) and torch.equal(d.want.double(), d.lin)
    assert torch.equal(hh, R.bwd_weight_f16x3_contract(d.x, d.dy, grad, 1))
    swapped_x = grad(xl, dh) + grad(xl, dl) + hh      # the halves of x swapped: xlo*dyhi + xlo*dylo + xhi*dyhi
    swapped_d = grad(xh, dl) + grad(xl, dl) + hh
    wrong, same = (swapped_d, swapped_x) if d.kind == "xlo" else (swapped_x, swapped_d)
    _check_can_fail(d.lin, hh, same, wrong, _support(d.grad, d.x, d.dy))
    return worst


@pytest.mark.parametrize("table,cid,kind,make", CASES, ids=IDS)
def test_case_is_exact_and_can_fail(table, cid, kind, make):
    d = make()
    worst = _dw(d) if hasattr(d, "grad") else (_conv_wino(d) if d.wino else _conv_direct(d))
    print(f"{table}:{cid}-{kind}: largest possible partial sum {worst / EXACT:.3f} * 2^24 units")


def test_the_exclusions_are_few_named_and_leave_every_kernel_class():
    per_table = {}
    for t, cid, k, _ in CASES:
        per_table.setdefault(t, set()).add(cid)
    for (t, cid, k), reason in gpu.EXCLUDED.items():      # (an excluded case is in none of the GPU file's parameter lists)
        assert t in per_table and isinstance(reason, str) and reason and "\n" not in reason
        per_table[t].add(cid)
    for t, cids in per_table.items():
        out = {cid for (tt, cid, k) in gpu.EXCLUDED if tt == t}
        assert 10 * len(out) <= len(cids), (t, sorted(out))
    kept = lambda t: {cid for tt, cid, k, _ in CASES if tt == t and not gpu.excluded(tt, cid, k)}      # noqa: E731
    for name in gpu.FB.KERNEL_NAMES:
        assert any(cid.startswith(name) for cid in kept("FWD_CASES")) and any(cid.startswith(name) for cid in kept("BWD_CASES"))
    assert {cid.split("-")[0] for cid in kept("K1_CASES")} == {"k1<8,2>", "k1<4,2>", "k1<1,1>", "k1<1,2>"}
    assert {cid.split("-")[0] for cid in kept("INT_CASES-3d")} == {"k3", "k1"}
    assert {cid.split("-")[1] for cid in kept("INT_CASES-2d")} == {f"k{gpu.B2.VEC}", f"k{gpu.B2.MASKED}"}


def test_both_kinds_run_on_every_row_and_the_half_schedule_is_left_out():
    assert len(gpu.FWD_PARAMS) + sum(1 for key in gpu.EXCLUDED if key[0] == "FWD_CASES") == 2 * sum(1 for c in gpu.FB.FWD_CASES if not c.half)
    assert {c.kernel for c, _ in gpu.FWD_PARAMS} == set(range(6))
    assert {nm for _, nm in gpu.ROI_PARAMS} == {"tile-edges", "corner+volume", "empty+straddle", "frames3", "volume"}
    assert len(gpu.ROI_PARAMS) == len(gpu.FB.ROI_CASES) and len(gpu.GNIN_PARAMS) > len(gpu.FB.GNIN_CASES)
    assert {r for _, _, r in gpu.GNIN_PARAMS} == {0, 1}
    assert len(gpu.DW3_PARAMS) + len(gpu.DW2_PARAMS) + sum(1 for key in gpu.EXCLUDED if key[0].startswith("INT_CASES")) \
        == 2 * (len(gpu.WB.INT_CASES) + len(gpu.B2.INT_CASES))
