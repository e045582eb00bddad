"""The fused 2-D blocks (model.ResBlock2DFused, model.ResBlockCustomFused) with `half_precision=True` on the GPU.

Two bitwise contracts:
  autocast  an fp32 block inside torch.autocast('cuda', float16) returns float16 and
                out == fused_fp32_out_under(ops.half_products(True))(x.float()).half()
  twin      a .half() / .bfloat16() block equals its fp32 twin rounded once: copy.deepcopy(block).float(), fused, run under
            ops.half_products(True) on x.float(), cast to the model dtype.
Accuracy, once per block and mode: against the ORIGINAL block evaluated in float64 on the same (half) parameters and input,
e_hip <= 4 * e_torch + ulp, e_torch = the error of the stock block run by torch in the same mode (autocast, or as a half module), 4 the
project's rule for another summation order, ulp = one unit in the last place of the output dtype at max|y64| (the floor where torch
happens to be exact).  Pairs are printed (`conv2d_lp_parity`) and go to profiles/conv2d_lp_parity.json (tests/test_gpu_conv2d_lp.py)."""
import copy
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_gpu_conv2d_lp import record

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HALF = (torch.float16, torch.bfloat16)
MANTISSA = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}


def _seed(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.5)
    return module


def _make(kind):
    """-> (fused class, an fp32 block on the GPU in eval mode, its input)"""
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(11)
    if kind == "res32":
        return M.ResBlock2DFused, _seed(E.ResBlock2D(32, 32), 1).to(DEV).eval(), torch.randn(2, 32, 9, 11, device=DEV)
    if kind == "res32to64":
        return M.ResBlock2DFused, _seed(E.ResBlock2D(32, 64), 2).to(DEV).eval(), torch.randn(2, 32, 9, 11, device=DEV)
    return M.ResBlockCustomFused, E.ResBlock_Custom(2, 64, 128).to(DEV).eval(), torch.randn(2, 64, 13, 19, device=DEV) - 0.5


KINDS = ["res32", "res32to64", "custom64to128"]


def _ulp(dtype, top):
    return 2.0 ** (math.floor(math.log2(top)) - MANTISSA[dtype])


def _accuracy(case, y_hip, y_torch, y64, dtype):
    e_hip = (y_hip.cpu().double() - y64).abs().max().item()
    e_torch = (y_torch.cpu().double() - y64).abs().max().item()
    bar = 4 * e_torch + _ulp(dtype, y64.abs().max().item())
    record(case, e_hip=e_hip, e_torch=e_torch, bar=bar, max_y64=y64.abs().max().item())
    assert e_hip <= bar, (case, e_hip, bar)


@pytest.mark.parametrize("kind", KINDS)
def test_autocast_contract(kind):
    from megaportrait_hack_amd import ops

    cls, blk, x = _make(kind)
    fused = cls.from_block(blk, half_precision=True)
    ops.f16x3_saturation_count(reset=True)
    with torch.no_grad():
        with ops.half_products(True):
            ref32 = fused(x)                                          # the fp32 block under the one-product policy, outside the region
            assert ref32.dtype == torch.float32 and fused._half_out(x) == torch.float32
        three = fused(x)                                              # no region, no policy: today's three-product path
        assert three.dtype == torch.float32 and fused._half_out(x) is None and not torch.equal(three, ref32)
        assert torch.equal(three, cls.from_block(blk)(x))
        fold = fused.__dict__["_mphip_fold"]
        with torch.autocast("cuda", dtype=torch.float16):
            assert fused._half_out(x) == torch.float16
            out = fused(x)
            out_h = fused(x.half())                                   # the dtype an autocast producer upstream hands over
            y_torch = blk(x)
        # (the stock block itself returns float16 there, except an Identity-shortcut ResBlock2D fed an fp32 map: `y + x` promotes to fp32)
        assert y_torch.dtype == (torch.float32 if kind == "res32" else torch.float16)
        assert out.dtype == out_h.dtype == torch.float16 and out.is_contiguous() and out_h.is_contiguous()
        assert torch.equal(out, ref32.half())                         # the contract, bit for bit
        with ops.half_products(True):
            assert torch.equal(out_h, fused(x.half().float()).half())
        assert fused.__dict__["_mphip_fold"] is fold                  # the cached fold served every call
        with torch.autocast("cuda", dtype=torch.bfloat16):            # bf16 regions are left alone
            assert fused._half_out(x) is None
        y64 = copy.deepcopy(blk).cpu().double()(x.cpu().double())
        _accuracy(f"{kind} autocast", out, y_torch, y64, torch.float16)
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("dt", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_half_module_equals_its_fp32_twin_rounded_once(kind, dt):
    from megaportrait_hack_amd import ops

    cls, blk, x = _make(kind)
    hb, xh = copy.deepcopy(blk).to(dt), x.to(dt)
    fused = cls.from_block(hb, half_precision=True)

    def twin_out():
        twin = cls.from_block(copy.deepcopy(hb).float(), half_precision=True)
        with ops.half_products(True):
            return twin(xh.float()).to(dt)

    ops.f16x3_saturation_count(reset=True)
    with torch.no_grad():
        assert fused._half_out(xh) == dt
        out = fused(xh)
        assert out.dtype == dt and out.is_contiguous() and ops.tensor_range(out) is not None
        assert torch.equal(out, twin_out())                           # the contract, bit for bit
        fold = fused.__dict__["_mphip_fold"]
        assert torch.equal(fused(xh), out) and fused.__dict__["_mphip_fold"] is fold          # the cached fold is reused
        assert all(p.weight.dtype == torch.float32 for p in fold[1] if p is not None)          # folded in fp32 from the widened parameters
        y64 = copy.deepcopy(hb).cpu().double()(xh.cpu().double())
        _accuracy(f"{kind} {dt}", out, hb(xh), y64, dt)
        first = hb.conv1 if kind != "custom64to128" else hb.conv_ws
        first.weight.mul_(0.5)                                        # an in-place update of the half parameters
        out2 = fused(xh)
        assert fused.__dict__["_mphip_fold"] is not fold and not torch.equal(out2, out) and torch.equal(out2, twin_out())
        assert fused._half_out(x) is None                             # an fp32 map into a half block: not this path
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("kind", KINDS)
def test_keyword_off_keeps_todays_fallbacks(kind):
    cls, blk, x = _make(kind)
    on, off = cls.from_block(blk, half_precision=True), cls.from_block(blk)
    with torch.no_grad():
        for probe in (x, x.half(), x.cpu(), x[:, :16]):
            assert on._native_ok(probe) == off._native_ok(probe)      # _native_ok is unchanged
        with torch.autocast("cuda", dtype=torch.float16):
            y = off(x.half())
        assert y.dtype == torch.float32 and torch.equal(y, off(x.half())) and off._half_out(x.half()) is None   # a half input: an fp32 result
        hb = copy.deepcopy(blk).half()
        f_off = cls.from_block(hb)
        assert not f_off._native_ok(x.half()) and f_off._half_out(x.half()) is None
        got = f_off(x.half())
        assert got.dtype == torch.float16 and "_mphip_fold" not in f_off.__dict__                               # a half block: the PyTorch expression
        assert torch.equal(got, hb(x.half()))


@pytest.mark.parametrize("kind", KINDS)
def test_train_mode_and_autograd_take_the_pytorch_expression(kind):
    cls, blk, x = _make(kind)
    fused = cls.from_block(blk, half_precision=True)
    with torch.autocast("cuda", dtype=torch.float16):
        assert fused._half_out(x) is None                             # the Parameters require grad
        y = fused(x)
        assert y.requires_grad and "_mphip_fold" not in fused.__dict__
        y.float().square().sum().backward()
    first = blk.conv1 if kind != "custom64to128" else blk.conv_ws
    assert first.weight.grad is not None and first.weight.grad.abs().max() > 0                                  # the block's own Parameters
    if kind != "custom64to128":
        fused.train()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert fused._half_out(x) is None and "_mphip_fold" not in fused.__dict__
            stats = [b.clone() for b in blk.buffers()]
            got = fused(x)
            for b, s in zip(blk.buffers(), stats):
                b.copy_(s)
            assert torch.equal(got, blk(x))                           # batch statistics: the original forward


def test_whole_g2d_under_autocast():
    from megaportrait_hack_amd import encoders2d as E

    torch.manual_seed(7)
    g2d = _seed(E.G2d(), 2).eval()
    x = torch.randn(1, 96, 8, 8)
    with torch.no_grad():
        g64 = copy.deepcopy(g2d).double()       # (the head's forward is HIP only: its two 1x1 convs in fp64 by hand, then the body)
        head = F.conv2d(F.conv2d(x.double(), g64.reshape.weight, g64.reshape.bias), g64.conv1x1.weight, g64.conv1x1.bias)
        y64 = g64.body(head)
        g2d, xg = g2d.to(DEV), x.to(DEV)
        slots = lambda: list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1]]
        originals = slots()
        with torch.autocast("cuda", dtype=torch.float16):
            y_torch = g2d(xg).clone()
            try:
                assert g2d.native_body(half_precision=True) is g2d
                assert all(b.__dict__.get("_mphip_half") for b in slots())
                y_hip = g2d(xg)
                assert all("_mphip_fold" in b.__dict__ for b in slots())            # every block took the native path
            finally:
                g2d.native_body(False)
        assert all(a is b for a, b in zip(originals, slots()))                      # the very same module objects are back
        assert y_hip.shape == y_torch.shape and y_hip.dtype == y_torch.dtype
        e_hip = (y_hip.cpu().double() - y64).abs().max().item()
        e_torch = (y_torch.cpu().double() - y64).abs().max().item()
        bar = 4 * e_torch + 2.0 ** -22 * y64.abs().max().item()
        record("G2d native_body(half_precision=True) autocast", e_hip=e_hip, e_torch=e_torch, bar=bar)
        assert e_hip <= bar
