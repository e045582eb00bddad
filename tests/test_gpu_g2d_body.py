"""G2d's ResBlock2D body on the matrix cores (model.ResBlock2DFused, model.native_g2d_body) against the unswapped blocks in fp64 on
the CPU.  Tolerance rule of the project for a different summation order: e_hip <= 4 * e_torch + floor, floor = 2^-22 * max|y64|."""
import copy
import json

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _seed(module, seed):
    """Parameters as initialised; BatchNorm statistics and affine moved away from their initial values."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)      # [0.5, 1.5]
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.5)
    return module


def _check(name, y_hip, y_torch, y64):
    e_hip = (y_hip.cpu().double() - y64).abs().max().item()
    e_torch = (y_torch.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -22 * y64.abs().max().item()
    print(f"g2d body parity {name}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} max|y64|={y64.abs().max().item():.3e} bound={bound:.3e}")
    assert e_hip <= bound, (name, e_hip, bound)


@pytest.mark.parametrize("ci,co,h,w", [(512, 512, 8, 8), (512, 256, 16, 16), (128, 64, 13, 19)])
def test_fused_block_against_fp64(ci, co, h, w):
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(ci + co)
    blk = _seed(E.ResBlock2D(ci, co), 1).eval()
    x = torch.randn(2, ci, h, w)
    with torch.no_grad():
        y64 = copy.deepcopy(blk).double()(x.double())
        gpu = blk.to(DEV)
        y_torch = gpu(x.to(DEV))
        fused = M.ResBlock2DFused.from_block(gpu)
        ops.f16x3_saturation_count(reset=True)
        y_hip = fused(x.to(DEV))
        assert fused._native_ok(x.to(DEV)) and "_mphip_fold" in fused.__dict__ and ops.tensor_range(y_hip) is not None
        assert y_hip.dtype == torch.float32 and y_hip.is_contiguous()
        _check(f"block {ci}->{co} {h}x{w}", y_hip, y_torch, y64)
        assert torch.equal(fused(x.to(DEV)), y_hip)                                             # same bits twice
        assert torch.equal(fused(x.to(DEV).contiguous(memory_format=torch.channels_last)), y_hip)   # NHWC input: copied once
        y_half = fused(x.to(DEV).half())                                                        # autocast upstream: widened, fp32 out
        assert y_half.dtype == torch.float32 and (y_half - y_hip).abs().max().item() < 0.05 * y_hip.abs().max().item()
    assert ops.f16x3_saturation_count() == 0


@pytest.fixture(scope="module")
def g2d_case():
    from megaportrait_hack_amd import encoders2d as E

    torch.manual_seed(7)
    g2d = _seed(E.G2d(), 2).eval()
    x = torch.randn(1, 96, 8, 8)
    with torch.no_grad():
        g64 = copy.deepcopy(g2d).double()       # (the head's forward is HIP only: its two 1x1 convs in fp64 by hand, then the body)
        head = F.conv2d(F.conv2d(x.double(), g64.reshape.weight, g64.reshape.bias), g64.conv1x1.weight, g64.conv1x1.bias)
        y64 = g64.body(head)
        gpu = g2d.to(DEV)
        y_torch = gpu(x.to(DEV)).clone()
    return gpu, x.to(DEV), y_torch, y64


def test_whole_g2d_against_fp64(g2d_case):
    g2d, x, y_torch, y64 = g2d_case
    assert tuple(y64.shape) == (1, 3, 64, 64)
    slots = lambda: list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1], g2d.final_conv]
    originals = slots()
    with torch.no_grad():
        try:
            assert g2d.native_body() is g2d
            _check("G2d native_body", g2d(x), y_torch, y64)
            g2d.native_final_conv()
            _check("G2d native_body + native_final_conv", g2d(x), y_torch, y64)
        finally:
            g2d.native_final_conv(False)
            g2d.native_body(False)
        # switched off: the very modules of before.  What they compute is then stock torch's own forward, which promises no bitwise
        # reproducibility from call to call (its conv backend picks the solver, and with it the summation order, at run time: two such
        # runs differed in the last bits on an MI355X).  So identity of the objects, and the same accuracy rule as above, not the same bits
        assert all(a is b for a, b in zip(originals, slots()))
        _check("G2d switched off again", g2d(x), y_torch, y64)


@pytest.mark.parametrize("mode", ["train", "input_grad", "param_grad", "half"])
def test_fallbacks_are_the_original_forward(mode):
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(3)
    blk = _seed(E.ResBlock2D(32, 64), 4).to(DEV).eval()
    x = torch.randn(2, 32, 9, 11, device=DEV)
    if mode == "train":
        blk.train()
    if mode == "half":
        blk, x = blk.half(), x.half()
    if mode != "param_grad":
        blk.requires_grad_(mode == "train")
    x.requires_grad_(mode == "input_grad")
    fused = M.ResBlock2DFused.from_block(blk)
    assert not fused._native_ok(x)
    stats = [b.clone() for b in blk.buffers()]
    want = blk(x)
    for b, s in zip(blk.buffers(), stats):      # train mode steps the running statistics: rewind, so both see the same state
        b.copy_(s)
    got = fused(x)
    assert torch.equal(got, want) and got.dtype == want.dtype and "_mphip_fold" not in fused.__dict__
    if mode in ("train", "input_grad", "param_grad"):
        got.square().sum().backward()
        if mode == "input_grad":
            assert x.grad is not None and x.grad.abs().max() > 0
        else:
            assert blk.conv1.weight.grad is not None and blk.shortcut[1].weight.grad.abs().max() > 0   # the block's own Parameters


def test_switch_mechanics_on_the_gpu(g2d_case):
    from megaportrait_hack_amd import gbase, integration, model as M

    g2d, x, y_torch, _ = g2d_case
    keys = list(g2d.state_dict().keys())
    originals = list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1]]
    with torch.no_grad():
        try:
            assert M.native_g2d_body(g2d, True) is True and M.native_g2d_body(g2d, True) is False      # twice: a no-op
            assert list(g2d.state_dict().keys()) == keys
            y0 = g2d(x)
            fold0 = g2d.res_blocks[0].__dict__["_mphip_fold"]
            assert torch.equal(g2d(x), y0) and g2d.res_blocks[0].__dict__["_mphip_fold"] is fold0      # cached
            g2d.res_blocks[0].conv1.weight.mul_(1.5)                                                  # in-place update: repacked
            y1 = g2d(x)
            assert g2d.res_blocks[0].__dict__["_mphip_fold"] is not fold0 and not torch.equal(y1, y0)
            g2d.native_body(False)
            e_ref = (g2d(x) - y1).abs().max().item()
            g2d.native_body()
            assert e_ref < 1e-3, e_ref                                                                # tracks torch on the updated weight
            g2d.res_blocks[0].conv1.weight.div_(1.5)
            g2d.upsample2[1].bn2.running_mean.add_(0.25)                                              # a running buffer counts too
            y2 = g2d(x)
            g2d.upsample2[1].bn2.running_mean.sub_(0.25)
            assert not torch.equal(y2, y0) and (g2d(x) - y0).abs().max().item() < 1e-4
        finally:
            assert M.native_g2d_body(g2d, False) is True
    assert all(a is b for a, b in zip(originals, list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1]]))
    assert list(g2d.state_dict().keys()) == keys
    g = gbase.Gbase(G2d=g2d)
    assert len(g.state_dict()) == 971
    assert "G2d.body" in integration.install(g, eapp_tail=False, g2d_body=True) and len(g.state_dict()) == 971
    assert isinstance(g.G2d.upsample3[1], M.ResBlock2DFused)
    g.native_body(False)
    assert g.G2d.upsample3[1] is originals[-1]


def test_cli_flag_reaches_the_switch(tmp_path, capsys, monkeypatch):
    from megaportrait_hack_amd import gbase, reenact

    seen = []
    real = gbase.Gbase.native_body
    monkeypatch.setattr(gbase.Gbase, "native_body", lambda self, enable=True: (seen.append(enable), real(self, enable))[1])
    xs, xd = torch.rand(1, 3, 64, 64) * 2 - 1, torch.rand(2, 3, 64, 64) * 2 - 1
    torch.save(xs, str(tmp_path / "xs.pt"))
    torch.save(xd, str(tmp_path / "xd.pt"))
    base = ["--random-init", "--source-tensor", str(tmp_path / "xs.pt"), "--drivers-tensor", str(tmp_path / "xd.pt"), "--any-size"]
    torch.manual_seed(5)
    assert reenact.main(base + ["--output-tensor", str(tmp_path / "a.pt")]) == 0 and seen == []
    torch.manual_seed(5)
    assert reenact.main(base + ["--output-tensor", str(tmp_path / "b.pt"), "--native-g2d-body"]) == 0 and seen == [True]
    assert isinstance(json.loads(capsys.readouterr().out.strip().splitlines()[-1]), dict)      # the CLI's JSON summary line
    a, b = torch.load(str(tmp_path / "a.pt"))["frames"], torch.load(str(tmp_path / "b.pt"))["frames"]
    assert a.shape == b.shape == (2, 3, 64, 64) and (a - b).abs().max().item() < 1e-3
