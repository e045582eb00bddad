"""Eapp's 2-D ResBlock_Custom trunk on the matrix cores (model.ResBlockCustomFused, model.native_eapp_trunk: two mphip_conv2d_cat_fwd
launches per block) against the unswapped blocks in fp64 on the CPU and against the reference's own block (tests/golden/eapp_trunk.npz,
tools/make_eapp_trunk_golden.py).  Tolerance rule of the project for a different summation order: e_hip <= 4 * e_torch + floor,
floor = 2^-22 * max|y64| (tests/test_gpu_g2d_body.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eapp_trunk.npz")


def _check(name, y_hip, e_torch, y64):
    e_hip = (y_hip.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -22 * y64.abs().max().item()
    print(f"eapp trunk parity {name}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} max|y64|={y64.abs().max().item():.3e} bound={bound:.3e}")
    assert e_hip <= bound, (name, e_hip, bound)


def _err(y, y64):
    return (y.cpu().double() - y64).abs().max().item()


def test_reference_block_fixture():
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    gold = np.load(GOLDEN)
    blk = E.ResBlock_Custom(2, 32, 64)
    blk.load_state_dict({k: torch.from_numpy(gold[k]) for k in blk.state_dict()})
    x, y32, y64 = (torch.from_numpy(gold[k]) for k in ("x", "y32", "y64"))
    assert tuple(x.shape) == (2, 32, 12, 20) and y64.dtype == torch.float64
    fused = M.ResBlockCustomFused.from_block(blk.to(DEV))
    ops.f16x3_saturation_count(reset=True)
    with torch.no_grad():
        assert fused._native_ok(x.to(DEV))
        y = fused(x.to(DEV))
    _check("reference ResBlock_Custom(2, 32, 64)", y, _err(y32, y64), y64)      # e_torch: the reference's own recorded fp32 error
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("n,ci,co,h,w", [(2, 64, 128, 13, 19), (1, 128, 256, 16, 16)])
def test_fused_block_against_fp64(n, ci, co, h, w):
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(ci + co)
    blk = E.ResBlock_Custom(2, ci, co)
    x = torch.randn(n, ci, h, w) - 0.5
    with torch.no_grad():
        y64 = copy.deepcopy(blk).double()(x.double())
        gpu = blk.to(DEV)
        xg = x.to(DEV)
        e_torch = _err(gpu(xg), y64)
        fused = M.ResBlockCustomFused.from_block(gpu)
        ops.f16x3_saturation_count(reset=True)
        y_hip = fused(xg)
        assert fused._native_ok(xg) and "_mphip_fold" in fused.__dict__ and ops.tensor_range(y_hip) is not None
        fold = fused.__dict__["_mphip_fold"]
        assert y_hip.dtype == torch.float32 and y_hip.is_contiguous() and tuple(y_hip.shape) == (n, co, h, w)
        _check(f"block {ci}->{co} {h}x{w}", y_hip, e_torch, y64)
        assert torch.equal(fused(xg), y_hip) and fused.__dict__["_mphip_fold"] is fold                 # same bits twice, fold cached
        fused.train()                                                                                  # no mode-dependent layer
        assert fused._native_ok(xg) and torch.equal(fused(xg), y_hip)
        assert torch.equal(fused(xg.contiguous(memory_format=torch.channels_last)), y_hip)             # NHWC input: copied once
        y_half = fused(xg.half())                                                                      # autocast upstream: widened, fp32 out
        assert y_half.dtype == torch.float32 and (y_half - y_hip).abs().max().item() < 0.05 * y_hip.abs().max().item()
    assert ops.f16x3_saturation_count() == 0


@pytest.fixture(scope="module")
def eapp_case():
    from megaportrait_hack_amd import encoders2d as E

    torch.manual_seed(11)
    eapp = E.Eapp().eval()
    x = torch.rand(1, 3, 64, 64) * 2 - 1
    with torch.no_grad():
        y64 = copy.deepcopy(eapp).double().trunk2d(x.double())
        gpu = eapp.to(DEV)
        y_torch = gpu.trunk2d(x.to(DEV)).clone()
    return gpu, x.to(DEV), y_torch, y64


def test_whole_trunk_against_fp64_and_the_switch(eapp_case):
    from megaportrait_hack_amd import gbase, integration, model as M

    eapp, x, y_torch, y64 = eapp_case
    assert tuple(y64.shape) == (1, 1536, 8, 8)
    slots = lambda: [eapp.resblock_128, eapp.resblock_256, eapp.resblock_512]
    originals, keys = slots(), list(eapp.state_dict().keys())
    with torch.no_grad():
        try:
            assert eapp.native_trunk() is eapp and all(isinstance(b, M.ResBlockCustomFused) for b in slots())
            assert M.native_eapp_trunk(eapp, True) is False                                            # twice: a no-op
            assert list(eapp.state_dict().keys()) == keys
            y0 = eapp.trunk2d(x)
            _check("Eapp.trunk2d native_trunk", y0, _err(y_torch, y64), y64)
            fold0 = eapp.resblock_128.__dict__["_mphip_fold"]
            assert torch.equal(eapp.trunk2d(x), y0) and eapp.resblock_128.__dict__["_mphip_fold"] is fold0
            eapp.resblock_128.conv_ws.weight.mul_(torch.linspace(0.5, 1.5, 64 * 9, device=DEV).view(1, 64, 3, 3))   # in-place: re-folded
            y1 = eapp.trunk2d(x)
            assert eapp.resblock_128.__dict__["_mphip_fold"] is not fold0 and not torch.equal(y1, y0)
        finally:
            M.native_eapp_trunk(eapp, False)
    assert all(a is b for a, b in zip(originals, slots())) and list(eapp.state_dict().keys()) == keys
    assert M.native_eapp_trunk(eapp, False) is False
    g = gbase.Gbase(appearanceEncoder=eapp)
    assert len(g.state_dict()) == 971
    done = integration.install(g, eapp_tail=False, eapp_trunk=True)
    assert "Eapp.trunk2d" in done and len(g.state_dict()) == 971 and isinstance(eapp.resblock_512, M.ResBlockCustomFused)
    assert "Eapp.trunk2d" not in integration.install(g, eapp_tail=False)
    assert g.native_trunk(False) is g and eapp.resblock_512 is originals[-1]


@pytest.mark.parametrize("mode", ["input_grad", "param_grad", "half"])
def test_fallbacks_are_the_original_forward(mode):
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(3)
    blk = E.ResBlock_Custom(2, 32, 64).to(DEV)
    x = torch.randn(2, 32, 9, 11, device=DEV)
    if mode == "half":
        blk, x = blk.half(), x.half()
    if mode != "param_grad":
        blk.requires_grad_(False)
    x.requires_grad_(mode == "input_grad")
    fused = M.ResBlockCustomFused.from_block(blk)
    assert not fused._native_ok(x)
    want, got = blk(x), fused(x)
    assert torch.equal(got, want) and got.dtype == want.dtype and "_mphip_fold" not in fused.__dict__
    if mode == "input_grad":
        got.square().sum().backward()
        assert x.grad is not None and x.grad.abs().max() > 0
    if mode == "param_grad":
        got.square().sum().backward()
        assert all(p.grad is not None and p.grad.abs().max() > 0 for p in blk.parameters())             # the block's own Parameters


def test_cli_flag_reaches_the_switch(tmp_path, capsys, monkeypatch):
    from megaportrait_hack_amd import gbase, reenact

    seen = []
    real = gbase.Gbase.native_trunk
    monkeypatch.setattr(gbase.Gbase, "native_trunk", lambda self, enable=True: (seen.append(enable), real(self, enable))[1])
    xs, xd = torch.rand(1, 3, 64, 64) * 2 - 1, torch.rand(2, 3, 64, 64) * 2 - 1
    torch.save(xs, str(tmp_path / "xs.pt"))
    torch.save(xd, str(tmp_path / "xd.pt"))
    base = ["--random-init", "--source-tensor", str(tmp_path / "xs.pt"), "--drivers-tensor", str(tmp_path / "xd.pt"), "--any-size"]
    torch.manual_seed(5)
    assert reenact.main(base + ["--output-tensor", str(tmp_path / "a.pt")]) == 0 and seen == []
    torch.manual_seed(5)
    assert reenact.main(base + ["--output-tensor", str(tmp_path / "b.pt"), "--native-eapp-trunk"]) == 0 and seen == [True]
    assert isinstance(json.loads(capsys.readouterr().out.strip().splitlines()[-1]), dict)      # the CLI's JSON summary line
    a, b = torch.load(str(tmp_path / "a.pt"))["frames"], torch.load(str(tmp_path / "b.pt"))["frames"]
    assert a.shape == b.shape == (2, 3, 64, 64) and (a - b).abs().max().item() < 1e-3
