"""Eapp's ResNet-50 on the matrix cores (model.BottleneckFused, model.native_eapp_resnet50, Eapp.native_resnet50, Gbase.native_resnet50)
against the unswapped modules in fp64 on the CPU, with the conventions and the bar of tests/test_gpu_emtn_resnets.py:
e_hip <= 4 * e_torch + floor, floor = 2^-22 * max|y64|, e_torch from the unswapped module on the same GPU."""
import copy

import pytest
import torch
import torch.nn as nn

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
    print(f"eapp resnet50 parity {name}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} max|y64|={y64.abs().max().item():.3e} bound={bound:.3e}")
    assert e_hip <= bound, (name, e_hip, bound)


@pytest.mark.parametrize("ci,planes,stride,shape", [(64, 64, 1, (2, 64, 9, 11)), (256, 64, 1, (2, 256, 9, 11)), (256, 128, 2, (1, 256, 16, 18)),
                                                    (256, 128, 2, (1, 256, 9, 11)), (512, 256, 2, (1, 512, 4, 4))])
def test_fused_block_against_fp64(ci, planes, stride, shape):
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(ci + planes + stride)
    blk = _seed(E._Bottleneck(ci, planes, stride), 1).eval()
    assert (blk.downsample is None) == (ci == 4 * planes and stride == 1)
    x = torch.randn(*shape)
    with torch.no_grad():
        y64 = copy.deepcopy(blk).double()(x.double())
        gpu = blk.to(DEV)
        y_torch = gpu(x.to(DEV))
        fused = M.BottleneckFused.from_block(gpu)
        ops.f16x3_saturation_count(reset=True)
        y_hip = fused(x.to(DEV))
        assert fused._native_ok(x.to(DEV)) and "_mphip_fold" in fused.__dict__ and ops.tensor_range(y_hip) is not None
        assert y_hip.dtype == torch.float32 and y_hip.is_contiguous() and y_hip.shape == y64.shape
        _check(f"block {ci}->{planes}->{4 * planes} stride {stride} {shape}", y_hip, y_torch, y64)
        fold = fused.__dict__["_mphip_fold"]
        assert len(fold[1]) == 4 and (fold[1][3] is None) == (blk.downsample is None)
        assert [p.pointwise for p in fold[1] if p is not None] == [True, False, True] + [True] * (blk.downsample is not None)
        assert torch.equal(fused(x.to(DEV)), y_hip) and fused.__dict__["_mphip_fold"] is fold   # same bits twice, the fold cached
        assert torch.equal(fused(x.to(DEV).contiguous(memory_format=torch.channels_last)), y_hip)   # NHWC input: copied once
        y_half = fused(x.to(DEV).half())                                                        # autocast upstream: widened, fp32 out
        assert y_half.dtype == torch.float32 and (y_half - y_hip).abs().max().item() < 0.05 * y_hip.abs().max().item()
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("mode", ["train", "input_grad", "param_grad", "half"])
def test_fallbacks_are_the_original_forward(mode):
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(3)
    blk = _seed(E._Bottleneck(32, 32, 2), 4).to(DEV).eval()
    x = torch.randn(2, 32, 9, 11, device=DEV)
    if mode == "train":
        blk.train()
    if mode == "half":
        blk, x = blk.half(), x.half()
    if mode != "param_grad":
        blk.requires_grad_(mode == "train")
    x.requires_grad_(mode == "input_grad")
    fused = M.BottleneckFused.from_block(blk)
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
            assert blk.conv1.weight.grad is not None and blk.conv3.weight.grad.abs().max() > 0      # the block's own Parameters
            assert blk.downsample[1].weight.grad.abs().max() > 0


def _slots(net):
    return [b for name in ("layer1", "layer2", "layer3") for b in getattr(net, name)]


@pytest.fixture(scope="module")
def eapp_case():
    """(Eapp on the GPU, [(x, net_torch, net64, es_torch, es64)] for both input sizes): the references are computed once, before any swap."""
    from megaportrait_hack_amd import encoders2d as E

    torch.manual_seed(11)
    eapp = _seed(E.Eapp(), 5).eval()
    g = torch.Generator().manual_seed(6)
    # 64 x 64: layer3 runs at 4 x 4.  72 x 56: 72 -> 36 -> 18 -> 9 -> 5 and 56 -> 28 -> 14 -> 7 -> 4: odd and even halvings, non-square
    xs = [torch.randn(2, 3, 64, 64, generator=g), torch.randn(1, 3, 72, 56, generator=g)]
    with torch.no_grad():
        net64, fc64 = copy.deepcopy(eapp.custom_resnet50).double(), copy.deepcopy(eapp.fc).double()
        y64 = [net64(x.double()) for x in xs]
        es64 = [fc64(torch.flatten(y, start_dim=1)) for y in y64]
        gpu = eapp.to(DEV)
        cases = [(x.to(DEV), gpu.custom_resnet50(x.to(DEV)).clone(), y, gpu.descriptor(x.to(DEV)).clone(), e) for x, y, e in zip(xs, y64, es64)]
    return gpu, cases


def test_whole_net_against_fp64(eapp_case):
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    eapp, cases = eapp_case
    net = eapp.custom_resnet50
    originals, keys = _slots(net), list(eapp.state_dict().keys())
    assert len(originals) == 13 and all(type(b) is E._Bottleneck for b in originals)
    with torch.no_grad():
        try:
            assert M.native_eapp_resnet50(eapp) is True and M.native_eapp_resnet50(eapp) is False
            assert sum(isinstance(m, M.BottleneckFused) for m in eapp.modules()) == 13 and all(isinstance(b, M.BottleneckFused) for b in _slots(net))
            assert list(eapp.state_dict().keys()) == keys
            ops.f16x3_saturation_count(reset=True)
            for x, y_torch, y64, _, _ in cases:
                _check(f"custom_resnet50 {tuple(x.shape)} switched on", net(x), y_torch, y64)
            assert ops.f16x3_saturation_count() == 0
        finally:
            M.native_eapp_resnet50(eapp, False)
        # switched off: the very modules of before (stock torch promises no bitwise reproducibility from call to call: the same accuracy
        # rule, not the same bits)
        assert all(a is b for a, b in zip(originals, _slots(net))) and list(eapp.state_dict().keys()) == keys
        for x, y_torch, y64, _, _ in cases:
            _check(f"custom_resnet50 {tuple(x.shape)} switched off again", net(x), y_torch, y64)


@pytest.mark.parametrize("via", ["eapp", "gbase"])
def test_descriptor_with_native_resnet50(eapp_case, via):
    from megaportrait_hack_amd import gbase, model as M

    eapp, cases = eapp_case
    owner = eapp if via == "eapp" else gbase.Gbase(appearanceEncoder=eapp, motionEncoder=nn.Identity(), G2d=nn.Identity(), image_pyramid=nn.Identity())
    keys = list(owner.state_dict().keys())
    with torch.no_grad():
        try:
            assert owner.native_resnet50() is owner
            assert sum(isinstance(m, M.BottleneckFused) for m in eapp.modules()) == 13 and list(owner.state_dict().keys()) == keys
            got = [eapp.descriptor(x) for x, *_ in cases]
        finally:
            owner.native_resnet50(False)
        assert not any(isinstance(m, M.BottleneckFused) for m in eapp.modules())
    for (x, _, _, es_torch, es64), es in zip(cases, got):
        assert es.shape == es64.shape == (x.shape[0], 512)
        _check(f"Eapp.descriptor {tuple(x.shape)} via {via}", es, es_torch, es64)
