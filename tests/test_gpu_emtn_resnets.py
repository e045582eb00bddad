"""Emtn's two ResNet-18s on the matrix cores (model.BasicBlockFused, model.native_emtn_resnets, Emtn.native_resnets) against the unswapped
modules in fp64 on the CPU.  Tolerance rule of the project for a different summation order (tests/test_gpu_g2d_body.py):
e_hip <= 4 * e_torch + floor, floor = 2^-22 * max|y64|, e_torch from the unswapped module on the same GPU."""
import copy
import types

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
    print(f"emtn resnets parity {name}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} max|y64|={y64.abs().max().item():.3e} bound={bound:.3e}")
    assert e_hip <= bound, (name, e_hip, bound)


@pytest.mark.parametrize("ci,co,stride,shape", [(64, 64, 1, (2, 64, 9, 11)), (64, 128, 2, (2, 64, 9, 11)), (64, 128, 2, (1, 64, 16, 18)),
                                                (256, 512, 2, (1, 256, 4, 4))])
def test_fused_block_against_fp64(ci, co, stride, shape):
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(ci + co + stride)
    blk = _seed(E._BasicBlock(ci, co, stride), 1).eval()
    x = torch.randn(*shape)
    with torch.no_grad():
        y64 = copy.deepcopy(blk).double()(x.double())
        gpu = blk.to(DEV)
        y_torch = gpu(x.to(DEV))
        fused = M.BasicBlockFused.from_block(gpu)
        ops.f16x3_saturation_count(reset=True)
        y_hip = fused(x.to(DEV))
        assert fused._native_ok(x.to(DEV)) and "_mphip_fold" in fused.__dict__ and ops.tensor_range(y_hip) is not None
        assert y_hip.dtype == torch.float32 and y_hip.is_contiguous() and y_hip.shape == y64.shape
        _check(f"block {ci}->{co} stride {stride} {shape}", y_hip, y_torch, y64)
        fold = fused.__dict__["_mphip_fold"]
        assert torch.equal(fused(x.to(DEV)), y_hip) and fused.__dict__["_mphip_fold"] is fold   # same bits twice, the fold cached
        assert torch.equal(fused(x.to(DEV).contiguous(memory_format=torch.channels_last)), y_hip)   # NHWC input: copied once
        y_half = fused(x.to(DEV).half())                                                        # autocast upstream: widened, fp32 out
        assert y_half.dtype == torch.float32 and (y_half - y_hip).abs().max().item() < 0.05 * y_hip.abs().max().item()
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("mode", ["train", "input_grad", "param_grad", "half"])
def test_fallbacks_are_the_original_forward(mode):
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(3)
    blk = _seed(E._BasicBlock(32, 64, 2), 4).to(DEV).eval()
    x = torch.randn(2, 32, 9, 11, device=DEV)
    if mode == "train":
        blk.train()
    if mode == "half":
        blk, x = blk.half(), x.half()
    if mode != "param_grad":
        blk.requires_grad_(mode == "train")
    x.requires_grad_(mode == "input_grad")
    fused = M.BasicBlockFused.from_block(blk)
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
            assert blk.conv1.weight.grad is not None and blk.downsample[1].weight.grad.abs().max() > 0   # the block's own Parameters


def _stages(net):
    return [s for s in net.children() if isinstance(s, nn.Sequential)]


@pytest.fixture(scope="module", params=["cifar_resnet18", "expression_net"])
def net_case(request):
    """(net on the GPU, [(x, y_torch, y64)] for both input sizes): the references are computed once, before any swap."""
    from megaportrait_hack_amd import encoders2d as E

    torch.manual_seed(11)
    net = E.CifarResNet18(num_classes=6) if request.param == "cifar_resnet18" else E.Emtn().expression_net
    net = _seed(net, 5).eval()
    g = torch.Generator().manual_seed(6)
    # 32 x 32: layer4 runs at 2 x 2.  72 x 56: 72 -> 36 -> 18 -> 9 -> 5 and 56 -> 28 -> 14 -> 7 -> 4: odd and even halvings, non-square
    xs = [torch.randn(2, 3, 32, 32, generator=g), torch.randn(1, 3, 72, 56, generator=g)]
    with torch.no_grad():
        n64 = copy.deepcopy(net).double()
        y64 = [n64(x.double()) for x in xs]
        gpu = net.to(DEV)
        cases = [(x.to(DEV), gpu(x.to(DEV)).clone(), y) for x, y in zip(xs, y64)]
    return request.param, gpu, cases


def test_whole_net_against_fp64(net_case):
    from megaportrait_hack_amd import model as M, ops

    name, net, cases = net_case
    holder = types.SimpleNamespace(head_pose_net=net, expression_net=None)
    slots = lambda: [b for s in _stages(net) for b in s]
    originals, keys = slots(), list(net.state_dict().keys())
    assert len(_stages(net)) == 4 and len(originals) == 8
    with torch.no_grad():
        try:
            assert M.native_emtn_resnets(holder) is True and M.native_emtn_resnets(holder) is False
            assert sum(isinstance(m, M.BasicBlockFused) for m in net.modules()) == 8 and all(isinstance(b, M.BasicBlockFused) for b in slots())
            assert list(net.state_dict().keys()) == keys
            ops.f16x3_saturation_count(reset=True)
            for x, y_torch, y64 in cases:
                _check(f"{name} {tuple(x.shape)} switched on", net(x), y_torch, y64)
            assert ops.f16x3_saturation_count() == 0
        finally:
            M.native_emtn_resnets(holder, False)
        # switched off: the very modules of before.  Stock torch promises no bitwise reproducibility from call to call (its conv backend
        # picks the solver at run time), so identity of the objects and the same accuracy rule, not the same bits
        assert all(a is b for a, b in zip(originals, slots())) and list(net.state_dict().keys()) == keys
        for x, y_torch, y64 in cases:
            _check(f"{name} {tuple(x.shape)} switched off again", net(x), y_torch, y64)


def test_emtn_forward_with_native_resnets():
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(13)
    emtn = _seed(E.Emtn(), 7).eval()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(8)) * 2 - 1
    with torch.no_grad():
        pose64, expr64, fc64 = (copy.deepcopy(m).double() for m in (emtn.head_pose_net, emtn.expression_net, emtn.fc))
        t64 = pose64(x.double())[:, 3:]
        e64 = fc64(torch.flatten(expr64(x.double()), start_dim=1))
        gpu = emtn.to(DEV)
        rot_t, t_torch, e_torch = gpu(x.to(DEV))
        keys = list(gpu.state_dict().keys())
        try:
            assert gpu.native_resnets() is gpu
            assert sum(isinstance(m, M.BasicBlockFused) for m in gpu.modules()) == 16 and list(gpu.state_dict().keys()) == keys
            assert not any(isinstance(m, M.BasicBlockFused) for m in gpu.rotation_net.model.modules())
            rot, t_hip, e_hip = gpu(x.to(DEV))
        finally:
            gpu.native_resnets(False)
        assert not any(isinstance(m, M.BasicBlockFused) for m in gpu.modules())
    assert rot.shape == rot_t.shape == (2, 3) and t_hip.shape == (2, 3) and e_hip.shape == e64.shape
    _check("Emtn.forward translation", t_hip, t_torch, t64)
    _check("Emtn.forward expression", e_hip, e_torch, e64)
