"""Eapp's two 7x7 stems on the matrix cores (model.ConvStem7Fused, model.Stem7Fused, model.native_eapp_stems, Eapp.native_stems,
Gbase.native_stems) against the unswapped modules, with the conventions and the bar of tests/test_gpu_emtn_stem.py:
e_hip <= 4 * e_torch + 2^-22 * max|y64|, e_torch from the unswapped module on the same GPU, y64 the unswapped module in fp64 on the CPU.
Images are 64 x 64 and 40 x 56 (odd and even halvings, not square), B = 2."""
import copy

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
    print(f"eapp stems parity {name}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} max|y64|={y64.abs().max().item():.3e} bound={bound:.3e}")
    assert e_hip <= bound, (name, e_hip, bound)


def _images():
    g = torch.Generator().manual_seed(6)
    return [torch.randn(2, 3, 64, 64, generator=g), torch.randn(2, 3, 40, 56, generator=g)]


def _reference_forward_class():
    from megaportrait_hack_amd import encoders2d as E

    class ReferenceForwardResNet50(E.CustomResNet50):
        """The reference's forward: F.relu between bn1 and maxpool, one statement per step."""

        def forward(self, x):
            x = self.conv1(x)
            x = self.bn1(x)
            x = F.relu(x)
            x = self.maxpool(x)
            x = self.layer1(x)
            x = self.layer2(x)
            x = self.layer3(x)
            x = self.adaptive_avg_pool(x)
            return self.conv_reduce(x)

    return ReferenceForwardResNet50


@pytest.fixture(scope="module")
def eapp_case():
    """(Eapp on the GPU, [(x, trunk_torch, trunk64, es_torch, es64)]): the references are computed once, before any swap."""
    from megaportrait_hack_amd import encoders2d as E

    torch.manual_seed(11)
    eapp = _seed(E.Eapp(), 5).eval()
    xs = _images()
    with torch.no_grad():
        e64 = copy.deepcopy(eapp).double()
        t64 = [e64.trunk2d(x.double()) for x in xs]
        es64 = [e64.descriptor(x.double()) for x in xs]
        gpu = eapp.to(DEV)
        cases = [(x.to(DEV), gpu.trunk2d(x.to(DEV)).clone(), t, gpu.descriptor(x.to(DEV)).clone(), e) for x, t, e in zip(xs, t64, es64)]
    return gpu, cases


def test_swap_keeps_keys_names_and_objects(eapp_case):
    from megaportrait_hack_amd import model as M

    eapp, _ = eapp_case
    net = eapp.custom_resnet50
    conv, conv1, bn1, pool = eapp.conv, net.conv1, net.bn1, net.maxpool
    keys, names, params, bufs = (list(eapp.state_dict().keys()), [n for n, _ in eapp.named_modules()], list(eapp.parameters()),
                                 list(eapp.buffers()))
    try:
        assert M.native_eapp_stems(eapp) is True and M.native_eapp_stems(eapp) is False
        assert isinstance(eapp.conv, M.ConvStem7Fused) and isinstance(net.conv1, M.Stem7Fused)
        assert list(eapp.state_dict().keys()) == keys and [n for n, _ in eapp.named_modules()] == names
        assert all(a is b for a, b in zip(eapp.parameters(), params)) and all(a is b for a, b in zip(eapp.buffers(), bufs))
    finally:
        assert M.native_eapp_stems(eapp, False) is True
    assert eapp.conv is conv and net.conv1 is conv1 and net.bn1 is bn1 and net.maxpool is pool
    assert list(eapp.state_dict().keys()) == keys and [n for n, _ in eapp.named_modules()] == names


def test_conv_slot_is_the_kernel_call_and_carries_a_descriptor(eapp_case):
    from megaportrait_hack_amd import model as M, ops

    eapp, cases = eapp_case
    conv = eapp.conv
    pack = ops.PackedConv2dStem7(conv.weight, conv.bias)
    with torch.no_grad():
        try:
            eapp.native_stems()
            ops.f16x3_saturation_count(reset=True)
            for x, *_ in cases:
                x = x.clone()
                assert eapp.conv._native_ok(x) and ops.tensor_range(x) is None
                y = eapp.conv(x)
                assert ops.tensor_range(x) is not None      # the scan stays on the image: the other stem does not repeat it
                assert y.dtype == torch.float32 and y.shape == (x.shape[0], 64, *x.shape[2:]) and ops.current_range(y) is not None
                assert torch.equal(y, ops.conv2d_stem7(x, pack, stride=1, relu=False, pool=False))
                assert torch.equal(eapp.conv(x.contiguous(memory_format=torch.channels_last)), y)      # NHWC image: copied once
                y_half = eapp.conv(x.half())                                                           # widened, fp32 out
                assert y_half.dtype == torch.float32 and (y_half - y).abs().max().item() < 0.05 * y.abs().max().item()
                _check(f"Eapp.conv {tuple(x.shape)}", y, conv(x), F.conv2d(x.cpu().double(), conv.weight.cpu().double(),
                                                                         conv.bias.cpu().double(), padding=3))
            assert ops.f16x3_saturation_count() == 0
            assert eapp.conv.__dict__["_mphip_pack"] is eapp.conv._pack()      # cached on the parameter versions
        finally:
            eapp.native_stems(False)


@pytest.mark.parametrize("forward", ["package", "reference"])
def test_resnet50_stem_is_one_launch_into_layer1(forward):
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(21)
    cls = E.CustomResNet50 if forward == "package" else _reference_forward_class()
    net = _seed(cls(), 7).eval()
    xs = _images()
    with torch.no_grad():
        y64 = [copy.deepcopy(net).double()(x.double()) for x in xs]
        net = net.to(DEV)
        conv1, bn1, pool = net.conv1, net.bn1, net.maxpool
        y_torch = [net(x.to(DEV)).clone() for x in xs]
        seen = []
        hook = net.layer1.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
        try:
            assert M.Stem7Fused.swap(net) is True and M.Stem7Fused.swap(net) is False
            pack = ops.PackedConv2dStem7(*M.fold_batchnorm(conv1, bn1))
            ops.f16x3_saturation_count(reset=True)
            for x, yt, y in zip(xs, y_torch, y64):
                xg = x.to(DEV)
                del seen[:]
                got = net(xg)
                (t,) = seen
                assert t.dim() == 4 and t.dtype == torch.float32 and ops.current_range(t) is not None
                want = ops.conv2d_stem7(xg, pack, stride=2, relu=True, pool=True)
                assert t.shape == want.shape == (2, 64, (x.shape[2] + 3) // 4, (x.shape[3] + 3) // 4) and torch.equal(t, want)
                assert "_mphip_kept" not in net.conv1.__dict__      # the kept descriptor was used once
                _check(f"custom_resnet50 ({forward} forward) {tuple(x.shape)}", got, yt, y)
            assert ops.f16x3_saturation_count() == 0
            # ordinary 4-D tensors through the stand-ins: the original modules
            t4 = torch.randn(2, 64, 9, 11, device=DEV)
            assert torch.equal(net.maxpool(t4), pool(t4)) and torch.equal(net.bn1(t4), bn1(t4))
            assert ops.tensor_range(net.maxpool(t4)) is None
        finally:
            hook.remove()
            assert M.Stem7Fused.swap(net, False) is True
        assert net.conv1 is conv1 and net.bn1 is bn1 and net.maxpool is pool


@pytest.mark.parametrize("via", ["eapp", "gbase"])
def test_descriptor_and_trunk_with_every_eapp_switch_on(eapp_case, via):
    from megaportrait_hack_amd import gbase, model as M, ops

    eapp, cases = eapp_case
    owner = eapp if via == "eapp" else gbase.Gbase(appearanceEncoder=eapp, motionEncoder=nn.Identity(), G2d=nn.Identity(), image_pyramid=nn.Identity())
    keys = list(owner.state_dict().keys())
    with torch.no_grad():
        try:
            assert owner.native_stems() is owner and owner.native_trunk() is owner and owner.native_resnet50() is owner
            assert isinstance(eapp.conv, M.ConvStem7Fused) and isinstance(eapp.custom_resnet50.conv1, M.Stem7Fused)
            assert isinstance(eapp.resblock_128, M.ResBlockCustomFused) and list(owner.state_dict().keys()) == keys
            ops.f16x3_saturation_count(reset=True)
            got = [(eapp.trunk2d(x), eapp.descriptor(x)) for x, *_ in cases]
            assert ops.f16x3_saturation_count() == 0
        finally:
            owner.native_stems(False), owner.native_trunk(False), owner.native_resnet50(False)
        assert type(eapp.conv) is nn.Conv2d and type(eapp.custom_resnet50.conv1) is nn.Conv2d
    for (x, t_torch, t64, es_torch, es64), (t, es) in zip(cases, got):
        assert t.shape == t64.shape and es.shape == es64.shape == (x.shape[0], 512)
        _check(f"Eapp.trunk2d {tuple(x.shape)} via {via}", t, t_torch, t64)
        _check(f"Eapp.descriptor {tuple(x.shape)} via {via}", es, es_torch, es64)


@pytest.mark.parametrize("mode", ["train", "input_grad", "param_grad", "half"])
def test_fallbacks_are_the_original_expression(mode):
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(3)
    eapp = _seed(E.Eapp(), 4).to(DEV).eval()
    net = eapp.custom_resnet50
    x = torch.randn(2, 3, 40, 56, device=DEV)
    if mode == "train":
        eapp.train()
    if mode == "half":
        eapp, x = eapp.half(), x.half()
    if mode != "param_grad":
        eapp.requires_grad_(mode == "train")
    x.requires_grad_(mode == "input_grad")
    stem = lambda: net.maxpool(F.relu(net.bn1(net.conv1(x))))
    stats = [b.clone() for b in net.bn1.buffers()]
    want_conv, want_stem = eapp.conv(x), stem()
    with torch.no_grad():
        for b, s in zip(net.bn1.buffers(), stats):      # train mode steps the running statistics: rewind, so both see the same state
            b.copy_(s)
    conv1 = net.conv1
    assert M.native_eapp_stems(eapp) is True
    assert not eapp.conv._native_ok(x) and not net.conv1._native_ok(x)
    got_conv, got_stem = eapp.conv(x), stem()
    assert torch.equal(got_conv, want_conv) and torch.equal(got_stem, want_stem) and got_stem.dtype == want_stem.dtype and got_stem.dim() == 4
    assert "_mphip_fold" not in net.conv1.__dict__ and "_mphip_pack" not in eapp.conv.__dict__
    if mode in ("train", "input_grad", "param_grad"):
        (got_conv.square().sum() + got_stem.square().sum()).backward()
        if mode == "input_grad":
            assert x.grad is not None and x.grad.abs().max() > 0
        else:
            assert conv1.weight.grad is not None and conv1.weight.grad.abs().max() > 0      # the net's own Parameters
    assert M.native_eapp_stems(eapp, False) is True and net.conv1 is conv1
