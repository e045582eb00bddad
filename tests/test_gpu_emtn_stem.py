"""The stems of Emtn's two ResNet-18s as one launch each (model.StemFused, model.native_emtn_stems, Emtn.native_resnets(fuse_stem=True))
against the unswapped modules in fp64 on the CPU, with the bar of tests/test_gpu_emtn_resnets.py: e_hip <= 4 * e_torch + 2^-22 * max|y64|,
e_torch from the unswapped module on the same GPU.  The stem alone is exact fp32 with a fixed order: it is compared bitwise with
ops.conv2d_stem on the folded weights.  Stock torch promises no bitwise reproducibility from call to call on whole nets (its conv backend
picks the solver at run time: with MIOpen in its default immediate mode, torch.backends.cudnn.benchmark off, the second and third call of
the unswapped BasicBlocks of a CifarResNet18 on one [2,64,19,25] map — the fused stem's output, the same bits both times — gave different
bits; which solver changed between the calls was not looked up), so "switching off restores the
unswapped outputs" is held bitwise on the four stem modules, whose outputs the switch decides, and by object identity and the accuracy rule on
whole nets, as tests/test_gpu_emtn_resnets.py does."""
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
    print(f"emtn stem parity {name}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} max|y64|={y64.abs().max().item():.3e} bound={bound:.3e}")
    assert e_hip <= bound, (name, e_hip, bound)


def _image(seed=6):
    return torch.rand(2, 3, 37, 50, generator=torch.Generator().manual_seed(seed)) * 2 - 1


@pytest.fixture(scope="module")
def net_case():
    """(CifarResNet18 on the GPU, x, y_torch, y64): the references are computed once, before any swap."""
    from megaportrait_hack_amd import encoders2d as E

    torch.manual_seed(11)
    net = _seed(E.CifarResNet18(num_classes=6), 5).eval()
    x = _image()
    with torch.no_grad():
        y64 = copy.deepcopy(net).double()(x.double())
        gpu = net.to(DEV)
        y_torch = gpu(x.to(DEV)).clone()
    return gpu, x.to(DEV), y_torch, y64


@pytest.mark.parametrize("blocks", [False, True], ids=["stem_alone", "stem_and_blocks"])
def test_whole_net_against_fp64(net_case, blocks):
    from megaportrait_hack_amd import model as M, ops

    net, x, y_torch, y64 = net_case
    holder = types.SimpleNamespace(head_pose_net=net, expression_net=None)
    keys, names, originals = list(net.state_dict().keys()), [n for n, _ in net.named_modules()], list(net.children())
    with torch.no_grad():
        try:
            assert M.native_emtn_stems(holder) is True and M.native_emtn_stems(holder) is False
            assert blocks is False or M.native_emtn_resnets(holder) is True
            assert isinstance(net.conv1, M.StemFused) and sum(isinstance(m, M.BasicBlockFused) for m in net.modules()) == (8 if blocks else 0)
            assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_modules()] == names
            ops.f16x3_saturation_count(reset=True)
            y = net(x)
            assert "_mphip_fold" in net.conv1.__dict__                      # the native path ran
            _check(f"CifarResNet18 {tuple(x.shape)} stem{' + blocks' if blocks else ''}", y, y_torch, y64)
            assert ops.f16x3_saturation_count() == 0
        finally:
            M.native_emtn_resnets(holder, False)
            M.native_emtn_stems(holder, False)
        # switched off: the very modules of before, and the same accuracy rule
        assert all(a is b for a, b in zip(originals, net.children())) and list(net.state_dict().keys()) == keys
        _check(f"CifarResNet18 {tuple(x.shape)} switched off again", net(x), y_torch, y64)


def test_switching_off_restores_the_stem_bitwise():
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(14)
    emtn = _seed(E.Emtn(), 9).to(DEV).eval()
    x = _image(10).to(DEV)
    stems = {"head_pose_net": lambda: emtn.head_pose_net.maxpool(emtn.head_pose_net.relu(emtn.head_pose_net.bn1(emtn.head_pose_net.conv1(x)))),
             "expression_net": lambda: emtn.expression_net[:4](x)}
    with torch.no_grad():
        want = {k: f().clone() for k, f in stems.items()}
        slots = [emtn.head_pose_net.conv1, emtn.head_pose_net.bn1, emtn.head_pose_net.relu, emtn.head_pose_net.maxpool, *emtn.expression_net[:4]]
        assert M.native_emtn_stems(emtn) is True
        on = {k: f() for k, f in stems.items()}
        assert M.native_emtn_stems(emtn, False) is True
        now = [emtn.head_pose_net.conv1, emtn.head_pose_net.bn1, emtn.head_pose_net.relu, emtn.head_pose_net.maxpool, *emtn.expression_net[:4]]
        assert all(a is b for a, b in zip(slots, now))
        for k, f in stems.items():
            assert torch.equal(f(), want[k]), k                             # the unswapped outputs, bit for bit
            assert (on[k] - want[k]).abs().max().item() < 1e-4 * want[k].abs().max().item()     # (the fused launch in between: fp32 rounding apart)


def test_the_stem_alone_is_conv2d_stem_on_the_folded_weights():
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(12)
    emtn = _seed(E.Emtn(), 7).to(DEV).eval()
    x = _image(8).to(DEV)
    with torch.no_grad():
        folds = [M.fold_batchnorm(*s) for s in ((emtn.head_pose_net.conv1, emtn.head_pose_net.bn1), tuple(emtn.expression_net[:2]))]
        want = [ops.conv2d_stem(x, w, b, relu=True, pool=True) for w, b in folds]
        assert M.native_emtn_stems(emtn) is True
        try:
            hp = emtn.head_pose_net
            y = hp.conv1(x)
            assert y.__dict__.get("_mphip_stem") is hp.conv1 and ops.tensor_range(y) is not None
            version = y._version
            z = hp.maxpool(hp.relu(hp.bn1(y)))
            assert z is y and y._version == version and "_mphip_stem" not in y.__dict__ and ops.tensor_range(z) is not None
            assert torch.equal(z, want[0]) and z.shape == (2, 64, 19, 25)
            e = emtn.expression_net[:4](x)
            assert torch.equal(e, want[1]) and ops.tensor_range(e) is not None and "_mphip_stem" not in e.__dict__
            # an unmarked tensor goes through the original modules
            t = torch.randn(2, 64, 9, 9, device=DEV)
            assert torch.equal(hp.maxpool(t), nn.functional.max_pool2d(t, 3, 2, 1)) and torch.equal(hp.relu(t.clone()), t.clamp_min(0))
            # NHWC and half images: copied / widened, the same launch
            assert torch.equal(hp.maxpool(hp.relu(hp.bn1(hp.conv1(x.contiguous(memory_format=torch.channels_last))))), want[0])
            zh = hp.maxpool(hp.relu(hp.bn1(hp.conv1(x.half()))))
            assert zh.dtype == torch.float32 and torch.equal(zh, ops.conv2d_stem(x.half().float(), *folds[0]))
        finally:
            M.native_emtn_stems(emtn, False)


@pytest.mark.parametrize("mode", ["train", "half", "input_grad", "param_grad"])
def test_fallbacks_are_the_original_modules(mode):
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(3)
    net = _seed(E.CifarResNet18(num_classes=6), 4).to(DEV).eval()
    x = _image(9).to(DEV)
    if mode == "train":
        net.train()
    if mode == "half":
        net, x = net.half(), x.half()
    if mode != "param_grad":
        net.requires_grad_(mode == "train")
    x.requires_grad_(mode == "input_grad")
    stem = lambda n: n.maxpool(n.relu(n.bn1(n.conv1(x))))
    stats = [b.clone() for b in net.buffers()]
    want = stem(net)
    for b, s in zip(net.buffers(), stats):      # train mode steps the running statistics: rewind, so both see the same state
        b.copy_(s)
    assert M.StemFused.swap(net) is True
    try:
        assert not net.conv1._native_ok(x)
        got = stem(net)
        assert torch.equal(got, want) and got.dtype == want.dtype and "_mphip_fold" not in net.conv1.__dict__
        if mode != "half":
            got.square().sum().backward()
            assert (x.grad if mode == "input_grad" else net.bn1.weight.grad).abs().max() > 0
    finally:
        assert M.StemFused.swap(net, False) is True


def test_emtn_forward_with_stems_and_resnets():
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(13)
    emtn = _seed(E.Emtn(), 7).eval()
    x = _image(8)
    with torch.no_grad():
        pose64, expr64, fc64 = (copy.deepcopy(m).double() for m in (emtn.head_pose_net, emtn.expression_net, emtn.fc))
        t64 = pose64(x.double())[:, 3:]
        e64 = fc64(torch.flatten(expr64(x.double()), start_dim=1))
        gpu = emtn.to(DEV)
        rot_t, t_torch, e_torch = gpu(x.to(DEV))
        keys = list(gpu.state_dict().keys())
        try:
            assert gpu.native_resnets(True, fuse_stem=True) is gpu
            assert sum(isinstance(m, M.StemFused) for m in gpu.modules()) == 2 and sum(isinstance(m, M.BasicBlockFused) for m in gpu.modules()) == 16
            assert list(gpu.state_dict().keys()) == keys
            rot, t_hip, e_hip = gpu(x.to(DEV))
            assert "_mphip_fold" in gpu.head_pose_net.conv1.__dict__ and "_mphip_fold" in gpu.expression_net[0].__dict__
        finally:
            gpu.native_resnets(False)
        assert not any(isinstance(m, (M.StemFused, M._StemPass, M.BasicBlockFused)) for m in gpu.modules())
        _, t_off, e_off = gpu(x.to(DEV))
    assert rot.shape == rot_t.shape == (2, 3) and t_hip.shape == (2, 3) and e_hip.shape == e64.shape
    _check("Emtn.forward translation", t_hip, t_torch, t64)
    _check("Emtn.forward expression", e_hip, e_torch, e64)
    _check("Emtn.forward translation, switched off again", t_off, t_torch, t64)
    _check("Emtn.forward expression, switched off again", e_off, e_torch, e64)
