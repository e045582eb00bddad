"""6DRepNet's RepVGG backbone on the matrix cores (model.RepVGGBlockFused, model.native_rotation_net, Emtn.native_rotation_net) against
the unswapped modules in fp64 on the CPU.  Tolerance rule of the project for a different summation order (tests/test_gpu_emtn_resnets.py,
DESIGN 3.9 and 3.11): e_hip <= 4 * e_torch + floor, floor = 2^-22 * max|y64| (2^-22 * 180 for angles in degrees), e_torch from the
unswapped module on the same GPU."""
import copy
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NET_SEED, IMG_SEED = 3, 8      # chosen so that the fp64 6-D head is far from degenerate (asserted in net_case)


def _check(name, y_hip, y_torch, y64, scale=None):
    e_hip = (y_hip.cpu().double() - y64).abs().max().item()
    e_torch = (y_torch.cpu().double() - y64).abs().max().item()
    scale = y64.abs().max().item() if scale is None else scale
    bound = 4 * e_torch + 2.0 ** -22 * scale
    print(f"rotation net parity {name}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} scale={scale:.3e} bound={bound:.3e}")
    assert e_hip <= bound, (name, e_hip, bound)


def _reinit(net, seed):
    """Activations stay O(1) through 28 ReLU layers: He initialisation of every conv, small biases."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu", generator=g)
                m.bias.normal_(0.0, 0.1, generator=g)
    return net


@pytest.mark.parametrize("ci,co,stride,groups", [(128, 128, 1, 1), (128, 128, 1, 2), (64, 128, 2, 1)], ids=["g1s1", "g2s1", "g1s2"])
def test_one_block_of_each_kind(ci, co, stride, groups):
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(ci + co + stride + groups)
    blk = E._RepVGGDeployBlock(ci, co, stride, groups).eval()
    x = torch.randn(2, ci, 24, 20)
    with torch.no_grad():
        y64 = copy.deepcopy(blk).double()(x.double())
        gpu = blk.to(DEV)
        xg = x.to(DEV)
        y_torch = gpu(xg)
        fused = M.RepVGGBlockFused.from_block(gpu)
        ops.f16x3_saturation_count(reset=True)
        y_hip = fused(xg)
        assert fused._native_ok(xg) and "_mphip_fold" in fused.__dict__ and ops.tensor_range(y_hip) is not None
        assert y_hip.dtype == torch.float32 and y_hip.is_contiguous() and y_hip.shape == y64.shape
        _check(f"block {ci}->{co} stride {stride} groups {groups}", y_hip, y_torch, y64)
        conv = gpu.rbr_reparam
        pack = ops.PackedConv2d(conv.weight, conv.bias, groups)
        op = ops.conv2d_s2 if stride == 2 else ops.conv2d if groups == 1 else ops.conv2d_grouped
        assert torch.equal(y_hip, op(xg, pack, relu=True))      # one launch: the matching ops call on the block's own weight and bias
        fold = fused.__dict__["_mphip_fold"]
        assert torch.equal(fused(xg), y_hip) and fused.__dict__["_mphip_fold"] is fold      # same bits twice, the pack cached
        _check("channels_last input", fused(xg.contiguous(memory_format=torch.channels_last)), y_torch, y64)      # copied to NCHW once
        x16 = x.half()                                                                                              # widened, fp32 out
        y_half = fused(x16.to(DEV))
        assert y_half.dtype == torch.float32
        _check("fp16 input", y_half, gpu(x16.float().to(DEV)), copy.deepcopy(blk).cpu().double()(x16.double()))
    assert ops.f16x3_saturation_count() == 0


def test_unsupported_shape_takes_the_pytorch_expression():
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(2)
    blk = E._RepVGGDeployBlock(128, 128, 1, 4).to(DEV).eval()      # four groups at width 128: 32 output channels per group
    x = torch.randn(1, 128, 8, 8, device=DEV)
    fused = M.RepVGGBlockFused.from_block(blk)
    with torch.no_grad():
        assert not fused._native_ok(x) and torch.equal(fused(x), blk(x)) and "_mphip_fold" not in fused.__dict__


def _features(net, x):
    feat = net.layer4(net.layer3(net.layer2(net.layer1(net.layer0(x)))))
    return feat, net.linear_reg(torch.flatten(net.gap(feat), 1))


def _degrees64(n64, x):
    """SixDRepNet_Detector.predict in fp64 (the detector itself casts its image to fp32)."""
    from megaportrait_hack_amd import encoders2d as E

    return E.euler_from_matrix(n64(x.cpu().double())[0]) * 180.0 / math.pi


@pytest.fixture(scope="module")
def net_case():
    """(backbone on the GPU, image, torch's results on the GPU, fp64 results): the references are computed once, before any swap."""
    from megaportrait_hack_amd import encoders2d as E

    torch.manual_seed(NET_SEED)
    net = _reinit(E.SixDRepNetBackbone(), NET_SEED).eval()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(IMG_SEED)) * 2 - 1
    with torch.no_grad():
        n64 = copy.deepcopy(net).double()
        feat64, p64 = _features(n64, x.double())
        # the 6-D head of the fp64 reference is not near-degenerate: |unit(a) x b| / |b| (ortho6d_to_matrix, before its normalisation)
        a, b = p64[:, 0:3], p64[:, 3:6]
        sin = torch.cross(a / a.norm(dim=1, keepdim=True), b, dim=1).norm(dim=1) / b.norm(dim=1)
        assert sin.min().item() >= 0.1, sin
        deg64 = _degrees64(n64, x)
        gpu = net.to(DEV)
        for p in gpu.parameters():
            p.requires_grad_(False)
        xg = x.to(DEV)
        feat_t, p_t = _features(gpu, xg)
        deg_t, _ = E.SixDRepNet_Detector(gpu).predict(xg)
    return gpu, xg, (feat_t.clone(), p_t.clone(), deg_t.clone()), (feat64, p64, deg64), n64


def _slots(net):
    return [net.layer0] + [b for s in (net.layer1, net.layer2, net.layer3, net.layer4) for b in s]


def test_whole_net_against_fp64(net_case):
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    net, x, (feat_t, p_t, deg_t), (feat64, p64, deg64), n64 = net_case
    originals, keys, names = _slots(net), list(net.state_dict().keys()), [n for n, _ in net.named_modules()]
    det = E.SixDRepNet_Detector(net)
    emtn = E.Emtn(rotation_net=det).to(DEV).eval()
    with torch.no_grad():
        try:
            assert emtn.native_rotation_net() is emtn and M.native_rotation_net(det) is False
            assert sum(isinstance(m, M.RepVGGBlockFused) for m in net.modules()) == 27 and _slots(net)[0] is originals[0]
            assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_modules()] == names
            ops.f16x3_saturation_count(reset=True)
            feat, p = _features(net, x)
            assert all(b._native_ok(torch.empty(2, b.rbr_reparam.in_channels, 8, 8, device=DEV)) for b in _slots(net)[1:])
            _check("layer4 map", feat, feat_t, feat64)
            _check("linear_reg", p, p_t, p64)
            deg, _ = det.predict(x)
            _check("SixDRepNet_Detector.predict (degrees)", deg, deg_t, deg64, scale=180.0)
            rot, _, _ = emtn(x)
            _check("Emtn.forward rotations (degrees)", rot, deg_t, deg64, scale=180.0)
            _check("channels_last image", _features(net, x.contiguous(memory_format=torch.channels_last))[1], p_t, p64)
            x16 = x.half()                                   # an fp16 image into the fp32 net: the detector widens it
            deg16, _ = det.predict(x16)
            assert ops.f16x3_saturation_count() == 0
        finally:
            emtn.native_rotation_net(False)
        # switched off: the very modules of before
        assert all(a is b for a, b in zip(originals, _slots(net))) and list(net.state_dict().keys()) == keys
        assert not any(isinstance(m, M.RepVGGBlockFused) for m in net.modules())
        _check("fp16 image (degrees)", deg16, det.predict(x16)[0], _degrees64(n64, x16), scale=180.0)
        _check("switched off again", _features(net, x)[1], p_t, p64)


@pytest.fixture
def deterministic_convs():
    """Stock torch's fp32 convs do not reproduce their own bits from one call to the next on the MI355X by default (measured on this
    net in grad mode: `layer1(layer0(x))` of the unswapped net differed between its first three calls by 9.5e-7 and 1.2e-6, and one
    64 -> 128 stride-2 block differed from itself on the same input tensor), so nothing can be torch.equal to them.  The fall-back tests
    ask the conv backend for its deterministic solvers, for the reference and for the swapped net alike."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before


@pytest.mark.parametrize("mode", ["train", "input_grad", "half"])
def test_fallbacks_are_the_original_forward(mode, deterministic_convs):
    """A swapped net in train mode, under autograd and as a half module takes the PyTorch expression: its outputs are torch.equal to
    the unswapped net's, and each swapped block's to those of the block it replaced on the same input tensor."""
    from megaportrait_hack_amd import encoders2d as E, model as M

    net = _reinit(E.SixDRepNetBackbone(), 5).to(DEV).eval()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(DEV) * 2 - 1
    if mode == "train":
        net.train()
    if mode == "half":
        net, x = net.half(), x.half()
    net.requires_grad_(mode == "train")
    x.requires_grad_(mode == "input_grad")
    originals = _slots(net)[1:]
    with torch.set_grad_enabled(mode != "half"):
        want_rot, want_rest = net(x)
        assert M.native_rotation_net(net) is True
        blocks = _slots(net)[1:]
        assert len(blocks) == 27 and all(isinstance(b, M.RepVGGBlockFused) and b.training == (mode == "train") for b in blocks)
        rot, rest = net(x)
        h = net.layer0(x)
        for i, (orig, fused) in enumerate(zip(originals, blocks)):
            assert not fused._native_ok(h), i
            want = orig(h)
            got = fused(h)
            print(f"rotation net fall-back {mode} block {i}: max|got - want| = {(got - want).abs().max().item():.3e}")
            assert torch.equal(got, want) and got.dtype == want.dtype and got.requires_grad == want.requires_grad, (mode, i)
            h = want
    print(f"rotation net fall-back {mode}: max|rot - want_rot| = {(rot - want_rot).abs().max().item():.3e}")
    assert torch.equal(rot, want_rot) and torch.equal(rest, want_rest) and rot.dtype == want_rot.dtype == x.dtype
    assert not any("_mphip_fold" in b.__dict__ for b in blocks)
    if mode != "half":
        (rot * torch.linspace(-1.0, 1.0, 9, device=DEV).view(3, 3)).sum().backward()      # (sum of squares of a rotation is constant)
        if mode == "input_grad":
            assert x.grad is not None and x.grad.abs().max() > 0
        else:
            w = net.layer3[1].rbr_reparam.weight      # a grouped block's own Parameter
            assert w.grad is not None and w.grad.abs().max() > 0
    assert M.native_rotation_net(net, False) is True and all(a is b for a, b in zip(originals, _slots(net)[1:]))
