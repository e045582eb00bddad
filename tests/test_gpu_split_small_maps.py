"""The split_small_maps switches (model.BasicBlockFused / RepVGGBlockFused .split_small_maps, model.native_emtn_resnets,
model.native_rotation_net): the fused blocks' stride-1 convs launched with splits="auto" (csrc/conv2d_splitk_f16x3.hip), with the nets and
the setup of tests/test_gpu_emtn_resnets.py and tests/test_gpu_rotation_net.py.  Results are held to the bar of DESIGN 3.9 against the
unswapped modules in fp64 on the CPU: e_hip <= 4 * e_torch + 2^-22 * max|y64|, e_torch from the unswapped module on the same GPU.  Every
case asserts that a launch really took more than one split, and that without the keyword the outputs are the bits of the switched-on
path as it was."""
import copy
import types

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _check(name, y_hip, y_torch, y64):
    e_hip = (y_hip.cpu().double() - y64).abs().max().item()
    e_torch = (y_torch.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -22 * y64.abs().max().item()
    print(f"split_small_maps parity {name}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} max|y64|={y64.abs().max().item():.3e} bound={bound:.3e}")
    assert e_hip <= bound, (name, e_hip, bound)


def _seed_bn(module, seed):
    """tests/test_gpu_emtn_resnets.py: BatchNorm statistics and affine moved away from their initial values."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.5)
    return module


def _he(net, seed):
    """tests/test_gpu_rotation_net.py: He initialisation of every conv, small biases where a conv has one."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu", generator=g)
                if m.bias is not None:
                    m.bias.normal_(0.0, 0.1, generator=g)
    return net


class _Recorder:
    """Wraps ops.conv2d_splits: the recommendations handed out while it is installed."""

    def __enter__(self):
        from megaportrait_hack_amd import ops

        self.ops, self.orig, self.seen = ops, ops.conv2d_splits, []

        def wrapped(*shape):
            s = self.orig(*shape)
            self.seen.append((shape, s))
            return s

        ops.conv2d_splits = wrapped
        return self

    def __exit__(self, *exc):
        self.ops.conv2d_splits = self.orig


def test_basic_block_at_1x256x16x16():
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(41)
    blk = _seed_bn(E._BasicBlock(256, 256, 1), 1).eval()
    x = torch.randn(1, 256, 16, 16)
    with torch.no_grad():
        y64 = copy.deepcopy(blk).double()(x.double())
        gpu, xg = blk.to(DEV), x.to(DEV)
        y_torch = gpu(xg)
        fused = M.BasicBlockFused.from_block(gpu)
        y_on = fused(xg)                                   # the switched-on path as it is
        s = ops.conv2d_splits(1, 256, 256, 16, 16)
        assert s > 1 and ops.conv2d_split_supported(1, 256, 256, 16, 16, 1, s)
        fused.split_small_maps = True
        ops.f16x3_saturation_count(reset=True)
        with _Recorder() as rec:
            y_split = fused(xg)
        assert rec.seen == [((1, 256, 256, 16, 16, 1), s)] * 2          # both convs asked, both split
        assert ops.tensor_range(y_split) is not None and y_split.dtype == torch.float32 and y_split.is_contiguous()
        _check("BasicBlock 256 at 16 x 16", y_split, y_torch, y64)
        # the two launches, by hand, on the block's cached fold
        p1, p2, ps = fused.__dict__["_mphip_fold"][1]
        assert ps is None
        by_hand = ops.conv2d(ops.conv2d(xg, p1, relu=True, want_range=True, splits=s), p2, residual=xg, relu=True, splits=s)
        assert torch.equal(y_split, by_hand) and torch.equal(fused(xg), y_split)
        assert ops.f16x3_saturation_count() == 0
        del fused.split_small_maps                          # keyword off: the bits of before
        with _Recorder() as rec:
            assert torch.equal(fused(xg), y_on) and rec.seen == []


@pytest.mark.parametrize("groups", [1, 2], ids=["plain", "groups2"])
def test_repvgg_block_at_1x512x8x8(groups):
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(43 + groups)
    blk = E._RepVGGDeployBlock(512, 512, 1, groups).eval()
    x = torch.randn(1, 512, 8, 8)
    with torch.no_grad():
        y64 = copy.deepcopy(blk).double()(x.double())
        gpu, xg = blk.to(DEV), x.to(DEV)
        y_torch = gpu(xg)
        fused = M.RepVGGBlockFused.from_block(gpu)
        y_on = fused(xg)
        s = ops.conv2d_splits(1, 512, 512, 8, 8, groups)
        assert s > 1
        fused.split_small_maps = True
        ops.f16x3_saturation_count(reset=True)
        with _Recorder() as rec:
            y_split = fused(xg)
        assert rec.seen == [((1, 512, 512, 8, 8, groups), s)]
        _check(f"RepVGG block 512 at 8 x 8, groups {groups}", y_split, y_torch, y64)
        conv = gpu.rbr_reparam
        pack = ops.PackedConv2d(conv.weight, conv.bias, groups)
        op = ops.conv2d if groups == 1 else ops.conv2d_grouped
        assert torch.equal(y_split, op(xg, pack, relu=True, splits=s)) and ops.tensor_range(y_split) is not None
        assert ops.f16x3_saturation_count() == 0
        fused.split_small_maps = False
        assert torch.equal(fused(xg), y_on) and torch.equal(y_on, op(xg, pack, relu=True))


def test_cifar_resnet18():
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(11)
    net = _seed_bn(E.CifarResNet18(num_classes=6), 5).eval()      # (He-initialised by its constructor)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(6))      # layer4 runs at 2 x 2
    holder = types.SimpleNamespace(head_pose_net=net, expression_net=None)
    with torch.no_grad():
        y64 = copy.deepcopy(net).double()(x.double())
        gpu, xg = net.to(DEV), x.to(DEV)
        y_torch = gpu(xg).clone()
        originals = [b for s in gpu.children() if isinstance(s, nn.Sequential) for b in s]
        try:
            assert M.native_emtn_resnets(holder) is True
            y_on = gpu(xg).clone()                          # today's switched-on path
            assert M.native_emtn_resnets(holder, True, split_small_maps=True) is True
            ops.f16x3_saturation_count(reset=True)
            with _Recorder() as rec:
                y_split = gpu(xg)
            assert len(rec.seen) == 13 and max(s for _, s in rec.seen) > 1, rec.seen      # 16 convs less the three at stride 2
            _check("CifarResNet18 (2, 3, 32, 32)", y_split, y_torch, y64)
            assert torch.equal(gpu(xg), y_split) and ops.f16x3_saturation_count() == 0
            assert M.native_emtn_resnets(holder, True) is True                          # keyword off
            with _Recorder() as rec:
                assert torch.equal(gpu(xg), y_on) and rec.seen == []
        finally:
            M.native_emtn_resnets(holder, False)
        assert all(a is b for a, b in zip(originals, [b for s in gpu.children() if isinstance(s, nn.Sequential) for b in s]))


def test_rotation_net_backbone_at_64x64():
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(3)
    net = _he(E.SixDRepNetBackbone(), 3).eval()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(8)) * 2 - 1
    feats = lambda n, v: n.linear_reg(torch.flatten(n.gap(n.layer4(n.layer3(n.layer2(n.layer1(n.layer0(v)))))), 1))
    with torch.no_grad():
        p64 = feats(copy.deepcopy(net).double(), x.double())
        gpu, xg = net.to(DEV), x.to(DEV)
        for p in gpu.parameters():
            p.requires_grad_(False)
        p_torch = feats(gpu, xg).clone()
        try:
            assert M.native_rotation_net(gpu) is True
            p_on = feats(gpu, xg).clone()                   # today's switched-on path
            assert M.native_rotation_net(gpu, True, split_small_maps=True) is True
            ops.f16x3_saturation_count(reset=True)
            with _Recorder() as rec:
                p_split = feats(gpu, xg)
            assert len(rec.seen) == 23 and max(s for _, s in rec.seen) > 1, rec.seen      # 27 blocks less the four at stride 2
            assert any(shape[5] == 2 and s > 1 for shape, s in rec.seen) and any(shape[5] == 1 and s > 1 for shape, s in rec.seen)
            _check("SixDRepNetBackbone linear_reg (2, 3, 64, 64)", p_split, p_torch, p64)
            assert torch.equal(feats(gpu, xg), p_split) and ops.f16x3_saturation_count() == 0
            assert M.native_rotation_net(gpu, True) is True                             # keyword off
            with _Recorder() as rec:
                assert torch.equal(feats(gpu, xg), p_on) and rec.seen == []
        finally:
            M.native_rotation_net(gpu, False)
        assert not any(isinstance(m, M.RepVGGBlockFused) for m in gpu.modules())
