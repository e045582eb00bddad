"""Host-side checks of the fused ResNet-18 stem (no GPU): exported symbols (mphip_conv2d_stem_supported, mphip_conv2d_stem_fwd), ABI
version, the shape rule, argument refusals, the register table, module matching, the switches and the CPU fall-back of model.StemFused."""
import copy
import ctypes
import os
import sys

import torch
import torch.nn as nn

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, integration, model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mphip_conv2d_stem_supported", "mphip_conv2d_stem_fwd")
STEM_VGPRS, STEM_LDS_BYTES = 122, 16      # the pooled kernel, DESIGN.md section 3.12


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 24     # the entries exist since ABI 24


def test_shape_rule():
    lib = _lib.load()
    ok = lib.mphip_conv2d_stem_supported
    for bad in [(1, 1, 64, 8, 8), (1, 4, 64, 8, 8), (1, 16, 64, 8, 8), (1, 3, 8, 8, 8), (1, 3, 24, 8, 8), (1, 3, 0, 8, 8), (0, 3, 64, 8, 8),
                (1, 3, 64, 0, 8), (1, 3, 64, 8, 0), (1, 3, 16, 1 << 15, 1 << 16)]:      # the last: H * W = 2^31
        assert ok(*bad, 1) == 0 and ok(*bad, 0) == 0, bad
    for good in [(8, 3, 64, 512, 512), (1, 3, 16, 1, 1)]:
        assert ok(*good, 1) == 1 and ok(*good, 0) == 1, good
    # y = 2 * 64 * 4096 * 4096 = 2^31 elements without the pool, 2^29 with it; x = 2 * 3 * 2^24 fits either way
    assert ok(2, 3, 64, 4096, 4096, 0) == 0 and ok(2, 3, 64, 4096, 4096, 1) == 1
    assert ok(1, 3, 64, 4096, 4096, 0) == 1
    assert ok(64, 3, 16, 4096, 4096, 1) == 0                                             # x: 64 * 3 * 2^24 > 2^31


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q = (ctypes.c_void_p(base + i * 16384) for i in range(2))                    # two disjoint 16 KiB regions: x (and w, bias), y
    fwd = lambda n, ci, co, h, w, x=p, wt=p, b=p, y=q, pool=1: lib.mphip_conv2d_stem_fwd(x, wt, b, y, None, n, ci, co, h, w, 1, pool, None)
    for bad in [(1, 1, 64, 8, 8), (1, 4, 64, 8, 8), (1, 16, 64, 8, 8), (1, 3, 8, 8, 8), (1, 3, 24, 8, 8), (1, 3, 16, 0, 8), (0, 3, 16, 8, 8)]:
        assert fwd(*bad) == -1 and b"conv2d_stem_fwd: unsupported shape" in lib.mphip_last_error(), bad
    for missing in ("x", "wt", "b", "y"):
        assert fwd(1, 3, 16, 8, 8, **{missing: None}) == -1 and b"conv2d_stem_fwd: null pointer" in lib.mphip_last_error()
    # the order of the 2-D entries' shared check: a null pointer is reported before a bad shape, a bad shape before an overlap
    assert fwd(1, 4, 64, 8, 8, x=None) == -1 and b"conv2d_stem_fwd: null pointer" in lib.mphip_last_error()
    assert fwd(1, 3, 24, 8, 8, y=p) == -1 and b"conv2d_stem_fwd: unsupported shape" in lib.mphip_last_error()
    assert fwd(1, 3, 16, 8, 8, x=ctypes.c_void_p(p.value + 2)) == -1 and b"4-byte aligned" in lib.mphip_last_error()
    # x is [1,3,8,8] = 768 bytes; y is [1,16,4,4] = 1024 bytes pooled and [1,16,8,8] = 4096 bytes flat
    at = lambda base_, off: ctypes.c_void_p(base_.value + off)
    for alias in (dict(y=p), dict(y=at(p, 64)), dict(y=at(p, 764)), dict(x=at(q, 1020)), dict(x=at(q, 4092), pool=0)):
        assert fwd(1, 3, 16, 8, 8, **alias) == -1 and b"must not alias" in lib.mphip_last_error(), alias
    assert fwd(1, 3, 16, 8, 8, x=at(q, 1020), pool=0) == -1                          # inside the flat y


def test_kernel_is_in_the_register_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import register_table

    kernels = register_table.collect(["conv2d_stem.hip"])["conv2d_stem.hip"]["kernels"]
    names = [k["demangled"] for k in kernels]
    assert sorted(n.split("<")[0].split("(")[0].split("::")[-1] for n in names) == ["conv2d_stem_kernel", "conv2d_stem_kernel",
                                                                                      "stem_range_init_kernel"], names
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k.get("agpr_count", 0) == 0 and k["vgpr_count"] <= 128                  # four waves per SIMD
    pooled = [k for k in kernels if k["demangled"].startswith("conv2d_stem_kernel<1>")]      # POOL = true
    assert len(pooled) == 1, names
    assert pooled[0]["vgpr_count"] == STEM_VGPRS and pooled[0]["group_segment_fixed_size"] == STEM_LDS_BYTES
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 3.12"):]
    assert f"{STEM_VGPRS} VGPRs" in sec and f"{STEM_LDS_BYTES} B" in sec


class _TorchvisionNet(nn.Module):
    """The head of the reference's resnet.py ResNet with its CIFAR stem, attributes as torchvision names them."""

    def __init__(self, conv=None, bn=None, relu=None, pool=None, co=64):
        super().__init__()
        self.inplanes = co
        self.conv1 = conv if conv is not None else nn.Conv2d(3, co, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = bn if bn is not None else nn.BatchNorm2d(co)
        self.relu = relu if relu is not None else nn.ReLU(inplace=True)
        self.maxpool = pool if pool is not None else nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.fc = nn.Linear(co, 10)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        return self.fc(x.mean(dim=(2, 3)))


def test_matches_accepts_and_rejects_the_right_nets():
    ok = M.StemFused.matches
    assert ok(E.CifarResNet18()) and ok(_TorchvisionNet()) and ok(E.Emtn().expression_net)
    assert ok(_TorchvisionNet(conv=nn.Conv2d(3, 64, 3, padding=1, bias=True)))                      # a bias may be present
    assert ok(_TorchvisionNet(pool=nn.MaxPool2d((3, 3), (2, 2), (1, 1))))
    assert ok(nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), nn.BatchNorm2d(32), nn.ReLU(), nn.MaxPool2d(3, 2, 1)))
    assert not ok(_TorchvisionNet(conv=nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)))        # torchvision's ImageNet stem
    assert not ok(_TorchvisionNet(conv=nn.Conv2d(3, 64, 7, stride=1, padding=3, bias=False)))
    assert not ok(_TorchvisionNet(conv=nn.Conv2d(3, 64, 3, stride=2, padding=1, bias=False)))
    assert not ok(_TorchvisionNet(conv=nn.Conv2d(4, 64, 3, padding=1, bias=False)))
    assert not ok(_TorchvisionNet(conv=nn.Conv2d(16, 64, 3, padding=1, bias=False)))
    assert not ok(_TorchvisionNet(conv=nn.Conv2d(3, 63, 3, padding=1, groups=3, bias=False)))
    assert not ok(_TorchvisionNet(conv=nn.Conv2d(3, 64, 3, padding=1, dilation=1, padding_mode="reflect", bias=False)))
    assert not ok(_TorchvisionNet(conv=nn.Conv2d(3, 64, 3, padding=2, dilation=2, bias=False)))
    assert not ok(_TorchvisionNet(bn=nn.BatchNorm2d(64, track_running_stats=False)))
    assert not ok(_TorchvisionNet(bn=nn.BatchNorm2d(32)))
    assert not ok(_TorchvisionNet(bn=nn.GroupNorm(32, 64)))
    assert not ok(_TorchvisionNet(relu=nn.LeakyReLU(0.1)))
    for pool in (nn.MaxPool2d(2, 2), nn.MaxPool2d(3, 2, 0), nn.MaxPool2d(3, 1, 1), nn.MaxPool2d(3, 2, 1, dilation=2), nn.AvgPool2d(3, 2, 1),
                 nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.MaxPool2d(3, 2, 1, return_indices=True)):
        assert not ok(_TorchvisionNet(pool=pool)), pool
    assert not ok(nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), nn.BatchNorm2d(32), nn.ReLU())) and not ok(nn.Conv2d(3, 64, 3)) and not ok(None)
    fused = E.CifarResNet18()
    assert M.StemFused.swap(fused) is True and not ok(fused)                                        # already fused


def _seed_bn(module, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g))
                m.weight.copy_(torch.randn(m.num_features, generator=g))
                m.bias.copy_(torch.randn(m.num_features, generator=g))
    return module


def _stem(net):
    return [net[i] for i in range(4)] if isinstance(net, nn.Sequential) else [net.conv1, net.bn1, net.relu, net.maxpool]


def _describe(m):
    return (list(m.state_dict().keys()), [n for n, _ in m.named_modules()], [n for n, _ in m.named_parameters()], list(m.parameters()),
            [n for n, _ in m.named_buffers()], list(m.buffers()))


def _same(a, b):
    return a[:3] == b[:3] and a[4] == b[4] and all(x is y for x, y in zip(a[3], b[3])) and all(x is y for x, y in zip(a[5], b[5]))


def test_switches_are_off_by_default_and_leave_keys_names_and_objects_alone():
    emtn = E.Emtn()
    nets = (emtn.head_pose_net, emtn.expression_net)
    before, stems = _describe(emtn), [_stem(n) for n in nets]
    assert all(type(s[0]) is nn.Conv2d and type(s[3]) is nn.MaxPool2d for s in stems)
    assert M.native_emtn_resnets(emtn) is True                                                      # the blocks alone leave the stems
    assert all(type(_stem(n)[0]) is nn.Conv2d and type(_stem(n)[3]) is nn.MaxPool2d for n in nets)
    assert M.native_emtn_resnets(emtn, False) is True
    assert M.native_emtn_stems(emtn) is True and M.native_emtn_stems(emtn) is False                 # twice: nothing left to swap
    for n in nets:
        head, bn, relu, pool = _stem(n)
        assert isinstance(head, M.StemFused) and all(isinstance(m, M._StemPass) and m._head is head for m in (bn, relu, pool))
    assert sum(isinstance(m, M.StemFused) for m in emtn.modules()) == 2
    assert _same(_describe(emtn), before)
    assert copy.deepcopy(emtn).state_dict().keys() == emtn.state_dict().keys()
    assert emtn.state_dict()._metadata["head_pose_net.bn1"]["version"] == nn.BatchNorm2d._version == 2
    assert M.native_emtn_stems(emtn, False) is True and M.native_emtn_stems(emtn, False) is False
    assert all(a is b for s, n in zip(stems, nets) for a, b in zip(s, _stem(n))) and _same(_describe(emtn), before)
    # Emtn.native_resnets: the stems only with the keyword, and back with enable off or without it
    assert emtn.native_resnets() is emtn and not any(isinstance(m, M.StemFused) for m in emtn.modules())
    assert emtn.native_resnets(fuse_stem=True) is emtn and sum(isinstance(m, M.StemFused) for m in emtn.modules()) == 2
    assert sum(isinstance(m, M.BasicBlockFused) for m in emtn.modules()) == 16 and _same(_describe(emtn), before)
    assert emtn.native_resnets() is emtn and not any(isinstance(m, M.StemFused) for m in emtn.modules())
    emtn.native_resnets(fuse_stem=True)
    assert emtn.native_resnets(False) is emtn and not any(isinstance(m, (M.StemFused, M.BasicBlockFused)) for m in emtn.modules())
    assert all(a is b for s, n in zip(stems, nets) for a, b in zip(s, _stem(n)))
    # Gbase and integration.install reach the same function (stubs for the encoders this test does not look at)
    g = gbase.Gbase(appearanceEncoder=nn.Identity(), motionEncoder=emtn, G2d=nn.Identity(), image_pyramid=nn.Identity())
    gkeys = list(g.state_dict().keys())
    assert g.native_motion_encoder(fuse_stem=True) is g and sum(isinstance(m, M.StemFused) for m in emtn.modules()) == 2
    assert list(g.state_dict().keys()) == gkeys
    assert g.native_motion_encoder(False) is g and all(a is b for s, n in zip(stems, nets) for a, b in zip(s, _stem(n)))
    done = integration.install(g, eapp_tail=False)
    assert "Emtn.stems" not in done and "Emtn.resnets" not in done and not any(isinstance(m, M.StemFused) for m in emtn.modules())
    try:
        integration.install(g, eapp_tail=False, fuse_stem=True)      # the keyword belongs to motion_encoder
        assert False
    except ValueError:
        pass
    from megaportrait_hack_amd import reenact
    try:
        reenact.parse(["--random-init", "--source-tensor", "s.pt", "--drivers-tensor", "d.pt", "--native-fuse-stem"])
        assert False
    except SystemExit:
        pass
    cli = reenact.parse(["--random-init", "--source-tensor", "s.pt", "--drivers-tensor", "d.pt", "--native-motion-encoder", "--native-fuse-stem"])
    assert cli.native_motion_encoder and cli.native_fuse_stem
    done = integration.install(g, eapp_tail=False, motion_encoder=True, fuse_stem=True)
    assert "Emtn.resnets" in done and "Emtn.stems" in done and sum(isinstance(m, M.StemFused) for m in emtn.modules()) == 2
    assert list(g.state_dict().keys()) == gkeys
    g.native_motion_encoder(False)
    assert _same(_describe(emtn), before)


def test_conversions_and_modes_reach_the_original_modules():
    net = _seed_bn(E.CifarResNet18(num_classes=6), 2)
    conv, bn, relu, pool = _stem(net)
    assert M.StemFused.swap(net)
    net.eval()
    assert not bn.training and not conv.training
    net.train()
    assert bn.training
    net.double()
    assert bn.running_mean.dtype == torch.float64 and bn.running_mean is net.bn1.running_mean and conv.weight is net.conv1.weight
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    assert M.StemFused.swap(net, False) and net.bn1 is bn and net.conv1 is conv and net.relu is relu and net.maxpool is pool


def test_cpu_fallback_is_the_original_expression():
    torch.manual_seed(5)
    emtn = _seed_bn(E.Emtn(), 3)
    x = torch.rand(2, 3, 24, 20) * 2 - 1
    for train in (False, True):
        emtn.train(train)
        ref = copy.deepcopy(emtn)
        assert M.native_emtn_stems(emtn) is True      # (the stems alone: a fused BasicBlock has no CPU path in eval mode)
        try:
            assert sum(isinstance(m, M.StemFused) for m in emtn.modules()) == 2 and emtn.training == train
            with torch.no_grad():
                # (train mode steps the running statistics: each module is called once per net, on its own copy of the buffers)
                pose, want_pose = emtn.head_pose_net(x), ref.head_pose_net(x)
                expr, want_expr = emtn.expression_net(x), ref.expression_net(x)
                assert torch.equal(pose, want_pose) and torch.equal(expr, want_expr)
                assert torch.equal(emtn.fc(torch.flatten(expr, start_dim=1)), ref.fc(torch.flatten(want_expr, start_dim=1)))
                assert torch.equal(pose[:, 3:], want_pose[:, 3:])
                if not train:
                    _, t, e = emtn(x)
                    _, wt, we = ref(x)
                    assert torch.equal(t, wt) and torch.equal(e, we)
            assert all(torch.equal(a, b) for a, b in zip(emtn.buffers(), ref.buffers()))          # the running statistics moved alike
            assert "_mphip_fold" not in emtn.head_pose_net.conv1.__dict__
        finally:
            M.native_emtn_stems(emtn, False)
    y = emtn.head_pose_net.conv1(x)
    assert not hasattr(y, "_mphip_stem")
