"""Host-side checks of the grouped 2-D 3x3 conv and of the 6DRepNet switch (no GPU): exported symbols (mphip_conv2d_grouped_supported,
_workspace_bytes, _fwd), ABI version, the shape rule, argument refusals and their order, the register table, module matching
(model.RepVGGBlockFused), the swap (model.native_rotation_net), the CPU fall-back and the switches."""
import copy
import ctypes
import os
import sys

import pytest
import torch
import torch.nn as nn

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, integration, model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mphip_conv2d_grouped_supported", "mphip_conv2d_grouped_workspace_bytes", "mphip_conv2d_grouped_fwd")
GRP_VGPRS, GRP_SGPRS, GRP_LDS_BYTES = 210, 58, 57696      # conv2d_k3_grp_f16x3_kernel, DESIGN.md section 3.13

GOOD = [(1, 32, 128, 1, 1, 2), (8, 512, 512, 32, 32, 2), (1, 96, 192, 5, 5, 3), (1, 64, 64, 8, 8, 1)]
BAD = [(1, 32, 64, 8, 8, 2),        # Cog = 32
       (1, 16, 128, 8, 8, 2),       # Cig = 8
       (1, 48, 128, 8, 8, 2),       # Cig = 24
       (1, 32, 128, 8, 8, 0), (1, 32, 128, 8, 8, -1),
       (1, 32, 128, 8, 8, 3),       # neither channel count is a multiple of 3
       (1, 128, 128, 8, 8, 4),      # Cog = 32
       (0, 32, 128, 8, 8, 2), (1, 0, 128, 8, 8, 2), (1, 32, 0, 8, 8, 2), (1, 32, 128, 0, 8, 2), (1, 32, 128, 8, 0, 2),
       (1, 32, 128, 1 << 15, 1 << 16, 2),      # a map of 2^31 elements
       (1, 8, 64, 8, 8, 1), (1, 16, 48, 8, 8, 1)]      # one group: the plain rule


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 25
    header = open(os.path.join(ROOT, "include", "mphip.h")).read()
    assert all(name + "(" in header for name in ENTRIES)


def test_shape_rule():
    from megaportrait_hack_amd import ops

    lib = _lib.load()
    for good in GOOD:
        assert lib.mphip_conv2d_grouped_supported(*good) == 1 and lib.mphip_conv2d_grouped_workspace_bytes(*good) > 0, good
        assert ops.conv2d_grouped_supported(*good)
    for bad in BAD:
        assert lib.mphip_conv2d_grouped_supported(*bad) == 0 and lib.mphip_conv2d_grouped_workspace_bytes(*bad) == 0, bad
        assert not ops.conv2d_grouped_supported(*bad)
    for shape in [(1, 64, 64, 8, 8), (1, 8, 64, 8, 8), (2, 16, 32, 1, 1), (1, 16, 48, 8, 8)]:      # one group: the plain entry's verdict
        assert lib.mphip_conv2d_grouped_supported(*shape, 1) == lib.mphip_conv2d_supported(*shape)
        assert lib.mphip_conv2d_grouped_workspace_bytes(*shape, 1) == lib.mphip_conv2d_workspace_bytes(*shape)


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 18)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q = (ctypes.c_void_p(base + i * (1 << 16)) for i in range(2))      # two disjoint 64 KiB regions: x (and pack, bias), y
    at = lambda b, off: ctypes.c_void_p(b.value + off)

    def fwd(n, ci, co, h, w, g, x=p, wp=p, b=p, res=None, y=q, ws=p, wsb=1 << 16):
        return lib.mphip_conv2d_grouped_fwd(x, None, wp, b, res, y, None, n, ci, co, h, w, g, 1, ws, wsb, None)

    for bad in BAD:
        assert fwd(*bad) == -1 and b"conv2d_grouped_fwd: unsupported shape" in lib.mphip_last_error(), (bad, lib.mphip_last_error())
    ok = (1, 32, 128, 4, 4, 2)      # x: 512 floats = 2 KiB, y: 2048 floats = 8 KiB
    for g in (2, 1):                # one group reports under the called entry's name too
        for missing in ("x", "wp", "b", "y"):
            assert fwd(*ok[:5], g, **{missing: None}) == -1 and b"conv2d_grouped_fwd: null pointer" in lib.mphip_last_error()
    # the shared order: null pointer, shape, alignment, aliasing, workspace
    assert fwd(1, 32, 64, 4, 4, 2, x=None) == -1 and b"conv2d_grouped_fwd: null pointer" in lib.mphip_last_error()
    assert fwd(1, 32, 64, 4, 4, 2, x=at(p, 2), y=p) == -1 and b"conv2d_grouped_fwd: unsupported shape" in lib.mphip_last_error()
    assert fwd(*ok, x=at(p, 2), y=p) == -1 and b"aligned" in lib.mphip_last_error()
    assert fwd(*ok, wp=at(p, 4), y=p) == -1 and b"16-byte aligned" in lib.mphip_last_error()
    for alias in (dict(y=p), dict(y=at(p, 2044)), dict(x=at(q, 8188)), dict(res=at(q, 8188)), dict(res=q)):
        assert fwd(*ok, wsb=0, **alias) == -1 and b"must not alias" in lib.mphip_last_error(), alias
    assert fwd(*ok, wsb=16) == -3 and b"conv2d_grouped_fwd: workspace" in lib.mphip_last_error()
    assert fwd(*ok, ws=None, wsb=0) == -3
    assert fwd(*ok, b=None, wsb=16) == -1      # the argument error wins


def test_kernel_is_in_the_register_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import register_table

    table = register_table.collect(["conv2d_grp_f16x3.hip", "conv2d_f16x3.hip"])
    grp = table["conv2d_grp_f16x3.hip"]["kernels"]
    assert [k["demangled"].split("(")[0] for k in grp] == ["conv2d_k3_grp_f16x3_kernel"], grp
    k = grp[0]
    plain = [p for p in table["conv2d_f16x3.hip"]["kernels"] if p["demangled"].startswith("conv2d_k3_f16x3_kernel")]
    assert len(plain) == 1
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= 256 and k["max_flat_workgroup_size"] == 256      # two waves per SIMD of 512 registers
    assert k["group_segment_fixed_size"] == plain[0]["group_segment_fixed_size"] == GRP_LDS_BYTES
    assert 2 * k["group_segment_fixed_size"] <= 160 * 1024                    # two workgroups per CU
    assert (k["vgpr_count"], k.get("agpr_count", 0), k["sgpr_count"]) == (GRP_VGPRS, 0, GRP_SGPRS)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 3.13"):]
    assert f"{GRP_VGPRS} VGPRs" in sec and f"{GRP_SGPRS} SGPRs" in sec and f"{GRP_LDS_BYTES} B" in sec


class _ReferenceStyleBlock(nn.Module):
    """The attribute set of the reference's RepVGGBlock(deploy=True): `nonlinearity`, `se`, `rbr_reparam`, registered in that order."""

    def __init__(self, conv=None, se=None, act=None):
        super().__init__()
        self.deploy, self.groups, self.in_channels = True, 1, 64
        self.nonlinearity = act if act is not None else nn.ReLU()
        self.se = se if se is not None else nn.Identity()
        self.rbr_reparam = conv if conv is not None else nn.Conv2d(64, 128, 3, stride=1, padding=1, groups=2, bias=True)

    def forward(self, inputs):
        return self.nonlinearity(self.se(self.rbr_reparam(inputs)))


class _TrainingStyleBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.nonlinearity, self.se = nn.ReLU(), nn.Identity()
        self.rbr_dense = nn.Sequential(nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64))
        self.rbr_1x1 = nn.Sequential(nn.Conv2d(64, 64, 1, bias=False), nn.BatchNorm2d(64))


def test_matches_accepts_and_rejects_the_right_blocks():
    ok = M.RepVGGBlockFused.matches
    assert ok(E._RepVGGDeployBlock(64, 128, 1, 1)) and ok(E._RepVGGDeployBlock(64, 128, 2, 1)) and ok(E._RepVGGDeployBlock(128, 128, 1, 2))
    assert ok(_ReferenceStyleBlock()) and ok(_ReferenceStyleBlock(act=nn.ReLU(inplace=True)))
    assert ok(E._RepVGGDeployBlock(128, 128, 1, 4))                                    # matched; the shape rule sends it to PyTorch
    assert not ok(_TrainingStyleBlock())
    assert not ok(_ReferenceStyleBlock(act=nn.LeakyReLU(0.1))) and not ok(_ReferenceStyleBlock(act=nn.Identity()))
    assert not ok(_ReferenceStyleBlock(se=nn.Sequential())) and not ok(_ReferenceStyleBlock(se=nn.Sigmoid()))
    conv = lambda **kw: _ReferenceStyleBlock(conv=nn.Conv2d(64, 128, **{"kernel_size": 3, "padding": 1, **kw}))
    assert ok(conv()) and ok(conv(stride=2))
    assert not ok(conv(bias=False)) and not ok(conv(padding=0)) and not ok(conv(padding=2, dilation=2)) and not ok(conv(stride=2, groups=2))
    assert not ok(conv(kernel_size=1, padding=0)) and not ok(conv(stride=3)) and not ok(conv(padding_mode="reflect"))
    assert not ok(E._RepVGGDeployBlock(3, 64, 2, 1))                                   # layer0: Ci = 3 fits no kernel
    assert not ok(nn.Conv2d(64, 64, 3, padding=1)) and not ok(None)
    fused = M.RepVGGBlockFused.from_block(E._RepVGGDeployBlock(64, 128, 1, 1))
    assert not ok(fused) and isinstance(fused, M._FusedBlock2D) and fused._EVAL_ONLY
    with pytest.raises(TypeError):
        M.RepVGGBlockFused.from_block(_TrainingStyleBlock())
    with pytest.raises(TypeError):
        M.RepVGGBlockFused.from_block(E._RepVGGDeployBlock(64, 128, 1, 1), half_precision=True)
    ref = _ReferenceStyleBlock()
    f = M.RepVGGBlockFused.from_block(ref)
    assert [n for n, _ in f.named_modules()] == [n for n, _ in ref.named_modules()] and f.rbr_reparam is ref.rbr_reparam
    assert f.nonlinearity is ref.nonlinearity and f.se is ref.se and list(f.state_dict()) == list(ref.state_dict())


def _describe(m):
    return (list(m.state_dict().keys()), [n for n, _ in m.named_modules()], [n for n, _ in m.named_parameters()], list(m.parameters()))


def _same(a, b):
    return a[:3] == b[:3] and len(a[3]) == len(b[3]) and all(x is y for x, y in zip(a[3], b[3]))


def _slots(net):
    return [net.layer0] + [b for s in (net.layer1, net.layer2, net.layer3, net.layer4) for b in s]


@pytest.mark.parametrize("kind", ["emtn", "detector", "backbone"])
def test_native_rotation_net_swaps_27_blocks_and_puts_them_back(kind):
    net = E.SixDRepNetBackbone()
    target = {"emtn": lambda: E.Emtn(rotation_net=E.SixDRepNet_Detector(net)), "detector": lambda: E.SixDRepNet_Detector(net),
              "backbone": lambda: net}[kind]()
    before, originals = _describe(net), _slots(net)
    outer = _describe(target) if isinstance(target, nn.Module) else None
    assert len(originals) == 28 and sum(b.rbr_reparam.groups == 2 for b in originals) == 13
    assert M.native_rotation_net(target, False) is False
    assert M.native_rotation_net(target) is True and M.native_rotation_net(target) is False       # a second time: nothing left to swap
    now = _slots(net)
    assert now[0] is originals[0] and type(now[0]) is E._RepVGGDeployBlock                          # layer0 stays
    assert all(isinstance(b, M.RepVGGBlockFused) for b in now[1:]) and sum(isinstance(m, M.RepVGGBlockFused) for m in net.modules()) == 27
    assert all(b.rbr_reparam is o.rbr_reparam for b, o in zip(now, originals))
    assert _same(_describe(net), before) and (outer is None or _same(_describe(target), outer))
    assert copy.deepcopy(net).state_dict().keys() == net.state_dict().keys()
    assert M.native_rotation_net(target, False) is True and M.native_rotation_net(target, False) is False
    assert all(a is b for a, b in zip(_slots(net), originals)) and _same(_describe(net), before)


def test_cpu_fallback_is_the_original_expression():
    torch.manual_seed(7)
    net = E.SixDRepNetBackbone().eval()
    x = torch.rand(2, 3, 40, 36) * 2 - 1
    with torch.no_grad():
        want_rot, want_rest = net(x)
        det = E.SixDRepNet_Detector(net)
        want_deg, _ = det.predict(x)
        assert M.native_rotation_net(net) is True
        try:
            rot, rest = net(x)
            deg, _ = det.predict(x)
            assert torch.equal(rot, want_rot) and torch.equal(rest, want_rest) and torch.equal(deg, want_deg)
            assert not any("_mphip_fold" in m.__dict__ for m in net.modules())
        finally:
            M.native_rotation_net(net, False)
    ref = _ReferenceStyleBlock().eval()
    xb = torch.randn(1, 64, 6, 5)
    with torch.no_grad():
        assert torch.equal(M.RepVGGBlockFused.from_block(ref)(xb), ref(xb))


def test_switches_are_off_by_default():
    emtn = E.Emtn()
    net = emtn.rotation_net.model
    count = lambda: sum(isinstance(m, M.RepVGGBlockFused) for m in net.modules())
    originals = _slots(net)
    assert emtn.native_resnets(fuse_stem=True) is emtn and count() == 0                 # the ResNet switch leaves the third net alone
    assert emtn.native_rotation_net() is emtn and count() == 27
    assert sum(isinstance(m, M.BasicBlockFused) for m in emtn.modules()) == 16          # and the other way round
    assert emtn.native_resnets(False) is emtn and count() == 27
    assert emtn.native_rotation_net(False) is emtn and count() == 0 and all(a is b for a, b in zip(_slots(net), originals))
    g = gbase.Gbase(appearanceEncoder=nn.Identity(), motionEncoder=emtn, G2d=nn.Identity(), image_pyramid=nn.Identity())
    gkeys = list(g.state_dict().keys())
    assert g.native_motion_encoder() is g and count() == 0
    assert g.native_motion_encoder(rotation_net=True) is g and count() == 27 and list(g.state_dict().keys()) == gkeys
    assert g.native_motion_encoder() is g and count() == 0                              # without the keyword the blocks are back
    g.native_motion_encoder(rotation_net=True)
    assert g.native_motion_encoder(False) is g and count() == 0 and all(a is b for a, b in zip(_slots(net), originals))
    done = integration.install(g, eapp_tail=False, motion_encoder=True)
    assert "Emtn.rotation_net" not in done and count() == 0
    g.native_motion_encoder(False)
    with pytest.raises(ValueError):
        integration.install(g, eapp_tail=False, rotation_net=True)                     # the keyword belongs to motion_encoder
    assert count() == 0
    done = integration.install(g, eapp_tail=False, motion_encoder=True, rotation_net=True)
    assert "Emtn.resnets" in done and "Emtn.rotation_net" in done and "Emtn.stems" not in done and count() == 27
    g.native_motion_encoder(False)
    assert count() == 0
    from megaportrait_hack_amd import reenact

    base = ["--random-init", "--source-tensor", "s.pt", "--drivers-tensor", "d.pt"]
    assert not reenact.parse(base).native_rotation_net
    with pytest.raises(SystemExit):
        reenact.parse(base + ["--native-rotation-net"])
    cli = reenact.parse(base + ["--native-motion-encoder", "--native-rotation-net"])
    assert cli.native_motion_encoder and cli.native_rotation_net and not cli.native_fuse_stem
