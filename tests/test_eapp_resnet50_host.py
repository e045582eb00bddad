"""Host-side checks of the pointwise 2-D conv and of Eapp's fused ResNet-50 bottlenecks (no GPU): exported symbols (mphip_conv2d_pw_supported,
mphip_conv2d_pw_packed_weight_bytes, mphip_pack_conv2d_pw_weight, mphip_conv2d_pw_workspace_bytes, mphip_conv2d_pw_fwd), ABI version, the
shape rule, argument refusals, the register table, module matching, the BatchNorm fold of the 1x1 convs and the switches."""
import ctypes
import inspect
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, model as M, ops, reenact

ENTRIES = ("mphip_conv2d_pw_supported", "mphip_conv2d_pw_packed_weight_bytes", "mphip_pack_conv2d_pw_weight",
           "mphip_conv2d_pw_workspace_bytes", "mphip_conv2d_pw_fwd")
PW_LDS_BYTES, PW_VGPRS_VEC, PW_VGPRS_B32 = 20576, 130, 146
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 28     # the entries exist since ABI 28
    i, p, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["mphip_conv2d_pw_supported"] == (i, [i] * 6)
    assert _lib.SIGNATURES["mphip_conv2d_pw_packed_weight_bytes"] == (sz, [i] * 2)
    assert _lib.SIGNATURES["mphip_pack_conv2d_pw_weight"] == (i, [p, p, i, i, p])
    assert _lib.SIGNATURES["mphip_conv2d_pw_workspace_bytes"] == (sz, [i] * 6)
    assert _lib.SIGNATURES["mphip_conv2d_pw_fwd"] == (i, [p] * 7 + [i] * 7 + [p, sz, p])
    header = open(os.path.join(ROOT, "include", "mphip.h")).read()
    for name in ENTRIES:
        assert name + "(" in header
    assert list(inspect.signature(ops.conv2d_pw).parameters) == ["x", "pack", "residual", "relu", "stride", "x_range", "want_range"]
    assert ops.PackedConv2dPW is ops.PackedConv2d and callable(ops.conv2d_pw_supported)
    # the packed size: a 16-byte header, then 4096 bytes per (64-channel tile, 16-channel chunk)
    assert lib.mphip_conv2d_pw_packed_weight_bytes(256, 64) == 16 + 4 * 4 * 4096
    assert lib.mphip_conv2d_pw_packed_weight_bytes(96, 32) == 16 + 2 * 2 * 4096
    assert lib.mphip_conv2d_pw_packed_weight_bytes(48, 16) == 0 and lib.mphip_conv2d_pw_packed_weight_bytes(32, 8) == 0


def test_shape_rule():
    lib = _lib.load()
    for bad in [(1, 3, 64, 8, 8, 1), (1, 16, 48, 8, 8, 1), (1, 8, 32, 8, 8, 2), (1, 16, 32, 0, 8, 1), (1, 16, 32, 8, 0, 2), (0, 16, 32, 8, 8, 1),
                (1, 16, 32, 8, 8, 0), (1, 16, 32, 8, 8, 3), (1, 16, 32, 8, 8, -2),      # the stride is 1 or 2
                (1, 16, 32, 1 << 15, 1 << 16, 2),       # H * W = 2^31
                (2, 1024, 32, 1024, 1024, 2),           # x: 2^31 elements, y: 2^24
                (1, 16, 1 << 21, 32, 32, 1),            # x: 2^14 elements, y: 2^21 * 32 * 32 = 2^31
                (1, 16, 1 << 21, 64, 64, 2)]:           # the same y from the halved map
        assert lib.mphip_conv2d_pw_supported(*bad) == 0 and lib.mphip_conv2d_pw_workspace_bytes(*bad) == 0, bad
        assert not ops.conv2d_pw_supported(*bad)
    for ok in [(8, 64, 256, 128, 128, 1), (1, 16, 32, 1, 1, 1), (1, 16, 32, 1, 1, 2), (1, 16, (1 << 21) - 32, 64, 64, 2), (8, 256, 512, 64, 64, 2),
               (3, 48, 96, 13, 19, 1), (3, 48, 96, 13, 19, 2)]:
        assert lib.mphip_conv2d_pw_supported(*ok) == 1 and lib.mphip_conv2d_pw_workspace_bytes(*ok) >= 4100 * 4, ok
    # a y of the stride-1 size would not fit, the halved map does: the rule counts Ho * Wo
    assert lib.mphip_conv2d_pw_supported(1, 16, 1 << 20, 64, 64, 1) == 0 and lib.mphip_conv2d_pw_supported(1, 16, 1 << 20, 64, 64, 2) == 1
    assert ops.conv2d_pw_supported(1, 16, 32, 8, 8) and ops.conv2d_pw_supported(1, 16, 32, 8, 8, 2)


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, r = (ctypes.c_void_p(base + i * 16384) for i in range(3))                 # three disjoint 16 KiB regions: x, y, workspace
    fwd = lambda n, ci, co, h, w, s, x=p, wp=p, b=p, res=None, y=q, ws=r, wsb=1 << 20: lib.mphip_conv2d_pw_fwd(
        x, None, wp, b, res, y, None, n, ci, co, h, w, s, 1, ws, wsb, None)
    for bad in [(1, 8, 32, 8, 8, 1), (1, 16, 48, 8, 8, 2), (1, 16, 32, 0, 8, 1), (1, 16, 32, 8, 8, 0), (1, 16, 32, 8, 8, 3)]:
        assert fwd(*bad) == -1 and b"conv2d_pw_fwd: unsupported shape" in lib.mphip_last_error()
    assert b"stride=3" in lib.mphip_last_error()
    for missing in ("x", "wp", "b", "y"):
        assert fwd(1, 16, 32, 8, 8, 2, **{missing: None}) == -1 and b"conv2d_pw_fwd: null pointer" in lib.mphip_last_error()
    assert fwd(1, 16, 32, 8, 8, 3, b=None) == -1 and b"conv2d_pw_fwd: null pointer" in lib.mphip_last_error()   # null pointer, then shape
    assert fwd(1, 16, 32, 8, 8, 2, wp=ctypes.c_void_p(p.value + 4)) == -1 and b"conv2d_pw_fwd: w_packed" in lib.mphip_last_error()
    assert fwd(1, 8, 32, 8, 8, 2, wp=ctypes.c_void_p(p.value + 4)) == -1 and b"unsupported shape" in lib.mphip_last_error()   # shape, then alignment
    assert fwd(1, 16, 32, 8, 8, 2, wsb=4100 * 4 - 1) == -3 and b"conv2d_pw_fwd: workspace" in lib.mphip_last_error()
    assert fwd(1, 16, 32, 8, 8, 2, ws=None, wsb=0) == -3
    assert fwd(1, 16, 32, 8, 8, 2, b=None, wsb=0) == -1                             # the argument error wins
    for alias in (dict(y=p), dict(y=ctypes.c_void_p(p.value + 64)), dict(res=q)):   # y = x, y inside x, residual = y
        assert fwd(1, 16, 32, 8, 8, 2, **alias) == -1 and b"must not alias" in lib.mphip_last_error(), alias
        assert fwd(1, 16, 32, 8, 8, 2, wsb=0, **alias) == -1                        # aliasing, then the workspace
    # stride 2: y is [1,32,4,4] = 2048 bytes: a residual that begins where y ends does not overlap it; one that begins 4 bytes earlier does
    after = lambda off: ctypes.c_void_p(q.value + off)
    assert fwd(1, 16, 32, 8, 8, 2, res=after(2044), wsb=0) == -1 and b"must not alias" in lib.mphip_last_error()
    assert fwd(1, 16, 32, 8, 8, 2, res=after(2048), wsb=0) == -3                    # passes the overlap rule, stops at the workspace
    assert fwd(1, 16, 32, 8, 8, 2, x=after(2048), wsb=0) == -3
    # stride 1: y is [1,32,8,8] = 8192 bytes: the extents follow Ho * Wo
    assert fwd(1, 16, 32, 8, 8, 1, res=after(2048), wsb=0) == -1 and b"must not alias" in lib.mphip_last_error()
    assert fwd(1, 16, 32, 8, 8, 1, res=after(8188), wsb=0) == -1 and fwd(1, 16, 32, 8, 8, 1, res=after(8192), wsb=0) == -3
    # the pack entry refuses on the host as well
    assert lib.mphip_pack_conv2d_pw_weight(None, p, 32, 16, None) == -1 and b"pack_conv2d_pw_weight: null" in lib.mphip_last_error()
    assert lib.mphip_pack_conv2d_pw_weight(p, q, 48, 16, None) == -1 and lib.mphip_pack_conv2d_pw_weight(p, after(4), 32, 16, None) == -1


def test_kernels_are_in_the_register_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import register_table

    kernels = register_table.collect(["conv2d_pw_f16x3.hip"])["conv2d_pw_f16x3.hip"]["kernels"]
    by_name = {k["demangled"]: k for k in kernels}
    assert sorted(by_name) == ["conv2d_pw_absmax_kernel", "conv2d_pw_f16x3_kernel<0>", "conv2d_pw_f16x3_kernel<1>", "conv2d_pw_pack_kernel"]
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    vec, b32 = by_name["conv2d_pw_f16x3_kernel<1>"], by_name["conv2d_pw_f16x3_kernel<0>"]
    assert vec["group_segment_fixed_size"] == b32["group_segment_fixed_size"] == PW_LDS_BYTES <= 160 * 1024 // 3   # three workgroups per CU
    assert vec["vgpr_count"] == PW_VGPRS_VEC and b32["vgpr_count"] == PW_VGPRS_B32 <= 168                            # three waves per SIMD
    assert vec.get("agpr_count", 0) == 0 and b32.get("agpr_count", 0) == 0
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 3.15"):]
    assert f"{PW_LDS_BYTES} B" in sec and f"{PW_VGPRS_VEC} VGPRs" in sec and f"{PW_VGPRS_B32} VGPRs" in sec


def _seed_bn(block, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in block.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g))
                m.weight.copy_(torch.randn(m.num_features, generator=g))
                m.bias.copy_(torch.randn(m.num_features, generator=g))
    return block


class _TorchvisionBottleneck(nn.Module):
    """torchvision's Bottleneck (v1.5: the stride on the 3x3) as its resnet.py writes it; v1=True puts the stride on conv1."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, dilation=1, v1=False):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=stride if v1 else 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1 if v1 else stride, padding=dilation, groups=groups, bias=False,
                               dilation=dilation)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


def _ds(ci, co, stride, **kw):
    return nn.Sequential(nn.Conv2d(ci, co, 1, stride=stride, bias=False, **kw), nn.BatchNorm2d(co))


def test_matches_accepts_and_rejects_the_right_modules():
    ok = M.BottleneckFused.matches
    assert ok(E._Bottleneck(64, 64, 1)) and ok(E._Bottleneck(256, 64, 1)) and ok(E._Bottleneck(256, 128, 2)) and ok(E._Bottleneck(32, 32, 2))
    assert E._Bottleneck(256, 64, 1).downsample is None and isinstance(E._Bottleneck(64, 64, 1).downsample, nn.Sequential)
    assert ok(_TorchvisionBottleneck(256, 64)) and ok(_TorchvisionBottleneck(256, 128, 2, _ds(256, 512, 2)))
    assert ok(_TorchvisionBottleneck(64, 64, 1, _ds(64, 256, 1)))
    assert all(ok(b) for name in ("layer1", "layer2", "layer3") for b in getattr(E.CustomResNet50(), name))
    with_bias = E._Bottleneck(32, 32, 2)
    with_bias.conv1 = nn.Conv2d(32, 32, 1, bias=True)
    assert ok(with_bias)                                               # a bias may be present
    assert not ok(E._BasicBlock(64, 64, 1)) and not ok(E.ResBlock2D(32, 32)) and not ok(nn.Conv2d(3, 3, 3)) and not ok(nn.Sequential())
    assert not M.BasicBlockFused.matches(E._Bottleneck(64, 64, 1)) and not M.ResBlock2DFused.matches(E._Bottleneck(64, 64, 1))
    assert not ok(M.BottleneckFused(32, 32, 2)) and not ok(M.BottleneckFused.from_block(E._Bottleneck(32, 32)))     # already fused
    assert not ok(_TorchvisionBottleneck(256, 128, 2, _ds(256, 512, 2), v1=True))      # the v1 layout: the stride on conv1
    assert not ok(_TorchvisionBottleneck(256, 128, 2, _ds(256, 512, 1)))               # the downsample conv at another stride than conv2
    assert not ok(_TorchvisionBottleneck(256, 128, 1, _ds(256, 512, 2)))
    assert not ok(_TorchvisionBottleneck(256, 128, 2))                                 # stride 2 without a downsample
    assert not ok(_TorchvisionBottleneck(64, 64, 1))                                   # 64 -> 256 channels without one
    assert not ok(_TorchvisionBottleneck(256, 64, groups=2)) and not ok(_TorchvisionBottleneck(256, 64, dilation=2))

    def broken(edit):
        b = E._Bottleneck(32, 32, 2)
        edit(b)
        return b

    assert not ok(broken(lambda b: setattr(b, "conv1", nn.Conv2d(32, 32, 3, padding=1, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv3", nn.Conv2d(32, 128, 1, stride=2, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv3", nn.Conv2d(32, 128, 1, groups=2, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv2", nn.Conv2d(32, 32, 3, stride=(2, 1), padding=1, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv2", nn.Conv2d(32, 32, 3, stride=2, padding=1, padding_mode="reflect"))))
    assert not ok(broken(lambda b: setattr(b, "conv2", nn.Conv2d(32, 32, 5, stride=2, padding=2, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv2", nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "bn1", nn.BatchNorm2d(32, track_running_stats=False))))
    assert not ok(broken(lambda b: setattr(b, "bn3", nn.GroupNorm(32, 128))))
    assert not ok(broken(lambda b: setattr(b, "downsample", nn.Sequential(nn.Conv2d(32, 128, 1, stride=2)))))
    assert not ok(broken(lambda b: setattr(b, "downsample", _ds(32, 128, 2, groups=2))))
    assert not ok(broken(lambda b: setattr(b, "downsample", _ds(32, 64, 2))))
    assert not ok(broken(lambda b: setattr(b, "shortcut", nn.Identity())))       # a ResBlock2D's attribute
    for bad in (lambda: M.BottleneckFused.from_block(E._BasicBlock(32, 32)), lambda: M.BottleneckFused.from_block(E._Bottleneck(32, 32), True)):
        try:
            bad()
            assert False
        except TypeError:
            pass


def test_batchnorm_fold_of_the_pointwise_convs_against_fp64():
    x = torch.randn(2, 16, 9, 11, dtype=torch.float64)
    for stride in (1, 2):
        conv, bn = nn.Conv2d(16, 32, 1, stride=stride, bias=False).double(), nn.BatchNorm2d(32).double()
        _seed_bn(bn, 3)
        bn.eval()
        w, b = M.fold_batchnorm(conv, bn)
        assert w.dtype == b.dtype == torch.float64 and not w.requires_grad and w.shape == (32, 16, 1, 1) and b.shape == (32,)
        want = bn(conv(x))
        assert (F.conv2d(x, w, b, stride=stride) - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    # a whole block: the four folded convs in fp64 reproduce the block
    blk = _seed_bn(E._Bottleneck(16, 16, 2), 7).double().eval()
    with torch.no_grad():
        (w1, b1), (w2, b2), (w3, b3), (wd, bd) = (M.fold_batchnorm(c, n) for c, n in M.BottleneckFused.from_block(blk)._fold_pairs())
        y = F.relu(F.conv2d(F.relu(F.conv2d(x, w1, b1)), w2, b2, stride=2, padding=1))
        y = F.relu(F.conv2d(y, w3, b3) + F.conv2d(x, wd, bd, stride=2))
        want = blk(x)
    assert (y - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_fused_block_shares_the_block_and_its_reference_is_the_original_forward():
    for ci, planes, stride in [(64, 16, 1), (16, 16, 2), (16, 16, 1)]:
        blk = _seed_bn(E._Bottleneck(ci, planes, stride), ci + stride).eval()
        fused = M.BottleneckFused.from_block(blk)
        assert list(fused.state_dict().keys()) == list(blk.state_dict().keys())
        assert [n for n, _ in fused.named_children()] == [n for n, _ in blk.named_children()]
        assert all(a is b for a, b in zip(fused.parameters(), blk.parameters())) and all(a is b for a, b in zip(fused.buffers(), blk.buffers()))
        assert list(M.BottleneckFused(ci, planes, stride).state_dict().keys()) == list(blk.state_dict().keys())
        assert not fused.training and "_mphip_half" not in fused.__dict__
        x = torch.randn(2, ci, 5, 7)
        with torch.no_grad():
            assert torch.equal(fused._reference(x), blk(x))
        assert torch.equal(fused(x), blk(x)) and fused(x).requires_grad      # parameters require grad: the original PyTorch expression
        assert "_mphip_fold" not in fused.__dict__
    assert M.BottleneckFused.from_block(E._Bottleneck(16, 16).train()).training


def _blocks(eapp):
    return [b for name in ("layer1", "layer2", "layer3") for b in getattr(eapp.custom_resnet50, name)]


def test_switches_are_off_by_default_and_leave_the_keys_alone():
    eapp = E.Eapp()
    blocks = _blocks(eapp)
    assert len(blocks) == 13 and all(type(b) is E._Bottleneck for b in blocks)
    keys, modules, params = list(eapp.state_dict().keys()), [n for n, _ in eapp.named_modules()], list(eapp.parameters())
    assert M.native_eapp_resnet50(eapp) is True and M.native_eapp_resnet50(eapp) is False      # twice: nothing left to swap
    assert all(isinstance(b, M.BottleneckFused) for b in _blocks(eapp)) and sum(isinstance(m, M.BottleneckFused) for m in eapp.modules()) == 13
    net = eapp.custom_resnet50
    assert isinstance(net.conv1, nn.Conv2d) and isinstance(net.maxpool, nn.MaxPool2d) and isinstance(net.conv_reduce, nn.Conv2d)   # these stay
    assert type(eapp.resblock_128) is E.ResBlock_Custom                                                     # another switch's blocks
    assert list(eapp.state_dict().keys()) == keys and [n for n, _ in eapp.named_modules()] == modules
    assert all(a is b for a, b in zip(eapp.parameters(), params))
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():       # on the CPU a fused block is the original forward
        es = eapp.eval().descriptor(x)
    assert M.native_eapp_resnet50(eapp, False) is True and M.native_eapp_resnet50(eapp, False) is False
    assert all(a is b for a, b in zip(blocks, _blocks(eapp))) and list(eapp.state_dict().keys()) == keys
    with torch.no_grad():
        assert torch.equal(eapp.descriptor(x), es)
    assert eapp.native_resnet50() is eapp and all(isinstance(b, M.BottleneckFused) for b in _blocks(eapp))
    assert eapp.native_resnet50(False) is eapp and all(a is b for a, b in zip(blocks, _blocks(eapp)))
    # Gbase reaches the same function (stubs for the modules this test does not look at)
    g = gbase.Gbase(appearanceEncoder=eapp, motionEncoder=nn.Identity(), G2d=nn.Identity(), image_pyramid=nn.Identity())
    gkeys = list(g.state_dict().keys())
    assert g.native_resnet50() is g and all(isinstance(b, M.BottleneckFused) for b in _blocks(eapp))
    assert list(g.state_dict().keys()) == gkeys
    assert g.native_resnet50(False) is g and all(a is b for a, b in zip(blocks, _blocks(eapp)))
    assert M.native_eapp_resnet50(nn.Identity()) is False      # nothing to swap: not an error


def test_cli_flag_parses():
    assert reenact.parse(["--random-init", "--source", "s", "--drivers", "d"]).native_eapp_resnet50 is False
    assert reenact.parse(["--random-init", "--source", "s", "--drivers", "d", "--native-eapp-resnet50"]).native_eapp_resnet50 is True
