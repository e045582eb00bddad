"""Host-side checks of the stride-2 2-D conv and of Emtn's fused ResNet-18 blocks (no GPU): exported symbols (mphip_conv2d_s2_supported,
mphip_conv2d_s2_workspace_bytes, mphip_conv2d_s2_fwd), ABI version, the shape rule, argument refusals, the register table, module
matching, the BatchNorm fold of a bias-less conv and the switches."""
import ctypes
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, model as M

ENTRIES = ("mphip_conv2d_s2_supported", "mphip_conv2d_s2_workspace_bytes", "mphip_conv2d_s2_fwd")
S2_LDS_BYTES, S2_VGPRS = 76128, 172


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 22     # the entries exist since ABI 22


def test_shape_rule():
    lib = _lib.load()
    for bad in [(1, 3, 64, 8, 8), (1, 16, 48, 8, 8), (1, 16, 32, 0, 8), (1, 16, 32, 8, 0), (0, 16, 32, 8, 8), (1, 8, 32, 8, 8),
                (1, 16, 32, 1 << 15, 1 << 16),          # H * W = 2^31
                (2, 1024, 32, 1024, 1024),              # x: 2^31 elements, y: 2^24
                (1, 16, 1 << 21, 64, 64)]:              # x: 2^16 elements, y: 2^21 * 32 * 32 = 2^31
        assert lib.mphip_conv2d_s2_supported(*bad) == 0 and lib.mphip_conv2d_s2_workspace_bytes(*bad) == 0, bad
    for ok in [(8, 64, 128, 256, 256), (1, 16, 32, 1, 1), (1, 16, (1 << 21) - 32, 64, 64), (8, 256, 512, 64, 64), (3, 48, 96, 13, 19)]:
        assert lib.mphip_conv2d_s2_supported(*ok) == 1 and lib.mphip_conv2d_s2_workspace_bytes(*ok) >= 4100 * 4, ok
    # a y of the stride-1 size would not fit, the halved map does: the rule counts Ho * Wo
    assert lib.mphip_conv2d_supported(1, 16, 1 << 20, 64, 64) == 0 and lib.mphip_conv2d_s2_supported(1, 16, 1 << 20, 64, 64) == 1


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, r = (ctypes.c_void_p(base + i * 16384) for i in range(3))                 # three disjoint 16 KiB regions: x, y, workspace
    fwd = lambda n, ci, co, h, w, x=p, wp=p, b=p, res=None, y=q, ws=r, wsb=1 << 20: lib.mphip_conv2d_s2_fwd(
        x, None, wp, b, res, y, None, n, ci, co, h, w, 1, ws, wsb, None)
    for bad in [(1, 8, 32, 8, 8), (1, 16, 48, 8, 8), (1, 16, 32, 0, 8)]:
        assert fwd(*bad) == -1 and b"conv2d_s2_fwd: unsupported shape" in lib.mphip_last_error()
    for missing in ("x", "wp", "b", "y"):
        assert fwd(1, 16, 32, 8, 8, **{missing: None}) == -1 and b"conv2d_s2_fwd: null pointer" in lib.mphip_last_error()
    assert fwd(1, 16, 32, 8, 8, wsb=4100 * 4 - 1) == -3 and b"conv2d_s2_fwd: workspace" in lib.mphip_last_error()
    assert fwd(1, 16, 32, 8, 8, ws=None, wsb=0) == -3
    assert fwd(1, 16, 32, 8, 8, b=None, wsb=0) == -1                                # the argument error wins
    for alias in (dict(y=p), dict(y=ctypes.c_void_p(p.value + 64)), dict(res=q)):   # y = x, y inside x, residual = y
        assert fwd(1, 16, 32, 8, 8, **alias) == -1 and b"must not alias" in lib.mphip_last_error(), alias
    # y is [1,32,4,4] = 2048 bytes: a residual that begins where y ends does not overlap it; one that begins 4 bytes earlier does
    after = lambda off: ctypes.c_void_p(q.value + off)
    assert fwd(1, 16, 32, 8, 8, res=after(2044), wsb=0) == -1 and b"must not alias" in lib.mphip_last_error()
    assert fwd(1, 16, 32, 8, 8, res=after(2048), wsb=0) == -3                       # passes the overlap rule, stops at the workspace
    assert fwd(1, 16, 32, 8, 8, x=after(2048), wsb=0) == -3


def test_kernel_is_in_the_register_table_without_scratch():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import register_table

    kernels = register_table.collect(["conv2d_s2_f16x3.hip"])["conv2d_s2_f16x3.hip"]["kernels"]
    assert [k["demangled"].split("<")[0].split("(")[0] for k in kernels] == ["conv2d_k3s2_f16x3_kernel"]
    k = kernels[0]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["group_segment_fixed_size"] == S2_LDS_BYTES <= 80 * 1024          # two workgroups per CU (160 KiB of LDS)
    assert k["vgpr_count"] == S2_VGPRS <= 256 and k.get("agpr_count", 0) == 0   # two waves per SIMD
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    sec = design[design.index("### 3.11"):]
    assert f"{S2_LDS_BYTES} B" in sec and f"{S2_VGPRS} VGPRs" in sec


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


class _TorchvisionBlock(nn.Module):
    """torchvision's BasicBlock as the reference's resnet.py writes it: a `stride` attribute, bias-less convs."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, groups=1, bias=False, dilation=1)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, groups=1, bias=False, dilation=1)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride


def _ds(ci, co, stride, **kw):
    return nn.Sequential(nn.Conv2d(ci, co, 1, stride=stride, bias=False, **kw), nn.BatchNorm2d(co))


def test_matches_accepts_and_rejects_the_right_modules():
    ok = M.BasicBlockFused.matches
    assert ok(E._BasicBlock(64, 64, 1)) and ok(E._BasicBlock(64, 128, 2)) and ok(E._BasicBlock(32, 64, 1))
    assert E._BasicBlock(64, 64, 1).downsample is None and isinstance(E._BasicBlock(64, 128, 2).downsample, nn.Sequential)
    assert ok(_TorchvisionBlock(64, 64)) and ok(_TorchvisionBlock(64, 128, 2, _ds(64, 128, 2)))
    with_bias = E._BasicBlock(32, 64, 2)
    with_bias.conv1 = nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=True)
    assert ok(with_bias)                                               # a bias may be present
    assert not ok(E.ResBlock2D(32, 32)) and not ok(E.ResBlock2D(32, 64)) and not ok(nn.Conv2d(3, 3, 3)) and not ok(nn.Sequential())
    assert not ok(M.BasicBlockFused(32, 64, 2)) and not ok(M.BasicBlockFused.from_block(E._BasicBlock(32, 32)))     # already fused
    assert not ok(_TorchvisionBlock(64, 128, 2, _ds(64, 128, 1)))      # the downsample conv at another stride than conv1
    assert not ok(_TorchvisionBlock(64, 128, 1, _ds(64, 128, 2)))
    assert not ok(_TorchvisionBlock(64, 128, 2))                       # stride 2 without a downsample
    assert not ok(_TorchvisionBlock(64, 128, 1))                       # 64 -> 128 channels without one

    def broken(edit):
        b = E._BasicBlock(32, 64, 2)
        edit(b)
        return b

    assert not ok(broken(lambda b: setattr(b, "conv1", nn.Conv2d(32, 64, 3, stride=2, padding=1, groups=2, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv2", nn.Conv2d(64, 64, 3, padding=1, groups=2, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv2", nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv1", nn.Conv2d(32, 64, 3, stride=(2, 1), padding=1, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv1", nn.Conv2d(32, 64, 3, stride=2, padding=1, dilation=1, padding_mode="reflect"))))
    assert not ok(broken(lambda b: setattr(b, "conv1", nn.Conv2d(32, 64, 5, stride=2, padding=2, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "bn1", nn.BatchNorm2d(64, track_running_stats=False))))
    assert not ok(broken(lambda b: setattr(b, "bn2", nn.GroupNorm(32, 64))))
    assert not ok(broken(lambda b: setattr(b, "downsample", nn.Sequential(nn.Conv2d(32, 64, 1, stride=2)))))
    assert not ok(broken(lambda b: setattr(b, "downsample", _ds(32, 64, 2, groups=2))))
    assert not ok(broken(lambda b: setattr(b, "shortcut", nn.Identity())))       # a ResBlock2D's attribute
    # the two fused classes keep apart
    assert not M.ResBlock2DFused.matches(E._BasicBlock(64, 64, 1)) and not M.ResBlock2DFused.matches(E._BasicBlock(64, 128, 2))
    for bad in (lambda: M.BasicBlockFused.from_block(E.ResBlock2D(32, 32)), lambda: M.BasicBlockFused.from_block(E._BasicBlock(32, 32), True)):
        try:
            bad()
            assert False
        except TypeError:
            pass


def test_batchnorm_fold_of_a_biasless_conv_and_the_unchanged_fold_with_bias():
    x = torch.randn(2, 16, 9, 11, dtype=torch.float64)
    for stride in (1, 2):
        conv, bn = nn.Conv2d(16, 32, 3, stride=stride, padding=1, bias=False).double(), nn.BatchNorm2d(32).double()
        _seed_bn(bn, 3)
        bn.eval()
        w, b = M.fold_batchnorm(conv, bn)
        assert w.dtype == b.dtype == torch.float64 and not w.requires_grad and b.shape == (32,)
        want = bn(conv(x))
        assert (F.conv2d(x, w, b, stride=stride, padding=1) - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    # with a bias: the bits of the expression as it has always been written
    for dtype in (None, torch.float32):
        conv, bn = nn.Conv2d(16, 32, 3, padding=1), _seed_bn(nn.BatchNorm2d(32), 5)
        if dtype is not None:
            conv, bn = conv.half(), bn.half()
        cast = (lambda t: t.detach()) if dtype is None else (lambda t: t.detach().to(dtype))
        s = cast(bn.weight) / torch.sqrt(cast(bn.running_var) + bn.eps)
        want_w = (cast(conv.weight) * s[:, None, None, None]).contiguous()
        want_b = ((cast(conv.bias) - cast(bn.running_mean)) * s + cast(bn.bias)).contiguous()
        w, b = M.fold_batchnorm(conv, bn, dtype)
        assert torch.equal(w, want_w) and torch.equal(b, want_b) and w.dtype == b.dtype == torch.float32


def test_fused_block_shares_the_block_and_its_reference_is_the_original_forward():
    for ci, co, stride in [(16, 16, 1), (16, 32, 2), (16, 32, 1)]:
        blk = _seed_bn(E._BasicBlock(ci, co, stride), ci + stride).eval()
        fused = M.BasicBlockFused.from_block(blk)
        assert list(fused.state_dict().keys()) == list(blk.state_dict().keys())
        assert [n for n, _ in fused.named_children()] == [n for n, _ in blk.named_children()]
        assert all(a is b for a, b in zip(fused.parameters(), blk.parameters())) and all(a is b for a, b in zip(fused.buffers(), blk.buffers()))
        assert list(M.BasicBlockFused(ci, co, stride).state_dict().keys()) == list(blk.state_dict().keys())
        assert not fused.training and "_mphip_half" not in fused.__dict__
        x = torch.randn(2, ci, 5, 7)
        with torch.no_grad():
            assert torch.equal(fused._reference(x), blk(x))
        assert torch.equal(fused(x), blk(x)) and fused(x).requires_grad      # parameters require grad: the original PyTorch expression
        assert "_mphip_fold" not in fused.__dict__
    assert M.BasicBlockFused.from_block(E._BasicBlock(16, 16).train()).training


def _blocks(emtn):
    return [b for net in (emtn.head_pose_net, emtn.expression_net) for s in net.children() if isinstance(s, nn.Sequential) for b in s]


def test_switches_are_off_by_default_and_leave_the_keys_alone():
    emtn = E.Emtn()
    blocks = _blocks(emtn)
    assert len(blocks) == 16 and all(type(b) is E._BasicBlock for b in blocks)
    keys, modules, params = list(emtn.state_dict().keys()), [n for n, _ in emtn.named_modules()], list(emtn.parameters())
    assert M.native_emtn_resnets(emtn) is True and M.native_emtn_resnets(emtn) is False      # twice: nothing left to swap
    fused = _blocks(emtn)
    assert all(isinstance(b, M.BasicBlockFused) for b in fused) and sum(isinstance(m, M.BasicBlockFused) for m in emtn.modules()) == 16
    assert not any(isinstance(m, M.BasicBlockFused) for m in emtn.rotation_net.model.modules())
    assert isinstance(emtn.head_pose_net.conv1, nn.Conv2d) and isinstance(emtn.expression_net[3], nn.MaxPool2d)      # the stems stay
    assert list(emtn.state_dict().keys()) == keys and [n for n, _ in emtn.named_modules()] == modules
    assert all(a is b for a, b in zip(emtn.parameters(), params))
    assert M.native_emtn_resnets(emtn, False) is True and M.native_emtn_resnets(emtn, False) is False
    assert all(a is b for a, b in zip(blocks, _blocks(emtn))) and list(emtn.state_dict().keys()) == keys
    assert emtn.native_resnets() is emtn and all(isinstance(b, M.BasicBlockFused) for b in _blocks(emtn))
    assert emtn.native_resnets(False) is emtn and all(a is b for a, b in zip(blocks, _blocks(emtn)))
    # Gbase reaches the same function (stubs for the encoders this test does not look at)
    g = gbase.Gbase(appearanceEncoder=nn.Identity(), motionEncoder=emtn, G2d=nn.Identity(), image_pyramid=nn.Identity())
    gkeys = list(g.state_dict().keys())
    assert g.native_motion_encoder() is g and all(isinstance(b, M.BasicBlockFused) for b in _blocks(emtn))
    assert list(g.state_dict().keys()) == gkeys
    assert g.native_motion_encoder(False) is g and all(a is b for a, b in zip(blocks, _blocks(emtn)))
