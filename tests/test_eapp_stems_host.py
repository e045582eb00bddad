"""Host-side checks of the 7x7 stem conv unit and of Eapp's two fused stems (no GPU): exported symbols (mphip_conv2d_stem7_supported,
mphip_conv2d_stem7_packed_weight_bytes, mphip_pack_conv2d_stem7_weight, mphip_conv2d_stem7_workspace_bytes, mphip_conv2d_stem7_fwd), ABI
version, the shape rule, argument refusals in their order, the register table, module matching and the switches."""
import ctypes
import inspect
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, integration, model as M, ops, reenact

ENTRIES = ("mphip_conv2d_stem7_supported", "mphip_conv2d_stem7_packed_weight_bytes", "mphip_pack_conv2d_stem7_weight",
           "mphip_conv2d_stem7_workspace_bytes", "mphip_conv2d_stem7_fwd")
# LDS bytes at stride 1 and 2; unified registers (vector + accumulator) of the flat and of the pooled kernels
S7_LDS_S1, S7_LDS_S2, S7_VGPRS_FLAT, S7_VGPRS_POOL = 78976, 102016, 132, 180
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 29     # the entries exist since ABI 29
    i, p, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["mphip_conv2d_stem7_supported"] == (i, [i] * 7)
    assert _lib.SIGNATURES["mphip_conv2d_stem7_packed_weight_bytes"] == (sz, [i])
    assert _lib.SIGNATURES["mphip_pack_conv2d_stem7_weight"] == (i, [p, p, i, p])
    assert _lib.SIGNATURES["mphip_conv2d_stem7_workspace_bytes"] == (sz, [i] * 7)
    assert _lib.SIGNATURES["mphip_conv2d_stem7_fwd"] == (i, [p] * 6 + [i] * 8 + [p, sz, p])
    header = open(os.path.join(ROOT, "include", "mphip.h")).read()
    for name in ENTRIES:
        assert name + "(" in header
    assert list(inspect.signature(ops.conv2d_stem7).parameters) == ["x", "pack", "stride", "relu", "pool", "x_range", "want_range"]
    assert callable(ops.conv2d_stem7_supported) and ops.PackedConv2dStem7 is not ops.PackedConv2d
    # the packed size: a 16-byte header, then 11 chunks x 2 parts x 2 k groups x 64 channels x 8 halfs, whatever Co
    for co in (16, 32, 48, 64):
        assert lib.mphip_conv2d_stem7_packed_weight_bytes(co) == 16 + 11 * 2 * 2 * 64 * 8 * 2
    for co in (0, 8, 24, 80, 128, -16):
        assert lib.mphip_conv2d_stem7_packed_weight_bytes(co) == 0


def test_shape_rule():
    lib = _lib.load()
    for bad in [(1, 4, 64, 8, 8, 1, 0), (1, 16, 64, 8, 8, 1, 0), (1, 3, 24, 8, 8, 1, 0), (1, 3, 8, 8, 8, 1, 0), (1, 3, 80, 8, 8, 2, 1),
                (1, 3, 128, 8, 8, 1, 0),                                               # Co <= 64
                (1, 3, 64, 0, 8, 1, 0), (1, 3, 64, 8, 0, 2, 1), (0, 3, 64, 8, 8, 1, 0),
                (1, 3, 64, 8, 8, 0, 0), (1, 3, 64, 8, 8, 3, 1), (1, 3, 64, 8, 8, -1, 0),    # the stride is 1 or 2
                (1, 3, 16, 1 << 15, 1 << 16, 2, 1),     # H * W = 2^31
                (1, 3, 64, 1 << 13, 1 << 12, 1, 0),     # x: 3 * 2^25 elements, y: 64 * 2^25 = 2^31
                (256, 3, 64, 2048, 2048, 2, 1)]:        # x: 3 * 2^30 elements
        assert lib.mphip_conv2d_stem7_supported(*bad) == 0 and lib.mphip_conv2d_stem7_workspace_bytes(*bad) == 0, bad
        assert not ops.conv2d_stem7_supported(*bad)
    for ok in [(8, 3, 64, 512, 512, 1, 0), (8, 3, 64, 512, 512, 2, 1), (1, 3, 16, 1, 1, 1, 0), (1, 3, 16, 1, 1, 2, 1), (3, 3, 48, 13, 19, 1, 1),
               (3, 3, 32, 13, 19, 2, 0),
               (1, 3, 64, 1 << 13, 1 << 12, 2, 0),      # the rule counts the elements of y: the stride-2 map fits ...
               (1, 3, 64, 1 << 13, 1 << 12, 1, 1)]:     # ... and so does the pooled one
        assert lib.mphip_conv2d_stem7_supported(*ok) == 1 and lib.mphip_conv2d_stem7_workspace_bytes(*ok) >= 4100 * 4, ok
    assert ops.conv2d_stem7_supported(1, 3, 64, 8, 8) and ops.conv2d_stem7_supported(1, 3, 64, 8, 8, 2, True)


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced.  The order is the
    2-D entries': null pointer, unsupported shape, alignment, y overlapping x, then the workspace."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, r = (ctypes.c_void_p(base + i * 16384) for i in range(3))                 # three disjoint 16 KiB regions: x, y, workspace
    fwd = lambda n, ci, co, h, w, s, pool, x=p, wp=p, b=p, y=q, ws=r, wsb=1 << 20, xr=None: lib.mphip_conv2d_stem7_fwd(
        x, xr, wp, b, y, None, n, ci, co, h, w, s, 1, pool, ws, wsb, None)
    for bad in [(1, 4, 32, 8, 8, 1, 0), (1, 3, 24, 8, 8, 2, 0), (1, 3, 80, 8, 8, 1, 0), (1, 3, 32, 0, 8, 1, 0), (1, 3, 32, 8, 8, 0, 0),
                (1, 3, 32, 8, 8, 3, 1)]:
        assert fwd(*bad) == -1 and b"conv2d_stem7_fwd: unsupported shape" in lib.mphip_last_error()
    assert b"stride=3" in lib.mphip_last_error() and b"pool=1" in lib.mphip_last_error()
    ok = (1, 3, 32, 8, 8, 2, 0)      # x: 768 bytes, y: [1,32,4,4] = 2048 bytes
    for missing in ("x", "wp", "b", "y"):
        assert fwd(*ok, **{missing: None}) == -1 and b"conv2d_stem7_fwd: null pointer" in lib.mphip_last_error()
    assert fwd(1, 3, 32, 8, 8, 3, 0, b=None) == -1 and b"conv2d_stem7_fwd: null pointer" in lib.mphip_last_error()   # null pointer, then shape
    off = lambda ptr, n: ctypes.c_void_p(ptr.value + n)
    assert fwd(*ok, wp=off(p, 4)) == -1 and b"conv2d_stem7_fwd: w_packed" in lib.mphip_last_error()
    assert fwd(*ok, x=off(p, 2)) == -1 and b"4-byte aligned" in lib.mphip_last_error()
    assert fwd(*ok, xr=off(r, 1)) == -1 and b"4-byte aligned" in lib.mphip_last_error()
    assert fwd(1, 3, 24, 8, 8, 2, 0, wp=off(p, 4)) == -1 and b"unsupported shape" in lib.mphip_last_error()   # shape, then alignment
    assert fwd(*ok, wp=off(p, 4), y=p) == -1 and b"w_packed" in lib.mphip_last_error()                        # alignment, then aliasing
    assert fwd(*ok, wsb=4100 * 4 - 1) == -3 and b"conv2d_stem7_fwd: workspace" in lib.mphip_last_error()
    assert fwd(*ok, ws=None, wsb=0) == -3
    assert fwd(*ok, b=None, wsb=0) == -1                                            # the argument error wins
    for alias in (dict(y=p), dict(y=off(p, 64)), dict(x=off(q, 2044))):             # y = x, y inside x, x begins on y's last element
        assert fwd(*ok, **alias) == -1 and b"must not alias" in lib.mphip_last_error(), alias
        assert fwd(*ok, wsb=0, **alias) == -1                                       # aliasing, then the workspace
    assert fwd(*ok, x=off(q, 2048), wsb=0) == -3                                    # x begins where y ends: passes, stops at the workspace
    # the extents of y follow the stride and the pool: [1,32,8,8] = 8192 bytes at stride 1, [1,32,2,2] = 512 bytes pooled at stride 2
    assert fwd(1, 3, 32, 8, 8, 1, 0, x=off(q, 8188), wsb=0) == -1 and fwd(1, 3, 32, 8, 8, 1, 0, x=off(q, 8192), wsb=0) == -3
    assert fwd(1, 3, 32, 8, 8, 2, 1, x=off(q, 508), wsb=0) == -1 and fwd(1, 3, 32, 8, 8, 2, 1, x=off(q, 512), wsb=0) == -3
    # the pack entry refuses on the host as well
    assert lib.mphip_pack_conv2d_stem7_weight(None, p, 32, None) == -1 and b"pack_conv2d_stem7_weight: null" in lib.mphip_last_error()
    assert lib.mphip_pack_conv2d_stem7_weight(p, q, 80, None) == -1 and lib.mphip_pack_conv2d_stem7_weight(p, off(q, 4), 32, None) == -1


def test_kernels_are_in_the_register_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import register_table

    kernels = register_table.collect(["conv2d_stem7_f16x3.hip"])["conv2d_stem7_f16x3.hip"]["kernels"]
    by_name = {k["demangled"]: k for k in kernels}
    assert sorted(by_name) == ["conv2d_stem7_absmax_kernel", "conv2d_stem7_f16x3_kernel<1, 0>", "conv2d_stem7_f16x3_kernel<1, 1>",
                               "conv2d_stem7_f16x3_kernel<2, 0>", "conv2d_stem7_f16x3_kernel<2, 1>", "conv2d_stem7_pack_kernel"]
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    for stride, lds in ((1, S7_LDS_S1), (2, S7_LDS_S2)):
        flat, pool = by_name[f"conv2d_stem7_f16x3_kernel<{stride}, 0>"], by_name[f"conv2d_stem7_f16x3_kernel<{stride}, 1>"]
        assert flat["group_segment_fixed_size"] == pool["group_segment_fixed_size"] == lds
        # (vgpr_count is the unified file: vector and accumulator registers together) 512 / count >= 2 waves per SIMD
        assert flat["vgpr_count"] == S7_VGPRS_FLAT and pool["vgpr_count"] == S7_VGPRS_POOL <= 256
        assert flat["agpr_count"] == pool["agpr_count"] == 64       # the 2 x 2 tiles of 16 accumulators
    assert 2 * S7_LDS_S1 <= 160 * 1024 and S7_LDS_S2 <= 160 * 1024      # two workgroups per CU at stride 1, one at stride 2
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 3.16"):]
    assert f"{S7_LDS_S1} B" in sec and f"{S7_LDS_S2} B" in sec and f"{S7_VGPRS_FLAT} registers" in sec and f"{S7_VGPRS_POOL} registers" in sec


def _seed_bn(net, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g))
                m.weight.copy_(torch.randn(m.num_features, generator=g))
                m.bias.copy_(torch.randn(m.num_features, generator=g))
    return net


def test_matches_accepts_and_rejects_the_right_modules():
    ok = M.ConvStem7Fused.matches
    assert ok(nn.Conv2d(3, 64, 7, padding=3)) and ok(nn.Conv2d(3, 16, 7, stride=1, padding=3)) and ok(E.Eapp().conv)
    for bad in (nn.Conv2d(3, 64, 7, padding=3, bias=False), nn.Conv2d(3, 64, 7, stride=2, padding=3), nn.Conv2d(3, 64, 7, padding=2),
                nn.Conv2d(4, 64, 7, padding=3), nn.Conv2d(3, 128, 7, padding=3), nn.Conv2d(3, 24, 7, padding=3), nn.Conv2d(3, 64, 3, padding=1),
                nn.Conv2d(3, 64, 7, padding=3, padding_mode="reflect"), nn.Conv2d(3, 63, 7, padding=3, groups=3), nn.Identity(),
                M.ConvStem7Fused(nn.Conv2d(3, 64, 7, padding=3))):
        assert not ok(bad), bad
    assert M.Stem7Fused.matches(E.CustomResNet50())
    assert not M.Stem7Fused.matches(E.CifarResNet18()) and not M.StemFused.matches(E.CustomResNet50())      # the other stem's nets
    assert not M.Stem7Fused.matches(nn.Identity()) and not M.Stem7Fused.matches(nn.Sequential())

    def broken(edit):
        net = E.CustomResNet50()
        edit(net)
        return net

    assert not M.Stem7Fused.matches(broken(lambda n: setattr(n, "conv1", nn.Conv2d(3, 64, 7, stride=1, padding=3, bias=False))))
    assert not M.Stem7Fused.matches(broken(lambda n: setattr(n, "conv1", nn.Conv2d(3, 64, 7, stride=2, padding=1, bias=False))))
    assert not M.Stem7Fused.matches(broken(lambda n: setattr(n, "bn1", nn.BatchNorm2d(64, track_running_stats=False))))
    assert not M.Stem7Fused.matches(broken(lambda n: setattr(n, "bn1", nn.GroupNorm(32, 64))))
    assert not M.Stem7Fused.matches(broken(lambda n: setattr(n, "maxpool", nn.MaxPool2d(2, 2))))
    assert not M.Stem7Fused.matches(broken(lambda n: setattr(n, "maxpool", nn.MaxPool2d(3, 2, 1, ceil_mode=True))))
    assert not M.Stem7Fused.matches(broken(lambda n: setattr(n, "maxpool", nn.AvgPool2d(3, 2, 1))))
    with_bias = broken(lambda n: setattr(n, "conv1", nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=True)))
    assert M.Stem7Fused.matches(with_bias)      # a bias may be present: it is folded


def test_fold_of_the_stride2_stem_against_fp64():
    net = _seed_bn(E.CustomResNet50(), 5).double().eval()
    x = torch.randn(2, 3, 19, 23, dtype=torch.float64)
    with torch.no_grad():
        w, b = M.fold_batchnorm(net.conv1, net.bn1)
        want = net.maxpool(F.relu(net.bn1(net.conv1(x))))
        got = F.max_pool2d(F.relu(F.conv2d(x, w, b, stride=2, padding=3)), 3, 2, 1)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


class _ReferenceForwardResNet50(E.CustomResNet50):
    """The reference's forward (model.py:156-160): F.relu between bn1 and maxpool, one statement per step."""

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


def test_switches_are_off_by_default_and_leave_the_keys_alone():
    eapp = _seed_bn(E.Eapp(), 1)
    net = eapp.custom_resnet50
    conv, conv1, bn1, pool = eapp.conv, net.conv1, net.bn1, net.maxpool
    assert type(conv) is nn.Conv2d and type(conv1) is nn.Conv2d and type(bn1) is nn.BatchNorm2d and type(pool) is nn.MaxPool2d
    keys, modules, params, bufs = (list(eapp.state_dict().keys()), [n for n, _ in eapp.named_modules()], list(eapp.parameters()),
                                   list(eapp.buffers()))
    meta = eapp.state_dict()._metadata
    x = torch.randn(2, 3, 32, 40)
    with torch.no_grad():
        eapp.eval()
        t0, e0 = eapp.trunk2d(x), eapp.descriptor(x)
    assert M.native_eapp_stems(eapp) is True and M.native_eapp_stems(eapp) is False      # twice: nothing left to swap
    assert isinstance(eapp.conv, M.ConvStem7Fused) and isinstance(net.conv1, M.Stem7Fused)
    assert isinstance(net.bn1, M._Stem7Pass) and isinstance(net.maxpool, M._Stem7Pass)
    assert type(eapp.resblock_128) is E.ResBlock_Custom and type(net.layer1[0]) is E._Bottleneck      # other switches' blocks
    assert list(eapp.state_dict().keys()) == keys and [n for n, _ in eapp.named_modules()] == modules
    assert eapp.state_dict()._metadata == meta
    assert all(a is b for a, b in zip(eapp.parameters(), params)) and all(a is b for a, b in zip(eapp.buffers(), bufs))
    assert len(list(eapp.parameters())) == len(params) and len(list(eapp.buffers())) == len(bufs)
    assert not eapp.conv.training and not net.bn1.training
    with torch.no_grad():       # on the CPU the swapped modules run the original expression
        assert torch.equal(eapp.trunk2d(x), t0) and torch.equal(eapp.descriptor(x), e0)
        # ordinary 4-D tensors through the stand-ins: the original modules
        t = torch.randn(2, 64, 9, 11)
        assert torch.equal(net.bn1(t), bn1(t)) and torch.equal(net.maxpool(t), pool(t)) and torch.equal(net.conv1(x), conv1(x))
    eapp.train()
    assert bn1.training and conv.training and net.bn1.training      # train() reaches the originals
    eapp.eval()
    assert not bn1.training
    assert M.native_eapp_stems(eapp, False) is True and M.native_eapp_stems(eapp, False) is False
    assert eapp.conv is conv and net.conv1 is conv1 and net.bn1 is bn1 and net.maxpool is pool
    assert list(eapp.state_dict().keys()) == keys and [n for n, _ in eapp.named_modules()] == modules
    with torch.no_grad():
        assert torch.equal(eapp.descriptor(x), e0)
    assert eapp.native_stems() is eapp and isinstance(eapp.conv, M.ConvStem7Fused)
    # independent of the other two switches, in either order
    eapp.native_trunk().native_resnet50()
    assert isinstance(eapp.conv, M.ConvStem7Fused) and isinstance(eapp.resblock_128, M.ResBlockCustomFused)
    assert list(eapp.state_dict().keys()) == keys and [n for n, _ in eapp.named_modules()] == modules
    eapp.native_trunk(False).native_resnet50(False)
    assert isinstance(eapp.conv, M.ConvStem7Fused) and isinstance(net.conv1, M.Stem7Fused)
    assert eapp.native_stems(False) is eapp and eapp.conv is conv and net.conv1 is conv1
    # Gbase reaches the same function (stubs for the modules this test does not look at)
    g = gbase.Gbase(appearanceEncoder=eapp, motionEncoder=nn.Identity(), G2d=nn.Identity(), image_pyramid=nn.Identity())
    gkeys = list(g.state_dict().keys())
    assert g.native_stems() is g and isinstance(eapp.conv, M.ConvStem7Fused) and list(g.state_dict().keys()) == gkeys
    assert g.native_stems(False) is g and eapp.conv is conv and net.maxpool is pool
    assert M.native_eapp_stems(nn.Identity()) is False      # nothing to swap: not an error


def test_reference_forward_with_functional_relu_on_the_cpu():
    net = _seed_bn(_ReferenceForwardResNet50(), 2).eval()
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        want = net(x)
        assert M.Stem7Fused.swap(net) is True
        assert torch.equal(net(x), want)
        assert M.Stem7Fused.swap(net, False) is True and type(net.conv1) is nn.Conv2d


def test_load_state_dict_and_dtype_conversion_reach_the_originals():
    eapp = _seed_bn(E.Eapp(), 3).eval()
    net = eapp.custom_resnet50
    conv1, bn1 = net.conv1, net.bn1
    sd = {k: v.clone() for k, v in eapp.state_dict().items()}
    eapp.native_stems()
    with torch.no_grad():
        bn1.running_mean.add_(1.0)
    eapp.load_state_dict(sd, strict=True)
    assert torch.equal(bn1.running_mean, sd["custom_resnet50.bn1.running_mean"])
    eapp.custom_resnet50.conv1.double()
    assert conv1.weight.dtype == torch.float64
    eapp.native_stems(False)
    assert net.conv1 is conv1 and net.bn1 is bn1


def test_install_keyword_and_cli_flag_parse():
    assert list(inspect.signature(integration.install).parameters)[-1] == "eapp_stems"
    assert inspect.signature(integration.install).parameters["eapp_stems"].default is False
    eapp = E.Eapp()
    g = gbase.Gbase(appearanceEncoder=eapp, motionEncoder=nn.Identity(), G2d=nn.Identity(), image_pyramid=nn.Identity())
    assert "Eapp.stems" not in integration.install(g, eapp_tail=False) and type(eapp.conv) is nn.Conv2d
    done = integration.install(g, eapp_tail=False, eapp_stems=True)
    assert "Eapp.stems" in done and "Eapp.trunk2d" not in done and isinstance(eapp.conv, M.ConvStem7Fused)
    assert isinstance(eapp.custom_resnet50.conv1, M.Stem7Fused) and type(eapp.resblock_128) is E.ResBlock_Custom
    assert "Eapp.stems" not in integration.install(g, eapp_tail=False, eapp_stems=True)      # nothing left to swap
    assert reenact.parse(["--random-init", "--source", "s", "--drivers", "d"]).native_eapp_stems is False
    assert reenact.parse(["--random-init", "--source", "s", "--drivers", "d", "--native-eapp-stems"]).native_eapp_stems is True
