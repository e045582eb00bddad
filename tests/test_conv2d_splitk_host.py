"""Host-side checks of the split-K form of the 2-D 3x3 convs and of the split_small_maps switches (no GPU): exported symbols
(mphip_conv2d_split_supported, mphip_conv2d_splits, _workspace_bytes, _fwd) inside ABI 25, the shape rule, splits == 1 against the plain and
grouped entries, argument refusals and their order, the recommendation for the two nets' shapes, the register table, and the switches
(model.native_emtn_resnets / native_rotation_net, Emtn, Gbase, integration.install, reenact): swap, restore and the CPU fall-back."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn as nn

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, integration, model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mphip_conv2d_split_supported", "mphip_conv2d_splits", "mphip_conv2d_split_workspace_bytes", "mphip_conv2d_split_fwd")
RANGE_BYTES = 4100 * 4
# conv2d_k3_split_f16x3_kernel<GRP>, DESIGN.md section 3.14: (VGPRs, SGPRs, LDS bytes)
SPLIT_FIGURES = {"conv2d_k3_split_f16x3_kernel<0>": (208, 53, 57668), "conv2d_k3_split_f16x3_kernel<1>": (208, 54, 57668)}

# (N, Ci, Co, H, W, groups, splits)
GOOD = [(1, 32, 32, 1, 1, 1, 2), (2, 64, 96, 5, 7, 1, 4), (1, 96, 64, 17, 19, 1, 3), (1, 96, 64, 17, 19, 1, 6), (1, 64, 128, 9, 33, 2, 2),
        (1, 512, 512, 4, 4, 2, 8), (1, 256, 256, 8, 8, 1, 16), (8, 512, 512, 32, 32, 2, 16), (1, 16, 32, 8, 8, 1, 1), (1, 32, 128, 8, 8, 2, 1)]
BAD = [(1, 64, 64, 8, 8, 1, 0), (1, 64, 64, 8, 8, 1, -1), (1, 512, 512, 8, 8, 1, 17), (1, 512, 512, 8, 8, 1, 32),
       (1, 64, 64, 8, 8, 1, 3), (1, 96, 64, 8, 8, 1, 4), (1, 16, 32, 8, 8, 1, 2),      # no divisor of 4, 6 and 1 chunks
       (1, 32, 64, 8, 8, 2, 1), (1, 32, 64, 8, 8, 2, 2),      # Cog = 32: the grouped entry refuses it
       (1, 48, 128, 8, 8, 2, 1),                                # Cig = 24
       (1, 64, 128, 8, 8, 2, 4),                                # 4 divides Ci / 16 = 4, not (Ci / groups) / 16 = 2
       (1, 128, 256, 8, 8, 4, 8),                               # 8 divides Ci / 16 = 8, not (Ci / groups) / 16 = 2
       (1, 64, 128, 8, 8, 0, 2), (1, 64, 128, 8, 8, -1, 2),
       (0, 64, 64, 8, 8, 1, 2), (1, 0, 64, 8, 8, 1, 2), (1, 64, 0, 8, 8, 1, 2), (1, 64, 64, 0, 8, 1, 2), (1, 64, 64, 8, 0, 1, 2),
       (1, 32, 32, 1 << 15, 1 << 16, 1, 2)]                     # a map of 2^31 elements

# The recommendation (mphip_conv2d_splits) for every stride-1 3x3 conv shape (Ci, Co, H, W, groups) of Emtn's two ResNet-18s and of the
# RepVGG-B1g2 backbone at a 512 x 512 frame -> (at B = 1, at B = 8).  DESIGN.md section 3.14 has the sweep the rule's constants rest on.
NET_SHAPES = {
    (64, 64, 256, 256, 1): (1, 1),       # ResNet-18 layer1: four chunks
    (128, 128, 128, 128, 1): (4, 1),     # ResNet-18 layer2, RepVGG stage 1 (plain blocks)
    (128, 128, 128, 128, 2): (1, 1),     # RepVGG stage 1 (grouped blocks): four chunks
    (256, 256, 64, 64, 1): (8, 1),       # ResNet-18 layer3, RepVGG stage 2
    (256, 256, 64, 64, 2): (4, 1),
    (512, 512, 32, 32, 1): (8, 1),       # ResNet-18 layer4, RepVGG stage 3 (B = 8: 256 workgroups)
    (512, 512, 32, 32, 2): (8, 1),
}


def test_library_exports_the_entries_inside_abi_25():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 25
    header = open(os.path.join(ROOT, "include", "mphip.h")).read()
    assert all(name + "(" in header for name in ENTRIES)
    assert "added within ABI 25" in header and "probes for these entries" in header


def test_shape_rule():
    from megaportrait_hack_amd import ops

    lib = _lib.load()
    for good in GOOD:
        n, ci, co, h, w, g, s = good
        assert lib.mphip_conv2d_split_supported(*good) == 1 and ops.conv2d_split_supported(*good), good
        want = RANGE_BYTES + (s * n * co * h * w * 4 if s > 1 else 0)      # the scan slot, then the partial maps
        assert lib.mphip_conv2d_split_workspace_bytes(*good) == want, good
    for bad in BAD:
        assert lib.mphip_conv2d_split_supported(*bad) == 0 and lib.mphip_conv2d_split_workspace_bytes(*bad) == 0, bad
        assert not ops.conv2d_split_supported(*bad)
    for s in range(1, 17):      # 12 chunks
        assert lib.mphip_conv2d_split_supported(1, 192, 64, 8, 8, 1, s) == (1 if 12 % s == 0 else 0)


def test_one_split_agrees_with_the_plain_and_grouped_entries():
    lib = _lib.load()
    for shape in [(1, 64, 64, 8, 8), (1, 8, 64, 8, 8), (2, 16, 32, 1, 1), (1, 16, 48, 8, 8), (1, 32, 128, 1 << 15, 1 << 16)]:
        assert lib.mphip_conv2d_split_supported(*shape, 1, 1) == lib.mphip_conv2d_supported(*shape)
        assert lib.mphip_conv2d_split_workspace_bytes(*shape, 1, 1) == lib.mphip_conv2d_workspace_bytes(*shape)
    for shape in [(1, 32, 128, 1, 1, 2), (8, 512, 512, 32, 32, 2), (1, 96, 192, 5, 5, 3), (1, 32, 64, 8, 8, 2), (1, 16, 128, 8, 8, 2),
                  (1, 128, 128, 8, 8, 4), (1, 32, 128, 8, 8, 0)]:
        assert lib.mphip_conv2d_split_supported(*shape, 1) == lib.mphip_conv2d_grouped_supported(*shape)
        assert lib.mphip_conv2d_split_workspace_bytes(*shape, 1) == lib.mphip_conv2d_grouped_workspace_bytes(*shape)


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 19)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, r = (ctypes.c_void_p(base + i * (1 << 16)) for i in range(3))      # three disjoint 64 KiB regions: x (and pack, bias), y, workspace
    at = lambda b, off: ctypes.c_void_p(b.value + off)

    def fwd(n, ci, co, h, w, g, s, x=p, xr=None, wp=p, b=p, res=None, y=q, ws=r, wsb=1 << 16):
        return lib.mphip_conv2d_split_fwd(x, xr, wp, b, res, y, None, n, ci, co, h, w, g, s, 1, ws, wsb, None)

    for bad in BAD:
        assert fwd(*bad) == -1 and b"conv2d_split_fwd: unsupported shape" in lib.mphip_last_error(), (bad, lib.mphip_last_error())
    ok = (1, 32, 128, 4, 4, 1, 2)      # x: 512 floats = 2 KiB, y: 2048 floats = 8 KiB, two partial maps: 16 KiB behind the 16400-byte slot
    need = lib.mphip_conv2d_split_workspace_bytes(*ok)
    assert need == RANGE_BYTES + 2 * 8192
    for shape in (ok, (1, 64, 128, 4, 4, 2, 2), (1, 32, 128, 4, 4, 1, 1)):      # one split reports under the called entry's name too
        for missing in ("x", "wp", "b", "y"):
            assert fwd(*shape, **{missing: None}) == -1 and b"conv2d_split_fwd: null pointer" in lib.mphip_last_error()
    # the shared order: null pointer, shape, alignment, aliasing, workspace
    assert fwd(1, 32, 128, 4, 4, 1, 3, x=None) == -1 and b"conv2d_split_fwd: null pointer" in lib.mphip_last_error()
    assert fwd(1, 32, 128, 4, 4, 1, 3, x=at(p, 2), y=p) == -1 and b"conv2d_split_fwd: unsupported shape" in lib.mphip_last_error()
    assert fwd(*ok, x=at(p, 2), y=p) == -1 and b"aligned" in lib.mphip_last_error()
    assert fwd(*ok, wp=at(p, 4), y=p) == -1 and b"16-byte aligned" in lib.mphip_last_error()
    for alias in (dict(y=p), dict(y=at(p, 2044)), dict(x=at(q, 8188)), dict(res=at(q, 8188)), dict(res=q)):
        assert fwd(*ok, wsb=0, **alias) == -1 and b"must not alias" in lib.mphip_last_error(), alias
    assert fwd(*ok, wsb=need - 4) == -3 and b"conv2d_split_fwd: workspace" in lib.mphip_last_error()
    assert fwd(*ok, ws=None, wsb=0) == -3
    # the partial maps are needed with a descriptor too (the slot is not): 16 KiB then
    assert fwd(*ok, xr=p, wsb=2 * 8192 - 4) == -3 and b"conv2d_split_fwd: workspace" in lib.mphip_last_error()
    assert fwd(*ok, xr=p, ws=None, wsb=0) == -3
    assert fwd(*ok, b=None, wsb=16) == -1      # the argument error wins
    # a workspace that is large enough and whose partial maps lie on y, x or the residual
    # (refused before the scan of x is launched; every address lies inside the buffer all the same)
    for clash in (dict(ws=at(q, -RANGE_BYTES)), dict(x=at(p, 1 << 15), ws=at(p, (1 << 15) - RANGE_BYTES)),
                  dict(ws=at(q, 8192 - RANGE_BYTES), res=at(q, 8192))):
        assert fwd(*ok, wsb=1 << 17, **clash) == -1 and b"partial maps must not alias" in lib.mphip_last_error(), clash
    assert fwd(*ok, ws=at(r, 2), wsb=1 << 16) == -1 and b"4-byte aligned" in lib.mphip_last_error()


def test_the_recommendation_for_the_two_nets():
    from megaportrait_hack_amd import ops

    lib = _lib.load()
    for (ci, co, h, w, g), (b1, b8) in NET_SHAPES.items():
        for n, want in ((1, b1), (8, b8)):
            got = lib.mphip_conv2d_splits(n, ci, co, h, w, g)
            assert got == want == ops.conv2d_splits(n, ci, co, h, w, g), ((n, ci, co, h, w, g), got, want)
            assert lib.mphip_conv2d_split_supported(n, ci, co, h, w, g, got) == 1
    # the rule: at least eight chunks and at most 128 workgroups unsplit; a power of two up to 8 that divides the chunks and leaves every
    # workgroup two; at most 512 workgroups split
    assert lib.mphip_conv2d_splits(2, 128, 128, 128, 64, 1) == 4 and lib.mphip_conv2d_splits(2, 128, 128, 128, 80, 1) == 1      # 128 and 160 workgroups
    assert lib.mphip_conv2d_splits(1, 32, 32, 8, 8, 1) == 1 and lib.mphip_conv2d_splits(1, 112, 64, 8, 8, 1) == 1      # two and seven chunks
    assert lib.mphip_conv2d_splits(1, 128, 64, 8, 8, 1) == 4           # eight chunks: 8 would leave one each
    assert lib.mphip_conv2d_splits(1, 192, 64, 8, 8, 1) == 4           # twelve chunks: 4 divides, 8 does not
    assert lib.mphip_conv2d_splits(1, 160, 64, 8, 8, 1) == 2           # ten chunks
    assert lib.mphip_conv2d_splits(1, 144, 64, 8, 8, 1) == 1           # nine chunks: no power of two divides
    assert lib.mphip_conv2d_splits(1, 256, 64, 128, 128, 1) == 8 and lib.mphip_conv2d_splits(1, 256, 64, 144, 128, 1) == 4      # 64 and 72 workgroups
    assert lib.mphip_conv2d_splits(1, 1024, 64, 8, 8, 1) == 8          # 64 chunks: never above 8
    for bad in [(1, 8, 64, 8, 8, 1), (1, 32, 64, 8, 8, 2), (1, 64, 64, 8, 8, 0), (0, 64, 64, 8, 8, 1)]:
        assert lib.mphip_conv2d_splits(*bad) == 1                      # a shape no entry takes


def test_kernels_are_in_the_register_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import register_table

    table = register_table.collect(["conv2d_splitk_f16x3.hip"])
    kernels = {k["demangled"].split("(")[0]: k for k in table["conv2d_splitk_f16x3.hip"]["kernels"]}
    assert sorted(kernels) == sorted(list(SPLIT_FIGURES) + ["conv2d_split_finish_kernel<0>", "conv2d_split_finish_kernel<1>"]), sorted(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 3.14"):]
    for name, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["max_flat_workgroup_size"] == 256
    for name, (vgprs, sgprs, lds) in SPLIT_FIGURES.items():
        k = kernels[name]
        assert k["vgpr_count"] <= 256                                          # two waves per SIMD of 512 registers
        assert 2 * k["group_segment_fixed_size"] <= 160 * 1024                # two workgroups per CU
        assert (k["vgpr_count"], k.get("agpr_count", 0), k["sgpr_count"], k["group_segment_fixed_size"]) == (vgprs, 0, sgprs, lds), k
        assert f"{vgprs} VGPRs" in sec and f"{sgprs} SGPRs" in sec and f"{lds} B" in sec


def _fused(net, cls):
    return [m for m in net.modules() if isinstance(m, cls)]


def test_the_switches_set_the_attribute_and_take_it_back():
    assert M.BasicBlockFused.split_small_maps is False and M.RepVGGBlockFused.split_small_maps is False
    emtn = E.Emtn()
    nets = (emtn.head_pose_net, emtn.expression_net)
    res = lambda: [b for net in nets for b in _fused(net, M.BasicBlockFused)]
    rot = lambda: _fused(emtn.rotation_net.model, M.RepVGGBlockFused)
    keys = list(emtn.state_dict().keys())
    assert M.native_emtn_resnets(emtn, False, split_small_maps=True) is False and not res()
    assert M.native_emtn_resnets(emtn) is True and len(res()) == 16 and not any(b.split_small_maps for b in res())
    assert not any("split_small_maps" in b.__dict__ for b in res())
    assert M.native_emtn_resnets(emtn, True, split_small_maps=True) is True and all(b.split_small_maps for b in res())
    assert M.native_emtn_resnets(emtn, True, split_small_maps=True) is False                      # nothing left to change
    assert M.native_emtn_resnets(emtn, True) is True and not any(b.split_small_maps for b in res())       # without the keyword: off again
    assert M.native_emtn_resnets(emtn, True, True) is True and M.native_emtn_resnets(emtn, False) is True and not res()
    assert M.native_emtn_resnets(emtn, True) is True and not any(b.split_small_maps for b in res())       # new blocks start unsplit
    M.native_emtn_resnets(emtn, False)
    assert M.native_rotation_net(emtn, True, split_small_maps=True) is True and len(rot()) == 27 and all(b.split_small_maps for b in rot())
    assert not res()
    assert M.native_rotation_net(emtn, True) is True and not any(b.split_small_maps for b in rot())
    assert M.native_rotation_net(emtn.rotation_net, True, True) is True and M.native_rotation_net(emtn.rotation_net.model, True, True) is False
    assert M.native_rotation_net(emtn, False, split_small_maps=True) is True and not rot()
    # Emtn's and Gbase's methods, install and the command line
    assert emtn.native_resnets(split_small_maps=True) is emtn and all(b.split_small_maps for b in res()) and not rot()
    assert emtn.native_rotation_net(split_small_maps=True) is emtn and all(b.split_small_maps for b in rot())
    assert emtn.native_resnets() is emtn and not any(b.split_small_maps for b in res()) and all(b.split_small_maps for b in rot())
    assert emtn.native_resnets(False) is emtn and emtn.native_rotation_net(False) is emtn and not res() and not rot()
    assert list(emtn.state_dict().keys()) == keys
    g = gbase.Gbase(appearanceEncoder=nn.Identity(), motionEncoder=emtn, G2d=nn.Identity(), image_pyramid=nn.Identity())
    assert g.native_motion_encoder() is g and len(res()) == 16 and not any(b.split_small_maps for b in res())
    assert g.native_motion_encoder(rotation_net=True, split_small_maps=True) is g and all(b.split_small_maps for b in res() + rot())
    assert len(rot()) == 27
    assert g.native_motion_encoder(split_small_maps=True) is g and all(b.split_small_maps for b in res()) and not rot()
    assert g.native_motion_encoder() is g and not any(b.split_small_maps for b in res())
    assert g.native_motion_encoder(False, split_small_maps=True) is g and not res() and not rot()
    with pytest.raises(ValueError):
        integration.install(g, eapp_tail=False, split_small_maps=True)                     # the keyword belongs to motion_encoder
    assert not res() and not rot()
    done = integration.install(g, eapp_tail=False, motion_encoder=True)
    assert "Emtn.resnets" in done and not any(b.split_small_maps for b in res())
    g.native_motion_encoder(False)
    done = integration.install(g, eapp_tail=False, motion_encoder=True, rotation_net=True, split_small_maps=True)
    assert "Emtn.resnets" in done and "Emtn.rotation_net" in done and all(b.split_small_maps for b in res() + rot())
    g.native_motion_encoder(False)
    assert not res() and not rot() and list(emtn.state_dict().keys()) == keys
    from megaportrait_hack_amd import reenact

    base = ["--random-init", "--source-tensor", "s.pt", "--drivers-tensor", "d.pt"]
    assert not reenact.parse(base).native_split_small_maps
    assert not reenact.parse(base + ["--native-motion-encoder"]).native_split_small_maps
    with pytest.raises(SystemExit):
        reenact.parse(base + ["--native-split-small-maps"])
    cli = reenact.parse(base + ["--native-motion-encoder", "--native-split-small-maps"])
    assert cli.native_motion_encoder and cli.native_split_small_maps and not cli.native_rotation_net


def test_blocks_still_match_and_the_cpu_fallback_is_the_original_expression():
    torch.manual_seed(9)
    block = E._BasicBlock(64, 64, 1).eval()
    assert M.BasicBlockFused.matches(block)
    fused = M.BasicBlockFused.from_block(block)
    fused.split_small_maps = True
    assert not M.BasicBlockFused.matches(fused) and fused.conv1 is block.conv1
    x = torch.randn(1, 64, 9, 7)
    xg = x.clone().requires_grad_(True)      # under autograd the block evaluates the original expression (a CPU map in eval mode is refused)
    assert not fused._native_ok(xg) and torch.equal(fused(xg), block(xg))
    rep = E._RepVGGDeployBlock(64, 128, 1, 2).eval()
    assert M.RepVGGBlockFused.matches(rep)
    frep = M.RepVGGBlockFused.from_block(rep)
    frep.split_small_maps = True
    with torch.no_grad():
        assert torch.equal(frep(x), rep(x))
    net = E.SixDRepNetBackbone().eval()
    img = torch.rand(1, 3, 40, 36) * 2 - 1
    with torch.no_grad():
        want_rot, want_rest = net(img)
        assert M.native_rotation_net(net, True, split_small_maps=True) is True
        try:
            rot, rest = net(img)
            assert torch.equal(rot, want_rot) and torch.equal(rest, want_rest)
        finally:
            M.native_rotation_net(net, False)


def test_python_keyword_is_checked_before_any_launch():
    from megaportrait_hack_amd import ops

    shape = (1, 64, 64, 8, 8)
    for bad in ("best", 2.0, True):
        with pytest.raises(RuntimeError, match="splits"):
            ops._conv2d_splits("conv2d", bad, False, shape, 1)
    assert ops._conv2d_splits("conv2d", None, False, shape, 1) == 1 and ops._conv2d_splits("conv2d", 1, True, shape, 1) == 1
    assert ops._conv2d_splits("conv2d", 4, False, shape, 1) == 4
    assert ops._conv2d_splits("conv2d", "auto", False, shape, 1) == ops.conv2d_splits(*shape)
    for typed_splits in (2, "auto"):
        with pytest.raises(RuntimeError, match="typed map, out_dtype or products"):
            ops._conv2d_splits("conv2d", typed_splits, True, shape, 1)
    with pytest.raises(RuntimeError, match="does not fit"):
        ops._conv2d_splits("conv2d", 3, False, shape, 1)
    with pytest.raises(RuntimeError, match="does not fit"):
        ops._conv2d_splits("conv2d_grouped", 4, False, (1, 64, 128, 8, 8), 2)
