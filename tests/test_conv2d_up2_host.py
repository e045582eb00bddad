"""Host-side checks of the 2-D convs with a bilinear x2 up-sample folded in and of the fused G2d stage built on them (no GPU): exported
symbols (mphip_conv2d_up2_supported, mphip_conv2d_up2_workspace_bytes, mphip_conv2d_up2_fwd, mphip_conv2d_resup2_fwd), ABI version, the
shape rule, argument refusals, the register table, the arithmetic of model.up2_reference, the switches and the record that no existing
kernel changed."""
import copy
import ctypes
import json
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, integration, model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mphip_conv2d_up2_supported", "mphip_conv2d_up2_workspace_bytes", "mphip_conv2d_up2_fwd", "mphip_conv2d_resup2_fwd")


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 23     # the entries exist since ABI 23
    header = open(os.path.join(ROOT, "include", "mphip.h")).read()
    assert all(name + "(" in header for name in ENTRIES)


def test_shape_rule_is_the_plain_convs_on_the_output_map():
    lib = _lib.load()
    cases = [(1, 3, 64, 8, 8), (1, 16, 48, 8, 8), (1, 16, 32, 0, 8), (1, 16, 32, 8, 0), (0, 16, 32, 8, 8), (1, 8, 32, 8, 8),
             (1, 16, 32, 1 << 14, 1 << 15),          # 2h * 2w = 2^31
             (1, 16, 32, 1 << 14, (1 << 15) - 1),    # x: below 2^31 elements, y: not
             (1, 16, 32, 1 << 13, 1 << 13),          # x: 2^30, y: 2^33 elements
             (8, 512, 256, 64, 64), (8, 128, 64, 256, 256), (1, 16, 32, 1, 1), (3, 48, 96, 13, 19), (2, 16, 32, 4096, 4096),
             (1, 16, 32, 1, (1 << 25) - 1)]
    seen = set()
    for n, ci, co, h, w in cases:
        want = lib.mphip_conv2d_supported(n, ci, co, 2 * h, 2 * w)
        seen.add(want)
        assert lib.mphip_conv2d_up2_supported(n, ci, co, h, w) == want, (n, ci, co, h, w)
        assert lib.mphip_conv2d_up2_workspace_bytes(n, ci, co, h, w) == (4100 * 4 if want else 0)
        assert lib.mphip_conv2d_up2_workspace_bytes(n, ci, co, h, w) == lib.mphip_conv2d_workspace_bytes(n, ci, co, 2 * h, 2 * w)
    assert seen == {0, 1}
    for big in [(1, 16, 32, 1 << 30, 1), (1, 16, 32, 1, 1 << 30), (1, 16, 32, (1 << 31) - 1, 1)]:      # 2h, 2w do not fit an int
        assert lib.mphip_conv2d_up2_supported(*big) == 0 and lib.mphip_conv2d_up2_workspace_bytes(*big) == 0


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 17)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, r, s = (ctypes.c_void_p(base + i * 16384) for i in range(4))               # disjoint 16 KiB regions: x, y, workspace, residual
    at = lambda reg, off: ctypes.c_void_p(reg.value + off)

    def up2(n, ci, co, h, w, x=p, wp=p, b=p, res=None, y=q, ws=r, wsb=1 << 20):
        return lib.mphip_conv2d_up2_fwd(x, None, wp, b, res, y, None, n, ci, co, h, w, 1, ws, wsb, None)

    def resup2(n, ci, co, h, w, x=p, wp=p, b=p, res=s, y=q, ws=r, wsb=1 << 20):
        return lib.mphip_conv2d_resup2_fwd(x, None, wp, b, res, y, None, n, ci, co, h, w, 1, ws, wsb, None)

    for fwd, name in ((up2, b"conv2d_up2_fwd"), (resup2, b"conv2d_resup2_fwd")):
        for bad in [(1, 8, 32, 4, 4), (1, 16, 48, 4, 4), (1, 16, 32, 0, 4), (1, 16, 32, 4, 1 << 30)]:
            assert fwd(*bad) == -1 and name + b": unsupported shape" in lib.mphip_last_error(), bad
        for missing in ("x", "wp", "b", "y"):
            assert fwd(1, 16, 32, 4, 4, **{missing: None}) == -1 and name + b": null pointer" in lib.mphip_last_error()
        assert fwd(1, 16, 32, 4, 4, wsb=4100 * 4 - 1) == -3 and name + b": workspace" in lib.mphip_last_error()
        assert fwd(1, 16, 32, 4, 4, ws=None, wsb=0) == -3
        assert fwd(1, 16, 32, 4, 4, b=None, wsb=0) == -1                              # the argument error wins
        for alias in (dict(y=p), dict(y=at(p, 64)), dict(res=q)):                    # y = x, y inside x, residual = y
            assert fwd(1, 16, 32, 4, 4, **alias) == -1 and b"must not alias" in lib.mphip_last_error(), (name, alias)
    assert up2(1, 16, 32, 1 << 14, 1 << 15) == -1                                    # fits as an input, not as the doubled output
    # up2: x is [1,16,4,4] = 1 KiB, y and the residual are [1,32,8,8] = 8 KiB
    assert up2(1, 16, 32, 4, 4, x=at(q, -1024), wsb=0) == -3 and up2(1, 16, 32, 4, 4, x=at(q, -1020), wsb=0) == -1
    assert up2(1, 16, 32, 4, 4, res=at(q, 8192), wsb=0) == -3 and up2(1, 16, 32, 4, 4, res=at(q, 8188), wsb=0) == -1
    # resup2: the up-sampled residual is required, lives on the halved map ([1,32,4,4] = 2 KiB), and the map has even extents
    assert resup2(1, 16, 32, 8, 8, res=None) == -1 and b"conv2d_resup2_fwd: null pointer" in lib.mphip_last_error()
    assert resup2(1, 16, 32, 8, 8, res=at(q, -2048), wsb=0) == -3 and resup2(1, 16, 32, 8, 8, res=at(q, -2044), wsb=0) == -1
    assert resup2(1, 16, 32, 8, 8, res=at(q, 8192), wsb=0) == -3 and resup2(1, 16, 32, 8, 8, res=at(q, 8188), wsb=0) == -1
    for odd in [(7, 8), (8, 7), (1, 1)]:
        assert resup2(1, 16, 32, *odd) == -1 and b"even extents" in lib.mphip_last_error(), odd
        assert resup2(1, 16, 32, *odd, wsb=0) == -1                                   # before the workspace


def test_kernels_are_in_the_register_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import register_table

    kernels = register_table.collect(["conv2d_up2_f16x3.hip"])["conv2d_up2_f16x3.hip"]["kernels"]
    assert sorted(k["demangled"].split("<")[0].split("(")[0] for k in kernels) == ["conv2d_k3_resup2_f16x3_kernel", "conv2d_k3_up2_f16x3_kernel"]
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, k                     # two waves per SIMD
        assert k["group_segment_fixed_size"] <= 80 * 1024, k                           # two workgroups per CU (160 KiB of LDS)
    lds = {k["demangled"]: k["group_segment_fixed_size"] for k in kernels}
    # the patch (6400 B) and the two coordinate tables (2 * 18 * 16 B) on top of the plain kernel's LDS
    assert lds["conv2d_k3_up2_f16x3_kernel"] == lds["conv2d_k3_resup2_f16x3_kernel"] + 6400 + 576


def test_closed_form_coordinates_are_the_formula():
    """The kernels take i0 and the remainder from a closed form (conv2d_f16x3_tile.h, up2_coord): the same integers as the division."""
    for l in list(range(1, 200)) + [255, 256, 257, 511, 600, 4097, (1 << 20) + 1]:
        for i in (range(2 * l) if l <= 600 else [0, 1, 2, 3, l - 1, l, l + 1, 2 * l - 2, 2 * l - 1]):
            num, den = i * (l - 1), 2 * l - 1
            m, odd = i >> 1, i & 1
            i0 = m if odd else max(m - 1, 0)
            rem = l - 1 - m if odd else (2 * l - 1 - m if m else 0)
            assert (i0, rem) == (num // den, num % den), (l, i)
    # a 16 x 16 tile's 18 halo rows 16k-1 .. 16k+16 blend from at most 10 source rows, the first being i0 of the halo's first row
    for l in range(1, 601):
        for t0 in range(0, 2 * l, 16):
            rows = [g for g in range(t0 - 1, t0 + 17) if 0 <= g < 2 * l]
            i0s = [(g * (l - 1)) // (2 * l - 1) for g in rows]
            first = (t0 >> 1) - 1 if t0 else 0
            assert min(i0s) == first and min(max(i0s) + 1, l - 1) - first <= 9, (l, t0)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (2, 3), (5, 7), (9, 11), (16, 16)])
def test_up2_reference_against_fp64(h, w):
    torch.manual_seed(h * 31 + w)
    x = torch.randn(2, 3, h, w)
    u64 = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=True)
    u32 = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    u = M.up2_reference(x)
    assert u.dtype == torch.float32 and u.shape == u64.shape == (2, 3, 2 * h, 2 * w)
    e_ref, e_torch = (u.double() - u64).abs().max().item(), (u32.double() - u64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -22 * u64.abs().max().item()
    print(f"up2_reference {h}x{w}: e_ref={e_ref:.3e} e_torch={e_torch:.3e} bound={bound:.3e}")
    assert e_ref <= bound
    assert torch.equal(u[:, :, 0, 0], x[:, :, 0, 0]) and torch.equal(u[:, :, -1, -1], x[:, :, -1, -1])      # the corners are aligned


def test_up2_reference_refuses_other_inputs():
    for bad in (torch.zeros(3, 4, 5), torch.zeros(1, 1, 2, 2, dtype=torch.int32)):
        with pytest.raises(RuntimeError):
            M.up2_reference(bad)


def _up(**kw):
    return nn.Upsample(**{**dict(scale_factor=2, mode="bilinear", align_corners=True), **kw})


def test_matches_accepts_and_rejects_the_right_stages():
    ok = M.Up2ResBlock2DFused.matches
    assert ok(nn.Sequential(_up(), E.ResBlock2D(32, 64))) and ok(nn.Sequential(_up(scale_factor=(2.0, 2.0)), E.ResBlock2D(32, 64)))
    assert ok(nn.Sequential(_up(), M.ResBlock2DFused.from_block(E.ResBlock2D(32, 64))))
    assert all(ok(s) for s in (E.G2d().upsample1, E.G2d().upsample2, E.G2d().upsample3))
    assert not ok(nn.Sequential(_up(), E.ResBlock2D(32, 32)))                              # an Identity shortcut stays unfused
    assert not ok(nn.Sequential(_up(align_corners=False), E.ResBlock2D(32, 64)))
    assert not ok(nn.Sequential(_up(mode="nearest", align_corners=None), E.ResBlock2D(32, 64)))
    assert not ok(nn.Sequential(_up(mode="bicubic"), E.ResBlock2D(32, 64)))
    assert not ok(nn.Sequential(_up(scale_factor=3), E.ResBlock2D(32, 64))) and not ok(nn.Sequential(_up(scale_factor=(2, 1)), E.ResBlock2D(32, 64)))
    assert not ok(nn.Sequential(nn.Upsample(size=(8, 8), mode="bilinear", align_corners=True), E.ResBlock2D(32, 64)))
    assert not ok(nn.Sequential(_up(), E.ResBlock2D(32, 64, downsample=True)))
    assert not ok(nn.Sequential(_up(), E.ResBlock2D(32, 64), nn.ReLU())) and not ok(nn.Sequential(E.ResBlock2D(32, 64), _up()))
    assert not ok(E.ResBlock2D(32, 64)) and not ok(nn.Sequential())
    assert not ok(M.Up2ResBlock2DFused.from_sequential(nn.Sequential(_up(), E.ResBlock2D(32, 64))))      # already fused
    with pytest.raises(TypeError):
        M.Up2ResBlock2DFused.from_sequential(nn.Sequential(_up(), E.ResBlock2D(32, 32)))


def _stages(g2d):
    return [g2d.upsample1, g2d.upsample2, g2d.upsample3]


def _objects(g2d):
    return _stages(g2d) + [s[i] for s in _stages(g2d) for i in (0, 1)] + list(g2d.res_blocks)


def test_switch_is_off_by_default_and_leaves_keys_and_objects_alone():
    g2d = E.G2d()
    keys, modules, params = list(g2d.state_dict().keys()), [n for n, _ in g2d.named_modules()], list(g2d.parameters())
    originals = _objects(g2d)
    # without the keyword: today's behaviour, the Sequentials stay
    assert M.native_g2d_body(g2d) is True and all(type(s) is nn.Sequential for s in _stages(g2d))
    assert M.native_g2d_body(g2d, fuse_upsample=True) is True and M.native_g2d_body(g2d, fuse_upsample=True) is False      # twice: a no-op
    assert all(isinstance(s, M.Up2ResBlock2DFused) and isinstance(s[1], M.ResBlock2DFused) for s in _stages(g2d))
    assert all(s[0] is o for s, o in zip(_stages(g2d), originals[3::2])) and all(isinstance(b, M.ResBlock2DFused) for b in g2d.res_blocks)
    assert list(g2d.state_dict().keys()) == keys and [n for n, _ in g2d.named_modules()] == modules
    assert "upsample1.1.conv1.weight" in keys and all(a is b for a, b in zip(g2d.parameters(), params))
    # the keyword off again: the Sequentials come back, the blocks stay fused
    assert M.native_g2d_body(g2d) is True and all(a is b for a, b in zip(_stages(g2d), originals[:3]))
    assert all(isinstance(s[1], M.ResBlock2DFused) for s in _stages(g2d)) and M.native_g2d_body(g2d) is False
    # half_precision keeps the materialised up-sample
    assert M.native_g2d_body(g2d, True, True, True) is True and all(type(s) is nn.Sequential for s in _stages(g2d))
    assert all("_mphip_half" in s[1].__dict__ for s in _stages(g2d))
    assert M.native_g2d_body(g2d, fuse_upsample=True) is True and all(isinstance(s, M.Up2ResBlock2DFused) for s in _stages(g2d))
    assert not any("_mphip_half" in s[1].__dict__ for s in _stages(g2d))
    assert M.native_g2d_body(g2d, half_precision=True, fuse_upsample=True) is True and all(type(s) is nn.Sequential for s in _stages(g2d))
    # enable=False: the very objects of before, from either state
    assert M.native_g2d_body(g2d, False) is True and all(a is b for a, b in zip(originals, _objects(g2d)))
    assert M.native_g2d_body(g2d, False) is False
    assert g2d.native_body(fuse_upsample=True) is g2d and all(isinstance(s, M.Up2ResBlock2DFused) for s in _stages(g2d))
    assert g2d.native_body(False, fuse_upsample=True) is g2d and all(a is b for a, b in zip(originals, _objects(g2d)))
    assert list(g2d.state_dict().keys()) == keys and [n for n, _ in g2d.named_modules()] == modules
    # Gbase and integration.install reach the same function
    g = gbase.Gbase(appearanceEncoder=nn.Identity(), motionEncoder=nn.Identity(), G2d=g2d, image_pyramid=nn.Identity())
    gkeys = list(g.state_dict().keys())
    assert g.native_body(fuse_upsample=True) is g and all(isinstance(s, M.Up2ResBlock2DFused) for s in _stages(g2d))
    assert g.native_body(False) is g and all(a is b for a, b in zip(originals, _objects(g2d)))
    assert "G2d.body" in integration.install(g, eapp_tail=False, g2d_body=True) and all(type(s) is nn.Sequential for s in _stages(g2d))
    g.native_body(False)
    assert "G2d.body" in integration.install(g, eapp_tail=False, g2d_body=True, fuse_upsample=True)
    assert all(isinstance(s, M.Up2ResBlock2DFused) for s in _stages(g2d)) and list(g.state_dict().keys()) == gkeys
    g.native_body(False)
    assert all(a is b for a, b in zip(originals, _objects(g2d)))


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


@pytest.mark.parametrize("mode", ["train", "input_grad", "param_grad", "half"])
def test_fallbacks_are_the_original_sequential(mode):
    torch.manual_seed(3)
    seq = _seed_bn(nn.Sequential(_up(), E.ResBlock2D(16, 32)), 4).eval()
    x = torch.randn(2, 16, 5, 7)
    if mode == "train":
        seq.train()
    if mode == "half":
        seq, x = seq.bfloat16(), x.bfloat16()      # (a half dtype the CPU convolves)
    if mode != "param_grad":
        seq.requires_grad_(mode == "train")
    x.requires_grad_(mode == "input_grad")
    stage = M.Up2ResBlock2DFused.from_sequential(seq)
    assert stage.training == seq.training and not stage._native_ok(x)
    stats = [b.clone() for b in seq.buffers()]
    want = seq(x)
    with torch.no_grad():
        for b, s in zip(seq.buffers(), stats):      # train mode steps the running statistics: rewind, so both see the same state
            b.copy_(s)
    got = stage(x)
    assert torch.equal(got, want) and got.dtype == want.dtype and "_mphip_fold" not in stage[1].__dict__
    if mode != "half":
        got.square().sum().backward()
        assert (x.grad if mode == "input_grad" else seq[1].shortcut[0].weight.grad).abs().max() > 0


def test_cli_passes_the_keyword_only_with_the_flag():
    from megaportrait_hack_amd import reenact

    args = reenact.parse(["--random-init", "--source-tensor", "a", "--drivers-tensor", "b"])
    assert args.native_fuse_upsample is False
    assert reenact.parse(["--random-init", "--source-tensor", "a", "--drivers-tensor", "b", "--native-fuse-upsample"]).native_fuse_upsample
    src = open(os.path.join(ROOT, "megaportrait-hack_amd", "reenact.py")).read()
    assert '{"fuse_upsample": True} if args.native_fuse_upsample else {}' in src      # no extra argument when the flag is absent


def test_isa_record_says_no_existing_kernel_changed():
    rec = json.load(open(os.path.join(ROOT, "profiles", "conv2d_up2_isa.json")))
    files = ["conv2d_f16x3.hip", "conv2d_gn_f16x3.hip", "conv2d_lp.hip", "conv2d_s2_f16x3.hip", "conv3d.hip"]
    assert rec["files"] == files and rec["parent_commit"]
    assert {k["file"] for k in rec["kernels"]} == set(files) and len(rec["kernels"]) >= 20
    names = {k["result"].split("<")[0] for k in rec["kernels"]}
    assert {"conv2d_k3_f16x3_kernel", "conv2d_k3_cat_f16x3_kernel", "conv2d_k3_lp_kernel", "conv2d_k3_cat_lp_kernel", "conv2d_k3s2_f16x3_kernel"} <= names
    for k in rec["kernels"]:
        assert k["isa_equal"] is True and k["metadata_equal"] is True and k["isa_sha256"] == k["parent_isa_sha256"], k["result"]
        assert k["instructions"][0] == k["instructions"][1] > 0
