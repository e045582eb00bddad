"""Host-side checks of the 2-D 3x3 conv and of G2d's fused body (no GPU): exported symbols (mphip_conv2d_supported,
mphip_conv2d_packed_weight_bytes, mphip_pack_conv2d_weight, mphip_conv2d_workspace_bytes, mphip_conv2d_fwd), ABI version, size queries,
argument refusals, the register table, module matching, the BatchNorm fold and the switches."""
import ctypes
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, integration, model as M, reenact

ENTRIES = ("mphip_conv2d_supported", "mphip_conv2d_packed_weight_bytes", "mphip_pack_conv2d_weight", "mphip_conv2d_workspace_bytes",
           "mphip_conv2d_fwd")


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 19     # the entries exist since ABI 19
    assert lib.mphip_build_flags() == 0                                                            # the product build: no ablation


def test_size_queries_are_monotone():
    lib = _lib.load()
    pk = [lib.mphip_conv2d_packed_weight_bytes(co, 512) for co in (32, 64, 96, 128, 256, 512)]
    assert all(b > 0 for b in pk) and pk == sorted(pk) and pk[0] == pk[1] < pk[2] == pk[3]     # 64-channel co tiles
    pk = [lib.mphip_conv2d_packed_weight_bytes(512, ci) for ci in (16, 32, 64, 512)]
    assert pk == sorted(pk) and len(set(pk)) == 4
    assert lib.mphip_conv2d_packed_weight_bytes(64, 16) == 16 + 2 * 9 * 2 * 64 * 8 * 2           # header + one hi/lo slab
    assert lib.mphip_conv2d_packed_weight_bytes(512, 512) >= 512 * 512 * 9 * 4                   # two f16 halves per fp32 weight
    ws = [lib.mphip_conv2d_workspace_bytes(n, 512, 512, 64, 64) for n in (1, 2, 4, 8)]
    assert all(b >= 4100 * 4 for b in ws) and ws == sorted(ws)
    for ok in [(8, 512, 512, 64, 64), (8, 512, 256, 128, 128), (8, 128, 64, 512, 512), (1, 16, 32, 1, 1), (3, 48, 96, 13, 19)]:
        assert lib.mphip_conv2d_supported(*ok) == 1 and lib.mphip_conv2d_workspace_bytes(*ok) > 0
    for bad in [(1, 8, 32, 8, 8), (1, 16, 16, 8, 8), (1, 16, 32, 0, 8), (1, 16, 32, 8, 0), (0, 16, 32, 8, 8), (1, 24, 32, 8, 8),
                (1, 16, 48, 8, 8), (1, 16, 32, -1, 8), (64, 512, 512, 512, 512)]:
        assert lib.mphip_conv2d_supported(*bad) == 0 and lib.mphip_conv2d_workspace_bytes(*bad) == 0


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, r = (ctypes.c_void_p(base + i * 16384) for i in range(3))                 # three disjoint 16 KiB regions: x, y, workspace
    fwd = lambda n, ci, co, h, w, x=p, wp=p, b=p, res=None, y=q, ws=r, wsb=1 << 20: lib.mphip_conv2d_fwd(
        x, None, wp, b, res, y, None, n, ci, co, h, w, 1, ws, wsb, None)
    for bad in [(1, 8, 32, 8, 8), (1, 16, 16, 8, 8), (1, 16, 32, 0, 8)]:
        assert fwd(*bad) == -1 and b"unsupported shape" in lib.mphip_last_error()
    for missing in ("x", "wp", "b", "y"):
        assert fwd(1, 16, 32, 8, 8, **{missing: None}) == -1 and b"null pointer" in lib.mphip_last_error()
    assert fwd(1, 16, 32, 8, 8, wsb=4100 * 4 - 1) == -3 and b"workspace" in lib.mphip_last_error()
    assert fwd(1, 16, 32, 8, 8, ws=None, wsb=0) == -3
    for alias in (dict(y=p), dict(y=ctypes.c_void_p(p.value + 64)), dict(res=q)):   # y = x, y inside x, residual = y
        assert fwd(1, 16, 32, 8, 8, **alias) == -1 and b"must not alias" in lib.mphip_last_error(), alias
    assert lib.mphip_pack_conv2d_weight(p, p, 16, 16, None) == -1 and b"pack_conv2d_weight" in lib.mphip_last_error()
    assert lib.mphip_pack_conv2d_weight(p, p, 32, 8, None) == -1
    assert lib.mphip_pack_conv2d_weight(None, p, 32, 16, None) == -1 and b"null pointer" in lib.mphip_last_error()


def test_kernels_are_in_the_register_table_without_scratch():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import register_table

    kernels = register_table.collect(["conv2d_f16x3.hip"])["conv2d_f16x3.hip"]["kernels"]
    names = {k["demangled"].split("<")[0].split("(")[0] for k in kernels}
    assert names == {"conv2d_absmax_kernel", "conv2d_pack_kernel", "conv2d_range_kernel", "conv2d_out_range_init_kernel",
                     "conv2d_k3_f16x3_kernel"}
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    conv = [k for k in kernels if k["demangled"].startswith("conv2d_k3_f16x3_kernel")][0]
    assert conv["group_segment_fixed_size"] <= 80 * 1024          # two workgroups per CU (160 KiB of LDS)


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


def test_matches_accepts_and_rejects_the_right_modules():
    ok = M.ResBlock2DFused.matches
    assert ok(E.ResBlock2D(32, 32)) and ok(E.ResBlock2D(32, 64)) and isinstance(E.ResBlock2D(32, 64).shortcut, nn.Sequential)
    assert not ok(E.ResBlock2D(32, 32, downsample=True)) and not ok(nn.Conv2d(3, 3, 3)) and not ok(nn.Sequential())
    assert not ok(M.ResBlock2DFused(32, 32))                       # already fused

    def broken(edit):
        b = E.ResBlock2D(32, 64)
        edit(b)
        return b

    assert not ok(broken(lambda b: setattr(b, "conv1", nn.Conv2d(32, 64, 3, padding=1, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv2", nn.Conv2d(64, 64, 3, stride=2, padding=1))))
    assert not ok(broken(lambda b: setattr(b, "conv2", nn.Conv2d(64, 64, 5, padding=2))))
    assert not ok(broken(lambda b: setattr(b, "conv1", nn.Conv2d(32, 64, 3, padding=0))))
    assert not ok(broken(lambda b: setattr(b, "bn1", nn.BatchNorm2d(64, track_running_stats=False))))
    assert not ok(broken(lambda b: setattr(b, "bn2", nn.GroupNorm(32, 64))))
    assert not ok(broken(lambda b: setattr(b, "shortcut", nn.Identity())))         # 32 -> 64 channels need the 1x1 conv
    assert not ok(broken(lambda b: setattr(b, "shortcut", nn.Sequential(nn.Conv2d(32, 64, 1)))))
    assert not ok(broken(lambda b: setattr(b, "shortcut", nn.Sequential(nn.Conv2d(32, 64, 3, padding=1), nn.BatchNorm2d(64)))))

    class Other(nn.Module):                                         # the reference's own class qualifies by its attributes alone
        def __init__(self):
            super().__init__()
            self.downsample = False
            self.conv1, self.bn1 = nn.Conv2d(16, 32, 3, stride=1, padding=1), nn.BatchNorm2d(32)
            self.conv2, self.bn2 = nn.Conv2d(32, 32, 3, stride=1, padding=1), nn.BatchNorm2d(32)
            self.shortcut = nn.Sequential(nn.Conv2d(16, 32, 1, stride=1), nn.BatchNorm2d(32))

    assert ok(Other())
    try:
        M.ResBlock2DFused.from_block(nn.Conv2d(3, 3, 3))
        assert False
    except TypeError:
        pass


def test_fused_block_shares_the_block_and_falls_back_on_the_cpu_expression():
    blk = _seed_bn(E.ResBlock2D(16, 32)).eval()
    fused = M.ResBlock2DFused.from_block(blk)
    assert list(fused.state_dict().keys()) == list(blk.state_dict().keys())
    assert all(a is b for a, b in zip(fused.parameters(), blk.parameters())) and all(a is b for a, b in zip(fused.buffers(), blk.buffers()))
    assert not fused.training and M.ResBlock2DFused.from_block(E.ResBlock2D(16, 16).train()).training
    assert list(M.ResBlock2DFused(16, 32).state_dict().keys()) == list(blk.state_dict().keys())
    x = torch.randn(2, 16, 5, 7)
    assert torch.equal(fused(x), blk(x))                           # parameters require grad: the original PyTorch expression
    fused.train()
    assert fused.training and fused.bn1.training and fused(x).requires_grad     # train mode: batch statistics, autograd


def test_batchnorm_fold_equals_eval_mode_bn_of_conv_in_fp64():
    conv, bn = nn.Conv2d(16, 32, 3, padding=1).double(), nn.BatchNorm2d(32).double()
    _seed_bn(bn, 3)
    bn.eval()
    x = torch.randn(2, 16, 9, 11, dtype=torch.float64)
    w, b = M.fold_batchnorm(conv, bn)
    assert w.dtype == torch.float64 and not w.requires_grad
    want = bn(conv(x))
    assert (F.conv2d(x, w, b, padding=1) - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    sc = nn.Sequential(nn.Conv2d(16, 32, 1), nn.BatchNorm2d(32)).double().eval()
    _seed_bn(sc, 4)
    w, b = M.fold_batchnorm(sc[0], sc[1])
    assert (F.conv2d(x, w, b) - sc(x)).abs().max().item() <= 1e-12 * sc(x).abs().max().item()


def test_switches_are_off_by_default_and_leave_the_keys_alone():
    g2d = E.G2d()
    blocks = list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1]]
    assert len(blocks) == 11 and all(type(b) is E.ResBlock2D for b in blocks)
    g = gbase.Gbase(G2d=g2d)
    before = list(g.state_dict().keys())
    assert len(before) == 971        # the manifest tests/test_gbase.py checks name by name
    modules, params = [n for n, _ in g.named_modules()], list(g.parameters())
    assert g.native_body() is g
    fused = list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1]]
    assert all(isinstance(b, M.ResBlock2DFused) for b in fused) and isinstance(g2d.upsample1[0], nn.Upsample)
    assert list(g.state_dict().keys()) == before and all(a is b for a, b in zip(g.parameters(), params))
    assert [n for n, _ in g.named_modules()] == modules
    assert M.native_g2d_body(g2d, True) is False                    # twice: nothing left to swap
    assert all(a is b for a, b in zip(fused, list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1]]))
    assert g2d.native_body(False) is g2d
    assert all(a is b for a, b in zip(blocks, list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1]]))
    assert M.native_g2d_body(g2d, False) is False and list(g.state_dict().keys()) == before
    done = integration.install(g, eapp_tail=False, g2d_body=True)
    assert "G2d.body" in done and isinstance(g2d.res_blocks[0], M.ResBlock2DFused)
    assert "G2d.body" not in integration.install(gbase.Gbase(), eapp_tail=False)
    assert reenact.parse(["--random-init", "--source", "s", "--drivers", "d"]).native_g2d_body is False
    assert reenact.parse(["--random-init", "--source", "s", "--drivers", "d", "--native-g2d-body"]).native_g2d_body is True
