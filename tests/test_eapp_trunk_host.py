"""Host-side checks of the two-source 3x3 conv and of Eapp's fused 2-D trunk (no GPU): exported symbols (mphip_conv2d_cat_supported,
mphip_conv2d_cat_workspace_bytes, mphip_conv2d_cat_fwd), ABI version, size queries, argument refusals, the register table, module
matching, the weight fold (the identity the kernel relies on), the switches and the reference fixture."""
import copy
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, integration, model as M, reenact

ENTRIES = ("mphip_conv2d_cat_supported", "mphip_conv2d_cat_workspace_bytes", "mphip_conv2d_cat_fwd")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eapp_trunk.npz")


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 20     # the entries exist since ABI 20
    assert lib.mphip_build_flags() == 0


def test_shape_and_size_queries():
    lib = _lib.load()
    one = 4100 * 4                                                                  # MPHIP_RANGE_FLOATS floats: one descriptor
    # (N, C1, C2, Co, H, W): the six launches of Eapp's trunk at 512x512 with B = 8, and small ones
    for ok in [(8, 64, 0, 128, 512, 512), (8, 128, 64, 128, 512, 512), (8, 128, 0, 256, 256, 256), (8, 256, 128, 256, 256, 256),
               (8, 256, 0, 512, 128, 128), (8, 512, 256, 512, 128, 128), (1, 16, 0, 32, 1, 1), (2, 16, 32, 64, 1, 1), (3, 48, 16, 96, 13, 19)]:
        assert lib.mphip_conv2d_cat_supported(*ok) == 1 and lib.mphip_conv2d_cat_workspace_bytes(*ok) == 2 * one, ok
        assert lib.mphip_conv2d_supported(ok[0], ok[1] + ok[2], *ok[3:]) == 1                     # the concatenation's own rule
    for bad in [(1, 8, 0, 32, 8, 8), (1, 16, 8, 32, 8, 8), (1, 16, 24, 32, 8, 8), (1, 16, -16, 32, 8, 8), (1, 0, 16, 32, 8, 8),
                (1, 16, 16, 48, 8, 8), (1, 16, 16, 16, 8, 8), (0, 16, 16, 32, 8, 8), (1, 16, 16, 32, 0, 8), (1, 16, 16, 32, 8, -1),
                (64, 256, 256, 512, 512, 512)]:
        assert lib.mphip_conv2d_cat_supported(*bad) == 0 and lib.mphip_conv2d_cat_workspace_bytes(*bad) == 0, bad


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, r = (ctypes.c_void_p(base + i * 16384) for i in range(3))                 # three disjoint 16 KiB regions: x1, x2, y

    def fwd(n=1, c1=16, c2=16, co=32, h=4, w=4, x1=p, a1=None, r1=p, x2=q, a2=None, r2=q, wp=p, b=p, res=None, y=r, ws=p, wsb=1 << 20):
        return lib.mphip_conv2d_cat_fwd(x1, a1, 1, r1, c1, x2, a2, 0, r2, c2, wp, b, res, y, None, n, co, h, w, 0, ws, wsb, None)

    err = lib.mphip_last_error
    for missing in ("x1", "wp", "b", "y"):
        assert fwd(**{missing: None}) == -1 and b"null pointer" in err()
    assert fwd(x2=None) == -1 and b"second source" in err()                          # C2 without x2 ...
    assert fwd(c2=0) == -1 and b"second source" in err()                             # ... and x2 without C2
    for bad in (dict(c1=8), dict(c2=24), dict(co=48), dict(h=0), dict(n=0)):
        assert fwd(**bad) == -1 and b"unsupported shape" in err(), bad
    assert fwd(a1=p, r1=None) == -1 and b"affine1 without x1_range" in err()         # a table needs its descriptor
    assert fwd(a2=p, r2=None) == -1 and b"affine2 without" in err()
    assert fwd(c2=0, x2=None, a2=p, r2=p) == -1 and b"affine2 without" in err()      # ... and its source
    for alias in (dict(y=p), dict(y=q), dict(y=ctypes.c_void_p(q.value + 64)), dict(res=r)):
        assert fwd(**alias) == -1 and b"must not alias" in err(), alias
    assert fwd(x1=ctypes.c_void_p(p.value + 2)) == -1 and b"aligned" in err()
    assert fwd(wp=ctypes.c_void_p(p.value + 4)) == -1 and b"aligned" in err()
    assert fwd(r1=None, wsb=4100 * 4 - 1) == -3 and b"workspace" in err()            # one source to scan: one descriptor
    assert fwd(r1=None, r2=None, wsb=2 * 4100 * 4 - 1) == -3 and fwd(r1=None, ws=None, wsb=0) == -3


def test_kernels_are_in_the_register_table_within_budget():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import register_table

    kernels = register_table.collect(["conv2d_gn_f16x3.hip"])["conv2d_gn_f16x3.hip"]["kernels"]
    names = {k["demangled"].split("<")[0].split("(")[0] for k in kernels}
    assert names == {"conv2d_k3_cat_f16x3_kernel"}
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, k
        assert k["group_segment_fixed_size"] <= 80 * 1024, k                          # two workgroups per CU (160 KiB of LDS)


class _RefLayout(nn.Module):
    """The attribute layout of the reference's own ResBlock_Custom (model.py:88-107): qualifies by its attributes alone."""

    def __init__(self, dimension=2, ci=32, co=64):
        super().__init__()

        class Conv2d_WS(nn.Conv2d):
            pass

        self.dimension, self.in_channels, self.out_channels = dimension, ci, co
        self.conv_res = nn.Conv2d(ci, co, 3, padding=1)
        self.conv_ws = Conv2d_WS(in_channels=ci, out_channels=co, kernel_size=3, padding=1)
        self.conv = nn.Conv2d(co, co, 3, padding=1)


def test_matches_accepts_and_rejects_the_right_modules():
    ok = M.ResBlockCustomFused.matches
    assert ok(E.ResBlock_Custom(2, 32, 64)) and ok(E.ResBlock_Custom(2, 64, 64)) and ok(_RefLayout())
    assert not ok(M.ResBlockCustomFused(2, 32, 64)) and not ok(nn.Conv2d(3, 3, 3)) and not ok(None) and not ok(E.ResBlock2D(32, 32))
    assert not ok(_RefLayout(dimension=3))

    def broken(edit):
        b = E.ResBlock_Custom(2, 32, 64)
        edit(b)
        return b

    assert not ok(broken(lambda b: setattr(b, "dimension", 3)))
    assert not ok(broken(lambda b: setattr(b, "conv", nn.Conv2d(64, 64, 3, padding=1, bias=False))))          # a bias-free conv
    assert not ok(broken(lambda b: setattr(b, "conv_res", nn.Conv2d(32, 64, 3, padding=1, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv_ws", nn.Conv2d(32, 64, 3, padding=1))))                  # a plain conv as conv_ws
    assert not ok(broken(lambda b: setattr(b, "conv_ws", E.Conv2d_WS(32, 64, 3, padding=1, bias=False))))
    assert not ok(broken(lambda b: setattr(b, "conv", nn.Conv2d(64, 64, 3, stride=2, padding=1))))
    assert not ok(broken(lambda b: setattr(b, "conv_res", nn.Conv2d(32, 64, 5, padding=2))))
    assert not ok(broken(lambda b: setattr(b, "conv", nn.Conv2d(64, 64, 3, padding=0))))
    assert not ok(broken(lambda b: setattr(b, "conv", nn.Conv2d(64, 32, 3, padding=1))))
    assert not ok(broken(lambda b: setattr(b, "conv_res", nn.Conv2d(16, 64, 3, padding=1))))
    try:
        M.ResBlockCustomFused.from_block(E.ResBlock2D(32, 32))
        assert False
    except TypeError:
        pass


def test_fold_reproduces_the_block_in_fp64():
    """conv(a) + conv_res(x) == one conv over [a ; x] with [W_conv | W_res] and b_conv + b_res, and the standardised weight is
    Conv2d_WS.forward's: what the two launches of the native path compute."""
    torch.manual_seed(0)
    blk = E.ResBlock_Custom(2, 32, 64).double()
    x = torch.randn(2, 32, 7, 9, dtype=torch.float64) - 1.0
    with torch.no_grad():
        want = blk(x)
        (w_ws, b_ws), (w_cat, b_cat) = M.fold_resblock_custom(blk.conv_res, blk.conv_ws, blk.conv)
        assert w_ws.dtype == torch.float64 and not w_cat.requires_grad
        assert tuple(w_ws.shape) == (64, 32, 3, 3) and tuple(w_cat.shape) == (64, 96, 3, 3) and tuple(b_cat.shape) == (64,)
        assert torch.equal(w_cat[:, :64], blk.conv.weight) and torch.equal(w_cat[:, 64:], blk.conv_res.weight)
        assert torch.equal(b_cat, blk.conv.bias + blk.conv_res.bias)
        t = blk.conv_ws(F.relu(F.group_norm(x, 32)))                                 # by the block itself
        assert (F.conv2d(F.relu(F.group_norm(x, 32)), w_ws, b_ws, padding=1) - t).abs().max().item() <= 1e-12 * t.abs().max().item()
        got = F.conv2d(torch.cat([F.relu(F.group_norm(t, 32)), x], 1), w_cat, b_cat, padding=1)
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def test_fused_block_shares_the_block_and_falls_back_on_the_cpu_expression():
    blk = E.ResBlock_Custom(2, 32, 64)
    fused = M.ResBlockCustomFused.from_block(blk)
    assert list(fused.state_dict().keys()) == list(blk.state_dict().keys())
    assert all(a is b for a, b in zip(fused.parameters(), blk.parameters()))
    assert list(M.ResBlockCustomFused(2, 32, 64).state_dict().keys()) == list(blk.state_dict().keys())
    assert (fused.dimension, fused.in_channels, fused.out_channels) == (2, 32, 64)
    x = torch.randn(2, 32, 5, 7)
    assert not fused._native_ok(x)
    y = fused(x)
    assert torch.equal(y, blk(x)) and y.requires_grad and "_mphip_fold" not in fused.__dict__      # the original PyTorch expression
    with torch.no_grad():
        assert not fused._native_ok(x) and torch.equal(fused(x), blk(x))                            # a CPU map has no HIP path


def test_switches_are_off_by_default_and_leave_the_keys_alone():
    eapp = E.Eapp()
    slots = lambda: [eapp.resblock_128, eapp.resblock_256, eapp.resblock_512]
    blocks = slots()
    assert all(type(b) is E.ResBlock_Custom for b in blocks)
    g = gbase.Gbase(appearanceEncoder=eapp)
    before = list(g.state_dict().keys())
    assert len(before) == 971
    modules, params = [n for n, _ in g.named_modules()], list(g.parameters())
    assert g.native_trunk() is g
    fused = slots()
    assert all(isinstance(b, M.ResBlockCustomFused) for b in fused) and isinstance(eapp.conv, nn.Conv2d)
    assert list(g.state_dict().keys()) == before and all(a is b for a, b in zip(g.parameters(), params))
    assert [n for n, _ in g.named_modules()] == modules
    assert M.native_eapp_trunk(eapp, True) is False                  # twice: nothing left to swap
    assert all(a is b for a, b in zip(fused, slots()))
    x = torch.rand(1, 3, 16, 16)
    y = eapp.trunk2d(x)                                              # on the CPU: the fallback expression
    assert eapp.native_trunk(False) is eapp
    assert all(a is b for a, b in zip(blocks, slots())) and torch.equal(eapp.trunk2d(x), y)
    assert M.native_eapp_trunk(eapp, False) is False and list(g.state_dict().keys()) == before
    done = integration.install(g, eapp_tail=False, eapp_trunk=True)
    assert "Eapp.trunk2d" in done and isinstance(eapp.resblock_128, M.ResBlockCustomFused)
    assert "Eapp.trunk2d" not in integration.install(gbase.Gbase(), eapp_tail=False)
    assert reenact.parse(["--random-init", "--source", "s", "--drivers", "d"]).native_eapp_trunk is False
    assert reenact.parse(["--random-init", "--source", "s", "--drivers", "d", "--native-eapp-trunk"]).native_eapp_trunk is True


def test_golden_is_reproduced_by_this_packages_block():
    gold = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1 << 20
    blk = E.ResBlock_Custom(2, 32, 64)
    assert sorted(k for k in gold.files if k not in ("x", "y32", "y64")) == sorted(blk.state_dict().keys())
    blk.load_state_dict({k: torch.from_numpy(gold[k]) for k in blk.state_dict()})
    x, y32, y64 = (torch.from_numpy(gold[k]) for k in ("x", "y32", "y64"))
    assert tuple(x.shape) == (2, 32, 12, 20) and tuple(y32.shape) == tuple(y64.shape) == (2, 64, 12, 20) and y64.dtype == torch.float64
    shifts = -x.mean(dim=(2, 3)) / x.var(dim=(2, 3), unbiased=False).add(1e-5).sqrt()
    assert (shifts > 0).float().mean().item() >= 0.75                # the case in which a normalised padded zero would show
    with torch.no_grad():
        y = blk(x)
        e_ref32 = (y32.double() - y64).abs().max().item()
        floor = 2.0 ** -22 * y64.abs().max().item()
        assert (y.double() - y64).abs().max().item() <= 4 * e_ref32 + floor
        assert (copy.deepcopy(blk).double()(x.double()) - y64).abs().max().item() <= 1e-12 * y64.abs().max().item()
