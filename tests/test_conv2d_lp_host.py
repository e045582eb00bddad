"""Host-side checks of the typed, one-product form of the 2-D 3x3 convs (csrc/conv2d_lp.hip) and of the `half_precision` keyword of the
fused 2-D blocks (no GPU): exported symbols (mphip_conv2d_typed_supported, mphip_conv2d_fwd_typed, mphip_conv2d_cat_fwd_typed), ABI
version, the table of built combinations, every refusal, the register table of the new unit, and that nothing changes with the keyword
left out."""
import ctypes
import os
import sys

import torch
import torch.nn as nn

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, integration, model as M, reenact

ENTRIES = ("mphip_conv2d_typed_supported", "mphip_conv2d_fwd_typed", "mphip_conv2d_cat_fwd_typed")
F32, F16, BF16 = 0, 1, 2


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 21     # the entries exist since ABI 21
    assert lib.mphip_build_flags() == 0


def test_table_of_built_combinations():
    """One product: plain form x any -> y fp32 and x fp32 -> y any, two-source form fp32 sources -> y any; three products: fp32 only.
    The residual is fp32 or in y's dtype; one half dtype per call."""
    ok = _lib.load().mphip_conv2d_typed_supported
    for y in (F32, F16, BF16):
        for r in {F32, y}:
            assert ok(0, F32, r, y, 1) == 1 and ok(1, F32, r, y, 1) == 1, (r, y)
            assert ok(0, F32, r, y, 3) == (1 if y == F32 else 0) and ok(1, F32, r, y, 3) == (1 if y == F32 else 0)
    for x in (F16, BF16):
        assert ok(0, x, F32, F32, 1) == 1 and ok(0, x, F32, F32, 3) == 0
        assert ok(0, x, F32, x, 1) == 0 and ok(0, x, x, x, 1) == 0                   # not built: no block launches it
        assert ok(1, x, F32, F32, 1) == 0 and ok(1, x, F32, x, 1) == 0               # the two-source form reads fp32 sources
    assert ok(0, F32, F16, F32, 1) == 0 and ok(0, F32, BF16, F16, 1) == 0 and ok(0, F16, F32, BF16, 1) == 0
    assert ok(0, 3, F32, F32, 1) == 0 and ok(0, F32, -1, F32, 1) == 0 and ok(0, F32, F32, 7, 1) == 0
    assert ok(0, F32, F32, F32, 2) == 0 and ok(0, F32, F32, F32, -1) == 0 and ok(0, F32, F32, F32, 4) == 0
    prev = _lib.load().mphip_conv3d_set_half_products(0)
    try:
        assert ok(0, F32, F32, F16, 0) == 0 and ok(0, F32, F32, F32, 0) == 1         # 0 follows the thread's flag: three products
        _lib.load().mphip_conv3d_set_half_products(1)
        assert ok(0, F32, F32, F16, 0) == 1 and ok(0, F16, F32, F32, 0) == 1         # ... one product
    finally:
        _lib.load().mphip_conv3d_set_half_products(prev)


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, r = (ctypes.c_void_p(base + i * 16384) for i in range(3))                 # three disjoint 16 KiB regions
    err = lib.mphip_last_error

    def fwd(xd=F32, rd=F32, yd=F32, products=1, n=1, ci=16, co=32, h=4, w=4, x=p, wp=p, b=p, res=None, y=r, ws=p, wsb=1 << 20):
        return lib.mphip_conv2d_fwd_typed(x, xd, None, wp, b, res, rd, y, yd, None, n, ci, co, h, w, 0, products, ws, wsb, None)

    def cat(xd=F32, rd=F32, yd=F32, products=1, n=1, c1=16, c2=16, co=32, h=4, w=4, x1=p, x2=q, wp=p, b=p, res=None, y=r, ws=p, wsb=1 << 20):
        return lib.mphip_conv2d_cat_fwd_typed(x1, xd, None, 1, p, c1, x2, None, 0, q, c2, wp, b, res, rd, y, yd, None, n, co, h, w, 0,
                                              products, ws, wsb, None)

    for call, name in ((fwd, b"conv2d_fwd_typed"), (cat, b"conv2d_cat_fwd_typed")):
        for bad in (dict(xd=3), dict(xd=-1), dict(rd=5), dict(yd=3), dict(yd=-2)):
            assert call(**bad) == -1 and b"unknown" in err() and b"dtype" in err() and name in err(), bad
        for bad in (2, 4, -1, 30):
            assert call(products=bad) == -1 and b"products" in err() and name in err(), bad
        for bad in (dict(rd=F16, yd=BF16), dict(rd=BF16, yd=F16)):
            assert call(**bad) == -1 and b"two different half dtypes" in err(), bad
        assert call(rd=F16, yd=F32) == -1 and b"residual_dtype" in err()             # fp32 or the dtype of y
        assert call(yd=F16, products=3) == -1 and b"no kernel" in err()              # three products: fp32 maps only
    assert fwd(xd=F16, yd=BF16) == -1 and b"two different half dtypes" in err()
    assert fwd(xd=F16, yd=F16) == -1 and b"no kernel" in err()
    for xd in (F16, BF16):
        assert cat(xd=xd) == -1 and b"typed source" in err()
        assert cat(xd=xd, yd=xd) == -1 and b"typed source" in err()
    # the shape, pointer and workspace rules of the fp32 entries hold for the one-product kernels ...
    for missing in ("x", "wp", "b", "y"):
        assert fwd(**{missing: None}) == -1 and b"null pointer" in err()
    for missing in ("x1", "wp", "b", "y"):
        assert cat(**{missing: None}) == -1 and b"null pointer" in err()
    for bad in (dict(ci=8), dict(co=48), dict(h=0), dict(n=0)):
        assert fwd(**bad) == -1 and b"unsupported shape" in err(), bad
    for bad in (dict(c1=8), dict(c2=24), dict(co=48), dict(h=0), dict(n=0)):
        assert cat(**bad) == -1 and b"unsupported shape" in err(), bad
    assert cat(x2=None) == -1 and b"second source" in err()
    assert fwd(xd=F16, x=ctypes.c_void_p(p.value + 1)) == -1 and b"aligned" in err()
    assert fwd(x=ctypes.c_void_p(p.value + 2)) == -1 and b"aligned" in err()
    assert fwd(yd=F16, y=ctypes.c_void_p(r.value + 1)) == -1 and b"aligned" in err()
    assert fwd(xd=F16, x=ctypes.c_void_p(p.value + 2), wsb=0) == -3                   # a 2-byte aligned half map is fine: next rule
    for alias in (dict(y=p), dict(res=r), dict(yd=F16, rd=F16, res=ctypes.c_void_p(r.value + 64))):
        assert fwd(**alias) == -1 and b"must not alias" in err(), alias
    for alias in (dict(y=p), dict(y=q), dict(res=r)):
        assert cat(**alias) == -1 and b"must not alias" in err(), alias
    assert fwd(wsb=4100 * 4 - 1) == -3 and b"workspace" in err() and fwd(ws=None, wsb=0) == -3
    # ... and with fp32 maps and three products the typed entries are the fp32 entries, refusals included
    assert fwd(products=3, ci=8) == -1 and b"conv2d_fwd: unsupported shape" in err()
    assert cat(products=3, c1=8) == -1 and b"conv2d_cat_fwd: unsupported shape" in err()


def test_kernels_are_in_the_register_table_within_budget():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import register_table

    kernels = register_table.collect(["conv2d_lp.hip"])["conv2d_lp.hip"]["kernels"]
    names = {k["demangled"] for k in kernels}
    # <x dtype, y dtype, products> and, two-source, <y dtype, products>: what the table of built combinations promises, and no more
    assert names == {f"conv2d_k3_lp_kernel<{x}, {y}, 1>" for x, y in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2))} | \
        {f"conv2d_k3_cat_lp_kernel<{y}, 1>" for y in (0, 1, 2)}
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, k
        products = int(k["demangled"].rstrip(">").split(",")[-1])
        if products == 1:
            assert k["group_segment_fixed_size"] <= 29 * 1024, k          # hi planes only: a lo plane that is still staged cannot pass
        else:
            assert products == 3 and k["group_segment_fixed_size"] <= 80 * 1024, k
    # the kernel sets of the two fp32 units are pinned by tests/test_conv2d_host.py and tests/test_eapp_trunk_host.py


def test_keyword_left_out_builds_todays_objects():
    blk, cus = E.ResBlock2D(32, 64).eval(), E.ResBlock_Custom(2, 32, 64)
    for cls, b in ((M.ResBlock2DFused, blk), (M.ResBlockCustomFused, cus)):
        plain, off, on = cls.from_block(b), cls.from_block(b, half_precision=False), cls.from_block(b, half_precision=True)
        assert set(plain.__dict__) == set(off.__dict__) and "_mphip_half" not in plain.__dict__
        assert set(on.__dict__) - set(plain.__dict__) == {"_mphip_half"}
        for f in (plain, off, on):
            assert list(f.state_dict().keys()) == list(b.state_dict().keys())
            assert all(a is c for a, c in zip(f.parameters(), b.parameters())) and all(a is c for a, c in zip(f.buffers(), b.buffers()))
        x = torch.randn(2, 32, 5, 7)
        with torch.no_grad():
            assert on._half_out(x) is None                                      # a CPU map has no half-precision path
            if cls is M.ResBlockCustomFused:
                assert torch.equal(on(x), b(x))                                 # ... the PyTorch expression, as with the keyword off
            with torch.autocast("cpu", dtype=torch.bfloat16):
                assert on._half_out(x) is None
        assert on(x).requires_grad                                              # autograd: the PyTorch expression


def test_switches_are_off_by_default_and_leave_the_keys_alone():
    g2d, eapp = E.G2d(), E.Eapp()
    g = gbase.Gbase(G2d=g2d, appearanceEncoder=eapp)
    before = list(g.state_dict().keys())
    assert len(before) == 971        # the manifest tests/test_gbase.py checks name by name
    modules, params = [n for n, _ in g.named_modules()], list(g.parameters())
    body = lambda: list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1]]
    trunk = lambda: [eapp.resblock_128, eapp.resblock_256, eapp.resblock_512]
    originals = body() + trunk()
    flags = lambda: [b.__dict__.get("_mphip_half", False) for b in body() + trunk()]

    assert g.native_body() is g and g.native_trunk() is g and flags() == [False] * 14          # the keyword left out
    for on in (True, False):
        assert g.native_body(True, half_precision=on) is g and g.native_trunk(True, half_precision=on) is g
        assert flags() == [on] * 14                                                                 # fused blocks take the keyword's value
        assert all(isinstance(b, M.ResBlock2DFused) for b in body()) and all(isinstance(b, M.ResBlockCustomFused) for b in trunk())
        assert list(g.state_dict().keys()) == before and all(a is b for a, b in zip(g.parameters(), params))
        assert [n for n, _ in g.named_modules()] == modules
    assert M.native_g2d_body(g2d, True) is False and M.native_g2d_body(g2d, True, half_precision=True) is True
    assert M.native_g2d_body(g2d, True, half_precision=True) is False
    assert M.native_eapp_trunk(eapp, True, half_precision=True) is True and M.native_eapp_trunk(eapp, True, half_precision=True) is False
    assert g2d.native_body(False) is g2d and eapp.native_trunk(False) is eapp
    assert all(a is b for a, b in zip(originals, body() + trunk())) and list(g.state_dict().keys()) == before
    assert g2d.native_body(half_precision=True) is g2d and eapp.native_trunk(half_precision=True) is eapp and flags() == [True] * 14
    g.native_body(False), g.native_trunk(False)

    done = integration.install(g, eapp_tail=False, g2d_body=True, eapp_trunk=True)
    assert "G2d.body" in done and "Eapp.trunk2d" in done and flags() == [False] * 14
    g.native_body(False), g.native_trunk(False)
    done = integration.install(g, eapp_tail=False, g2d_body=True, eapp_trunk=True, half_precision=True)
    assert "G2d.body" in done and "Eapp.trunk2d" in done and flags() == [True] * 14
    assert list(g.state_dict().keys()) == before and all(a is b for a, b in zip(g.parameters(), params))
    assert integration.install(gbase.Gbase(), eapp_tail=False, half_precision=True) == integration.install(gbase.Gbase(), eapp_tail=False)

    base = ["--random-init", "--source", "s", "--drivers", "d"]
    assert reenact.parse(base).native_half_precision is False
    assert reenact.parse(base + ["--native-g2d-body"]).native_half_precision is False
    assert reenact.parse(base + ["--native-g2d-body", "--native-half-precision"]).native_half_precision is True


def test_half_fold_is_the_fp32_twins_fold():
    """A .half() block folds in fp32 from the widened parameters: what its fp32 twin (copy.deepcopy(block).float()) folds."""
    import copy

    torch.manual_seed(0)
    for dt in (torch.float16, torch.bfloat16):
        blk = E.ResBlock2D(16, 32).eval()
        with torch.no_grad():
            for m in blk.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.running_var.uniform_(0.5, 1.5), m.running_mean.normal_(), m.weight.normal_(), m.bias.normal_()
        blk = blk.to(dt)
        twin = copy.deepcopy(blk).float()
        for (c, b), (ct, bt) in (((blk.conv1, blk.bn1), (twin.conv1, twin.bn1)), ((blk.shortcut[0], blk.shortcut[1]), (twin.shortcut[0], twin.shortcut[1]))):
            w, bias = M.fold_batchnorm(c, b, torch.float32)
            wt, biast = M.fold_batchnorm(ct, bt)
            assert w.dtype == torch.float32 and torch.equal(w, wt) and torch.equal(bias, biast)
            assert M.fold_batchnorm(c, b)[0].dtype == dt                      # without the argument: the parameters' own dtype, as before
        cus = E.ResBlock_Custom(2, 32, 64).to(dt)
        tw = copy.deepcopy(cus).float()
        got = M.fold_resblock_custom(cus.conv_res, cus.conv_ws, cus.conv, torch.float32)
        want = M.fold_resblock_custom(tw.conv_res, tw.conv_ws, tw.conv)
        assert all(torch.equal(a, b) and a.dtype == torch.float32 for ga, wa in zip(got, want) for a, b in zip(ga, wa))
        assert M.fold_resblock_custom(cus.conv_res, cus.conv_ws, cus.conv)[0][0].dtype == dt
