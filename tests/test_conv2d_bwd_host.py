"""CPU tests of the 2-D conv backward (csrc/conv2d_bwd_f16x3.hip, ABI 30): the exports, the host-side queries against their stated
rules, the refusals that come before the first HIP call, the register table of the new unit, the claims of the GPU file's tables, and
the mechanics of the `trainable` switch on CPU modules."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import test_gpu_conv2d_bwd as gpu  # noqa: E402

NEW = ["mphip_conv2d_bwd_weight_supported", "mphip_conv2d_bwd_weight_workspace_bytes", "mphip_conv2d_bwd_weight",
       "mphip_pack_conv2d_weight_bwd_data", "mphip_debug_conv2d_bwd_weight_plan"]
CHANNELS = [8, 16, 24, 32, 48, 64, 80, 96, 128, 160, 256, 512]
MAPS = [(1, 1, 1), (3, 1, 1), (1, 1, 24), (2, 5, 3), (1, 8, 8), (1, 9, 16), (2, 12, 20), (1, 40, 72), (2, 24, 56), (1, 64, 64), (4, 64, 64),
        (1, 512, 512), (8, 128, 128), (1, 8192, 4096), (1, 8192, 8192), (1, 46341, 46341), (0, 8, 8), (1, 0, 8), (1, 8, -1)]
EINVAL, EWORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib():
    from megaportrait_hack_amd import _lib

    return _lib.load()


def rule_supported(n, ci, co, h, w):
    """the forward's rule (include/mphip.h): Ci % 16 == 0, Co % 32 == 0, N, H, W >= 1, fewer than 2^31 elements per tensor, and at most
    65535 output-channel tiles of 64 (the forward's grid)"""
    if n < 1 or h < 1 or w < 1 or ci < 16 or co < 32 or ci % 16 or co % 32 or (co + 63) // 64 > 65535:
        return False
    return h * w < 2 ** 31 and n * ci * h * w < 2 ** 31 and n * co * h * w < 2 ** 31


def rule_plan(n, ci, co, h, w):
    """8 x 8 pixel tiles per sample; (64 x 64 channel blocks) x splits fills 512 workgroups"""
    if not rule_supported(n, ci, co, h, w):
        return (0, 0, 0, 0)
    ntiles = n * ((h + 7) // 8) * ((w + 7) // 8)
    bxy = ((ci + 63) // 64) * ((co + 63) // 64)
    sp = min(max(1, 512 // bxy), ntiles)
    tps = (ntiles + sp - 1) // sp
    return (1 if w % 8 == 0 else 2, (ntiles + tps - 1) // tps, tps, ntiles)


def test_exports_and_abi(lib):
    from megaportrait_hack_amd import _lib

    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "mphip.h")) as f:
        header = f.read()
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() == 30
    assert int(re.search(r"#define\s+MPHIP_ABI_VERSION\s+(\d+)", header).group(1)) == 30
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name


def test_queries_agree_with_the_stated_rules(lib):
    from megaportrait_hack_amd import ops

    seen = {0: 0, 1: 0, 2: 0}
    for ci in CHANNELS:
        for co in CHANNELS:
            pack_t = lib.mphip_conv2d_packed_weight_bytes(ci, co)       # the transposed pack of a [co, ci, 3, 3] weight
            assert (pack_t != 0) == (co % 16 == 0 and ci % 32 == 0 and ci >= 32), (ci, co, pack_t)
            if pack_t:
                assert pack_t == 16 + ((ci + 63) // 64) * (co // 16) * 18432 * 2
            for n, h, w in MAPS:
                shape = (n, ci, co, h, w)
                ok = rule_supported(*shape)
                plan = gpu.bwd_plan(lib, shape)
                seen[plan[0]] += 1
                assert lib.mphip_conv2d_bwd_weight_supported(*shape) == int(ok), shape
                assert plan == rule_plan(*shape), (shape, plan)
                ws = lib.mphip_conv2d_bwd_weight_workspace_bytes(*shape)
                assert ws == (gpu.WS_HEAD + plan[1] * co * ci * 9 * 4 if ok else 0), (shape, ws)
                assert ops.conv2d_bwd_weight_supported(*shape) == ok
                assert ops.conv2d_bwd_supported(*shape, False) == ok
                assert ops.conv2d_bwd_supported(*shape, True) == (ok and pack_t != 0 and rule_supported(n, co, ci, h, w)), shape
    assert all(v > 50 for v in seen.values()), seen
    # the cases the rules name
    assert not rule_supported(1, 8, 32, 8, 8) and not rule_supported(1, 24, 32, 8, 8) and not rule_supported(1, 16, 16, 8, 8)
    assert ops.conv2d_bwd_supported(1, 16, 32, 8, 8, False) and not ops.conv2d_bwd_supported(1, 16, 32, 8, 8, True)
    assert rule_supported(3, 16, 32, 1, 1) and rule_supported(1, 16, 32, 8192, 4096)
    assert not rule_supported(1, 16, 32, 8192, 8192) and not rule_supported(1, 16, 32, 46341, 46341)
    assert gpu.bwd_plan(lib, (1, 64, 64, 512, 512)) == (1, 512, 8, 4096)       # one channel block: the split fills the part
    assert gpu.bwd_plan(lib, (1, 512, 512, 64, 64)) == (1, 8, 8, 64)
    assert lib.mphip_debug_conv2d_bwd_weight_plan(1, 16, 32, 8, 8, None) == 0


def test_refusals_come_before_the_first_hip_call(lib):
    """fake (never dereferenced) pointers: every refusal is decided on the host"""
    p, off = 4096, 4096 + 4
    shape = (1, 16, 32, 8, 8)
    need = lib.mphip_conv2d_bwd_weight_workspace_bytes(*shape)
    assert need == gpu.WS_HEAD + 32 * 16 * 9 * 4
    err = lambda: lib.mphip_last_error().decode()
    for args in ((None, None, p, p, p), (p, None, None, p, p), (p, None, p, None, p), (p, None, p, p, None)):
        assert lib.mphip_conv2d_bwd_weight(*args, *shape, p, need, None) == EINVAL and "null pointer" in err()
    assert lib.mphip_conv2d_bwd_weight(p, None, p, p, p, 1, 24, 32, 8, 8, p, 1 << 30, None) == EINVAL and "unsupported shape" in err()
    assert lib.mphip_conv2d_bwd_weight(p, None, p, p, p, *shape, None, need, None) == EWORKSPACE
    assert lib.mphip_conv2d_bwd_weight(p, None, p, p, p, *shape, p, need - 1, None) == EWORKSPACE and f"required {need}" in err()
    assert lib.mphip_conv2d_bwd_weight(p, p, p, p, p, *shape, p, 0, None) == EWORKSPACE       # (the slabs: a given x_range does not lift it)
    assert lib.mphip_conv2d_bwd_weight(off, None, p, p, p, *shape, p, need, None) == EINVAL and "16-byte aligned" in err()
    assert lib.mphip_conv2d_bwd_weight(p, None, off, p, p, *shape, p, need, None) == EINVAL and "16-byte aligned" in err()
    assert lib.mphip_conv2d_bwd_weight(p + 2, None, p, p, p, 1, 16, 32, 8, 5, p, 1 << 30, None) == EINVAL and "4-byte aligned" in err()
    assert lib.mphip_pack_conv2d_weight_bwd_data(None, p, 32, 32, None) == EINVAL and "null pointer" in err()
    assert lib.mphip_pack_conv2d_weight_bwd_data(p, p, 32, 16, None) == EINVAL and "roles swap" in err()     # Ci = 16: no transposed pack
    assert lib.mphip_pack_conv2d_weight_bwd_data(p, p, 24, 32, None) == EINVAL                               # Co = 24
    assert lib.mphip_pack_conv2d_weight_bwd_data(p, p + 4, 32, 32, None) == EINVAL and "16-byte aligned" in err()


def test_the_new_unit_uses_no_scratch():
    import register_table

    kernels = register_table.collect(["conv2d_bwd_f16x3.hip"])["conv2d_bwd_f16x3.hip"]["kernels"]
    names = sorted(k["demangled"] for k in kernels)
    assert names == ["conv2d_bwd_slab_reduce_kernel", "conv2d_bwd_weight_f16x3_kernel<0>", "conv2d_bwd_weight_f16x3_kernel<1>"], names
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
        if k["demangled"].startswith("conv2d_bwd_weight"):     # two workgroups per CU: 256 registers a lane, 50 KB of LDS
            assert k["vgpr_count"] + k["agpr_count"] <= 256 and k["group_segment_fixed_size"] <= 80 * 1024, k


def test_gpu_cases_claim_the_plan_the_library_reports(lib):
    """the claims of the GPU file's tables, checked here without a GPU; between them the integer cases reach every edge"""
    for row in gpu.INT_CASES + gpu.ROUNDING_CASES + [gpu.MAGNITUDE_CASE]:
        gpu.claim_holds(lib, row)
    for shape in gpu.OUTSIDE_CASES:
        assert gpu.bwd_plan(lib, shape) == (0, 0, 0, 0) and not rule_supported(*shape)
    claimed = {e for row in gpu.INT_CASES for e in row[2]}
    assert claimed >= {"ci%64", "co%64", "ci+16", "co+32", "ragged-h", "ragged-w", "w<8", "h1", "w1", "cols1", "cols2", "cols3", "tps>1",
                       "uneven-last", "cross-sample", "single"}
    assert {gpu.bwd_plan(lib, row[0])[0] for row in gpu.INT_CASES} == {gpu.VEC, gpu.MASKED}
    assert gpu.MAGNITUDE_CASE[0][0] * gpu.MAGNITUDE_CASE[0][3] * gpu.MAGNITUDE_CASE[0][4] == 128
    assert sum(s[1] >= 128 for s, _ in gpu.ROUNDING_CASES) >= 1 and any(p[2] > 1 for _, p in gpu.ROUNDING_CASES)


def test_switch_mechanics_on_cpu_modules():
    import inspect

    from megaportrait_hack_amd import encoders2d as E, gbase, model as M

    for fn in (M.ResBlock2DFused.from_block, M.native_g2d_body, E.G2d.native_body, gbase.Gbase.native_body):
        assert inspect.signature(fn).parameters["trainable"].default is False, fn
    g2d = E.G2d().eval()
    keys = list(g2d.state_dict().keys())
    slots = lambda: list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1], g2d.upsample1, g2d.upsample2, g2d.upsample3]
    originals = slots()
    assert g2d.native_body() is g2d                                            # the default: no attribute left behind
    assert all(isinstance(b, M.ResBlock2DFused) and "_mphip_trainable" not in b.__dict__ for b in slots()[:11])
    assert M.native_g2d_body(g2d, True, trainable=True) is True and M.native_g2d_body(g2d, True, trainable=True) is False
    assert all(b.__dict__.get("_mphip_trainable") is True for b in slots()[:11])
    assert list(g2d.state_dict().keys()) == keys
    x = torch.randn(1, 512, 2, 2, requires_grad=True)                          # a CPU map: the PyTorch expression, whatever the flag
    assert not g2d.res_blocks[0]._trainable_ok(x) and torch.equal(g2d.res_blocks[0](x), originals[0](x))
    assert M.native_g2d_body(g2d, True) is True                                # fused already: the keyword's value is taken, here off
    assert all("_mphip_trainable" not in b.__dict__ for b in slots()[:11])
    g2d.native_body(trainable=True, fuse_upsample=True)                        # the stages' blocks get the flag too
    assert all("_mphip_trainable" in b.__dict__ for b in slots()[:11])
    assert all(isinstance(s, M.Up2ResBlock2DFused) for s in slots()[11:]) and list(g2d.state_dict().keys()) == keys
    g2d.native_body(False)
    assert all(a is b for a, b in zip(originals, slots())) and list(g2d.state_dict().keys()) == keys
    blk = E.ResBlock2D(32, 64)
    fused = M.ResBlock2DFused.from_block(blk, trainable=True)
    assert fused.__dict__["_mphip_trainable"] is True and fused.conv1 is blk.conv1 and list(fused.state_dict()) == list(blk.state_dict())
    for conv in (blk.conv1, blk.conv2):                                        # what a train-mode call leaves on the shared convs
        conv.__dict__["_mphip_pack2d"] = conv.__dict__["_mphip_bwd_pack2d"] = object()
    fused.__dict__["_mphip_fold_bwd"] = object()
    assert M._set_trainable(fused, False) and not M._set_trainable(fused, False) and "_mphip_trainable" not in fused.__dict__
    assert not any(k.startswith("_mphip") for m in (fused, blk.conv1, blk.conv2) for k in m.__dict__)      # nothing left behind
    swapped = torch.nn.Sequential(E.ResBlock2D(32, 32))                        # ... and the same when the switch puts the block back
    orig = swapped[0]
    new, did = M._swap_slot(M.ResBlock2DFused, orig, True, False, True)
    orig.conv1.__dict__["_mphip_pack2d"] = orig.conv2.__dict__["_mphip_bwd_pack2d"] = object()
    back, did = M._swap_slot(M.ResBlock2DFused, new, False, False, False)
    assert back is orig and did and not any(k.startswith("_mphip") for m in (orig.conv1, orig.conv2) for k in m.__dict__)
    w, b = M.fold_batchnorm_autograd(blk.conv1, blk.bn1)                       # the differentiable fold: fold_batchnorm's bits
    w0, b0 = M.fold_batchnorm(blk.conv1, blk.bn1)
    assert torch.equal(w.detach(), w0) and torch.equal(b.detach(), b0) and w.requires_grad and b.requires_grad
    g = gbase.Gbase(G2d=g2d)
    assert g.native_body(trainable=True) is g and "_mphip_trainable" in g.G2d.res_blocks[0].__dict__
    g.native_body(False)
    assert all(a is b for a, b in zip(originals, slots()))
