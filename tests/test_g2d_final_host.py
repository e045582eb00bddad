"""Host-side checks of the fused G2d exit (no GPU): exported symbols, ABI version, module plumbing, workspace query."""
import os
import sys

import torch
import torch.nn as nn

from megaportrait_hack_amd import _lib, encoders2d as E, gbase, model as M


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ("mphip_g2d_final_workspace_bytes", "mphip_g2d_final_fwd", "mphip_g2d_final_bwd"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() >= 17     # the entries exist since ABI 17


def test_module_constructs_on_the_cpu():
    m = M.G2dFinalConv()
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"0.weight": (64,), "0.bias": (64,), "2.weight": (3, 64, 3, 3), "2.bias": (3,)}
    kinds = [type(c) for c in m]
    assert kinds == [nn.GroupNorm, nn.ReLU, nn.Conv2d, nn.Sigmoid] and m[0].num_groups == 32 and m[2].padding == (1, 1)
    assert isinstance(m, nn.Sequential) and M.model_dtype(m) == torch.float32
    ref = nn.Sequential(nn.GroupNorm(32, 64), nn.ReLU(inplace=True), nn.Conv2d(64, 3, 3, padding=1), nn.Sigmoid())
    assert list(ref.state_dict().keys()) == list(sd.keys())
    shared = M.G2dFinalConv.from_sequential(ref)
    assert all(a is b for a, b in zip(shared.parameters(), ref.parameters()))


def test_switch_is_off_by_default_and_leaves_the_keys_alone():
    g2d = E.G2d()
    assert type(g2d.final_conv) is nn.Sequential
    g = gbase.Gbase(G2d=g2d)
    before = list(g.state_dict().keys())
    assert len(before) == 971        # the manifest tests/test_gbase.py checks name by name
    modules = [n for n, _ in g.named_modules()]
    original, params = g2d.final_conv, list(g.parameters())
    g.native_final_conv()
    assert isinstance(g.G2d.final_conv, M.G2dFinalConv) and list(g.state_dict().keys()) == before
    assert all(a is b for a, b in zip(g.parameters(), params))
    g.native_final_conv(False)
    assert g.G2d.final_conv is original and list(g.state_dict().keys()) == before
    assert [n for n, _ in g.named_modules()] == modules


def test_workspace_query():
    lib = _lib.load()
    q = lib.mphip_g2d_final_workspace_bytes
    fwd = [q(n, 64, 512, 512, 32, 0) for n in (1, 2, 4, 8)]
    bwd = [q(n, 64, 512, 512, 32, 1) for n in (1, 2, 4, 8)]
    assert all(a > 0 for a in fwd) and fwd == sorted(fwd) and len(set(fwd)) == 4
    assert bwd == sorted(bwd) and len(set(bwd)) == 4 and all(b > f for b, f in zip(bwd, fwd))
    assert bwd[0] >= 2 * 64 * 512 * 512 * 4          # the activated map and its gradient, fp32
    assert q(1, 48, 8, 8, 32, 0) == 0 and q(1, 64, 8, 8, 5, 0) == 0 and q(0, 64, 8, 8, 32, 0) == 0


def test_kernels_are_in_the_register_table_without_scratch():
    """tools/register_table.py lists the new kernels; none of them touches scratch memory or spills."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import register_table

    kernels = register_table.collect(["g2d_final.hip"])["g2d_final.hip"]["kernels"]
    names = {k["demangled"].split("<")[0] for k in kernels}
    assert names == {"gf_stats_partial_kernel", "gf_fwd_kernel", "gf_bwd_kernel", "gf_fold_kernel"}
    assert sum(k["demangled"].startswith("gf_fwd_kernel") for k in kernels) == 9      # one template over (input dtype, output dtype)
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["group_segment_fixed_size"] <= 40 * 1024, k
