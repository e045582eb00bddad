"""Host-side checks of gn_apply_pool_warp_kernel (csrc/warp.hip; no GPU): its resources, read from hipcc's kernel metadata
(tools/register_table.py), and that the change behind it left the ABI alone."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPW_VGPRS, GPW_LDS_BYTES = 218, 86272   # gn_apply_pool_warp_kernel, DESIGN.md section 3.5c (image 84672 B + channel table 1536 B + range reduction 64 B)


def test_kernel_resources():
    """512 threads, one workgroup per CU: two waves per SIMD may hold 256 registers each; the kernel keeps to what DESIGN.md records, so that
    the other batch's small kernels still fit beside it, and has no scratch — a spilled register in the channel walk is a round trip to
    memory per channel pair."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import register_table

    table = register_table.collect(["warp.hip"])
    kernels = {k["demangled"]: k for t in table.values() for k in t["kernels"]}
    mine = [k for n, k in kernels.items() if "gn_apply_pool_warp_kernel" in n]
    assert len(mine) == 1, sorted(kernels)
    k = mine[0]
    assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, k
    assert k["max_flat_workgroup_size"] == 512 and k["vgpr_count"] == GPW_VGPRS and k["group_segment_fixed_size"] == GPW_LDS_BYTES, k
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"{GPW_VGPRS} registers, {GPW_LDS_BYTES} B of LDS, no scratch" in design   # section 3.5c states what is pinned here


def test_no_new_entry_point():
    """The launch is reached through mphip_hot_slice_forward only: nothing in include/mphip.h names it and the ABI version stands."""
    header = open(os.path.join(ROOT, "include", "mphip.h")).read()
    assert "pool_warp" not in header and "RESIDUAL_FROM_WARP" not in header
    assert int(re.search(r"#define\s+MPHIP_ABI_VERSION\s+(\d+)", header).group(1)) >= 25
