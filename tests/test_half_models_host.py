"""CPU tests of the half-model support (include/mphip.h "model dtypes", ABI 15): the new entry points are exported, the reenact CLI's
--dtype option, the mixed-dtype refusal before anything is launched, and the fp32 K2/K3 kernels' resources left as they were."""
import ctypes
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")

NEW_SYMBOLS = ("mphip_warp_volume_typed", "mphip_warp_corner_image_typed", "mphip_warp_volume_coords_img_typed", "mphip_warp_volume_dsum_typed",
               "mphip_warp_volume_dsum_coords_typed", "mphip_cast_to_f32_range", "mphip_cast_from_f32", "mphip_hot_slice_forward_typed",
               "mphip_g3d_workspace_bytes_typed", "mphip_g3d_forward_typed")


@pytest.fixture(scope="module")
def lib():
    from megaportrait_hack_amd import _lib

    _lib.build()
    return _lib.load()


def test_typed_entry_points_are_exported(lib):
    from megaportrait_hack_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert lib.mphip_version() >= 15   # (the ABI that introduced them; later exports bump it)
    hdr = open(os.path.join(ROOT, "include", "mphip.h")).read()
    for code, name in enumerate(("F32", "F16", "BF16")):
        assert f"#define MPHIP_DTYPE_{name} {code}" in hdr


def test_typed_entry_points_validate_arguments_without_a_gpu(lib):
    one = ctypes.c_void_p(16)
    assert lib.mphip_cast_to_f32_range(None, 1, 8, None, None, None) == -1
    assert lib.mphip_cast_to_f32_range(one, 7, 8, one, one, None) == -1
    assert b"unknown dtype" in lib.mphip_last_error()
    assert lib.mphip_warp_volume_dsum_coords_typed(one, one, one, 9, 1, 4, 4, 4, 4, 0, None) == -1
    assert lib.mphip_hot_slice_forward_typed(None, None, 1, *([None] * 7), None, 1, 1, None, 0, None) == -1


def test_reenact_dtype_option():
    from megaportrait_hack_amd import reenact

    assert reenact.parse([]).dtype == "fp32"
    assert reenact.parse(["--dtype", "bf16"]).dtype == "bf16"
    with pytest.raises(SystemExit):
        reenact.parse(["--dtype", "fp64"])


def test_model_dtype_and_mixed_dtype_refusal_before_any_launch():
    from megaportrait_hack_amd import model as M

    g = M.G3d(96)
    assert M.model_dtype(g) == torch.float32
    g.half()
    assert M.model_dtype(g) == torch.float16
    g.bfloat16()
    assert M.model_dtype(g) == torch.bfloat16
    g.final_conv.float()          # converted on its own (a plain nn.Conv3d): the module now mixes dtypes, the cached dtype says bf16
    x = torch.zeros(1, 96, 8, 8, 8, dtype=torch.bfloat16)   # a CPU tensor: any launch attempt would fail with a device error instead
    with torch.no_grad(), pytest.raises(RuntimeError, match="mix dtypes"):
        g(x)
    hot = M.GbaseHotSlice().half()
    hot.warp_generator_s2c.flowfield.gn.float()
    with torch.no_grad(), pytest.raises(RuntimeError, match="mix dtypes"):
        hot(x, x, x, x, x, x, x, x)


def test_twins_are_dropped_by_conversions_of_their_own_module_only():
    from megaportrait_hack_amd import model as M

    g = M.G2dHead().half()
    twin = M._twin(g)
    assert {p.dtype for p in twin.parameters()} == {torch.float32} and M._twin(g) is twin
    other = M.G2dHead().half()      # converting an unrelated module leaves this twin alone
    other.bfloat16()
    assert M._twin(g) is twin
    g.float()                       # converted back: no dead fp32 copy stays behind
    assert "_mphip_twin" not in g.__dict__
    g.half()
    g.conv1x1.weight.data = g.conv1x1.weight.data.float()   # a parameter replaced behind the module's back: checked afresh
    with pytest.raises(RuntimeError, match="mix dtypes"):
        M._twin(g)


def test_training_a_half_module_is_refused_before_any_launch():
    from megaportrait_hack_amd import model as M

    e = M.Eapp3DTail().half()
    with pytest.raises(RuntimeError, match="keep fp32 parameters and use torch.autocast"):
        e(torch.zeros(1, 1536, 4, 4, dtype=torch.float16))


def test_fp32_warp_kernels_keep_their_resources():
    """The K2/K3 kernels the fp32 path launches: registers, spills, scratch and LDS as recorded before the typed instantiations were
    added (every kernel is one template over the dtype; its fp32 instantiation, `name<0>`, is pinned here; tools/register_table.py)."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import register_table

    want = json.load(open(os.path.join(GOLD, "warp_fp32_kernel_meta.json")))
    table = register_table.collect(["warp.hip"])
    kernels = {k["demangled"]: k for t in table.values() for k in t["kernels"]}
    for name, meta in want.items():
        assert name in kernels, name
        got = {k: kernels[name].get(k) for k in meta}
        assert got == meta, (name, got, meta)
    # the fp16 / bf16 instantiations of the six K2/K3 kernels: the dtype is the (last) template argument
    typed = [n for n in kernels if re.fullmatch(r"warp_(gather(_columns|_direct|_scalar|_dsum)?|corner_image)_kernel<(\d+, )?[12]>", n)]
    assert len(typed) == 12, sorted(kernels)
    for n in typed:
        assert kernels[n].get("private_segment_fixed_size", 0) == 0 and kernels[n].get("vgpr_spill_count", 0) == 0, (n, kernels[n])
