"""GPU parity tests: every HIP kernel (through the C ABI, libmphip.so) against the CPU oracle
(oracle/hotpath_ref.py = ATen CPU, oracle/hotpath_c.c = plain C) and the committed golden
fixtures (outputs of the reference itself, tests/golden/, generator oracle/make_golden.py).

Bars: bit-exact for the flow-field index pipeline (coords, floor indices, warp-field
composition given identical theta/em); 1e-3 max-abs for float results (north_star), most
checks are far tighter and say so.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WEIGHT_SEED, INPUT_SEED = 7, 3


def gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from megaportrait_hack_amd import _lib, ops

    _lib.load()  # fail loudly if the HIP extension is missing
    return ops


@pytest.fixture(scope="module")
def _libmod():
    from megaportrait_hack_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def M():
    from megaportrait_hack_amd import model

    return model


@pytest.fixture(scope="module")
def sd():
    return R.seeded_gbase_hot_state_dict(WEIGHT_SEED)


@pytest.fixture(scope="module")
def hot(M, sd, dev):
    h = M.GbaseHotSlice()
    M.load_hot_state_dict(h, sd)
    return h.to(dev).eval()


def maxabs(a, b):
    return (a.detach().cpu().double() - torch.as_tensor(b).double()).abs().max().item()


# ------------------------------------------------------------------------------- K0 / K1
def test_rt_theta(ops, dev):
    rot = R.seeded_tensor((8, 3), 101, scale=30.0)
    tr = R.seeded_tensor((8, 3), 102, scale=0.17)
    for inv in (False, True):
        got = ops.rt_theta(rot.to(dev), tr.to(dev), inv)
        assert maxabs(got, R.affine_theta(rot, tr, inv)) < 2e-6


def test_warp_field_compose_bit_exact(ops, dev, oracle_c):
    theta = R.seeded_tensor((3, 3, 4), 201)
    em = (R.seeded_tensor((3, 3, 16, 16, 16), 202) + 1.0) * 0.5
    w, rt, e64 = ops.warp_field_compose(theta.to(dev), em.to(dev), 64, parts=True)
    rt_ref = oracle_c.affine_grid3d(theta, 64)
    em_ref = oracle_c.resize_trilinear(em, (64, 64, 64), False)
    assert torch.equal(rt.cpu(), rt_ref)                       # == F.affine_grid bit for bit
    assert torch.equal(e64.cpu(), em_ref)                      # == F.interpolate(AC=False) bit for bit
    assert torch.equal(w.cpu(), rt_ref + em_ref)
    # this host's ATen CPU kernels (bitwise equal to the C oracle in the build container, see
    # tests/test_oracle.py; FMA use inside ATen depends on the host ISA, so only a tolerance here)
    assert maxabs(rt_ref, F.affine_grid(theta, (3, 1, 64, 64, 64), align_corners=False).permute(0, 4, 1, 2, 3)) < 1e-6
    assert maxabs(em_ref, F.interpolate(em, size=(64, 64, 64), mode="trilinear", align_corners=False)) < 1e-6


def test_compute_rt_warp_golden(M, dev):
    g = gold("rt_warp")
    rot = R.seeded_tensor((8, 3), 101, scale=30.0).to(dev)
    tr = R.seeded_tensor((8, 3), 102, scale=0.17).to(dev)
    assert maxabs(M.compute_rt_warp(rot, tr, invert=False, grid_size=8), g["g8"]) < 5e-6
    assert maxabs(M.compute_rt_warp(rot, tr, invert=True, grid_size=8), g["g8_inv"]) < 5e-6
    assert maxabs(M.compute_rt_warp(rot, tr, invert=False, grid_size=64)[:, :, ::8, ::8, ::8], g["g64_s8"]) < 5e-6
    assert maxabs(M.compute_rt_warp(rot, tr, invert=True, grid_size=64)[:, :, ::8, ::8, ::8], g["g64_inv_s8"]) < 5e-6


# ------------------------------------------------------------------------------- K2 / K3
def _fields():
    faithful = R.seeded_tensor((2, 3, 64, 64, 64), 301, scale=1.3) + 0.4       # like rt+em: reaches the 4^3 corner
    wide = (R.seeded_tensor((2, 3, 64, 64, 64), 302) + 1.0) * torch.tensor([34.0, 34.0, 9.0]).view(1, 3, 1, 1, 1) - 2.0
    small = R.seeded_tensor((2, 3, 5, 7, 9), 303, scale=6.0) + 4.0             # generic (fD,fH,fW) != (D,H,W)
    return {"faithful": faithful, "wide": wide, "small": small}


@pytest.mark.parametrize("kind", ["faithful", "wide", "small"])
@pytest.mark.parametrize("shape", [(8, 16, 64, 64), (5, 6, 10, 14)])
def test_warp_volume_indices_bit_exact(ops, dev, oracle_c, kind, shape):
    C, D, H, W = shape
    field = _fields()[kind]
    v = R.seeded_tensor((2, C, D, H, W), 310, scale=1.7)
    out, coords, idx = ops.warp_volume(v.to(dev), field.to(dev), return_coords=True)
    c_ref, i_ref = oracle_c.warp_coords(field, D, H, W)
    assert torch.equal(coords.cpu(), c_ref), "clipped sample coordinates differ from the oracle"
    assert torch.equal(idx.cpu(), i_ref), "floor indices differ from the oracle"
    c_aten, i_aten = R.warp_coords(field, D, H, W)   # this host's ATen: tolerance only (host-ISA dependent bits)
    assert maxabs(c_ref, c_aten) < 1e-4 and (i_ref != i_aten).float().mean().item() < 1e-4
    want = R.apply_warping_field(v, field)
    assert maxabs(out, want) <= 1e-4
    assert torch.equal(out.cpu(), oracle_c.apply_warping_field(v, field))   # values too: bit for bit vs the C oracle
    got_sum = ops.warp_volume_dsum(v.to(dev), field.to(dev))
    assert maxabs(got_sum, want.sum(dim=2)) <= 2e-5


@pytest.mark.parametrize("B,C", [(1, 96), (2, 40), (8, 96), (3, 7), (8, 200), (1, 130)])
def test_warp_volume_corner_image_paths_are_bit_identical(ops, dev, oracle_c, B, C):
    """K2's corner gather (r04) has three ways to its LDS image — the corner image inside a larger workspace, an image built ahead
    of the call (mphip_warp_corner_image + mphip_warp_volume_coords_img: the plan's way), and no image at all (a caller whose
    workspace has the old size: the workgroup collects the corner itself) — and splits the channels over 1, 3 or 6 groups depending on
    the tile count.  All of them must give the C oracle's bits."""
    import ctypes
    lib = ops._lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    D, H, W = 16, 64, 64
    field = (R.seeded_tensor((B, 3, 64, 64, 64), 320 + B, scale=1.3) + 0.4)
    v = R.seeded_tensor((B, C, D, H, W), 330 + C, scale=1.7)
    want = oracle_c.apply_warping_field(v, field)
    vd, fd = v.to(dev), field.to(dev)
    lin = [ops.linspace_table(n, dev) for n in (D, H, W)]
    base = lib.mphip_warp_workspace_bytes(B, D, H, W)
    img_bytes = lib.mphip_warp_corner_image_bytes(B, C)
    assert img_bytes > 0
    outs = {}
    for name, extra in (("image in the workspace", img_bytes), ("no image", 0)):
        ws = torch.empty((base + extra) // 4, dtype=torch.float32, device=dev)
        out = torch.full_like(vd, float("nan"))
        rc = lib.mphip_warp_volume(P(vd), P(fd), P(lin[0]), P(lin[1]), P(lin[2]), P(out), None, None, None, B, C, D, H, W, 64, 64, 64,
                                   P(ws), base + extra, None)
        assert rc == 0, lib.mphip_last_error()
        outs[name] = out
    coords = torch.empty((B, D, H, W, 3), dtype=torch.float32, device=dev)
    assert lib.mphip_warp_coords(P(fd), P(lin[0]), P(lin[1]), P(lin[2]), P(coords), B, D, H, W, 64, 64, 64, None) == 0
    img = torch.empty(img_bytes // 4, dtype=torch.float32, device=dev)
    assert lib.mphip_warp_corner_image(P(vd), P(img), img_bytes, B, C, D, H, W, None) == 0, lib.mphip_last_error()
    ws = torch.empty(base // 4, dtype=torch.float32, device=dev)
    out = torch.full_like(vd, float("nan"))
    assert lib.mphip_warp_volume_coords_img(P(vd), P(coords), P(out), None, B, C, D, H, W, P(ws), base, P(img), None) == 0, lib.mphip_last_error()
    outs["image built ahead"] = out
    torch.cuda.synchronize()
    for name, out in outs.items():
        assert torch.equal(out.cpu(), want), name


def test_apply_warping_field_golden(ops, M, dev, hot, sd):
    g = gold("apply_warping_field")
    inp = R.seeded_hot_inputs(1, INPUT_SEED)
    with torch.no_grad():
        w_s2c = hot.warp_generator_s2c(inp["Rs"].to(dev), inp["ts"].to(dev), inp["zs"].to(dev), inp["es"].to(dev))
    v_small = R.seeded_tensor((1, 8, 16, 16, 16), 104, scale=1.7)
    out, coords, _ = ops.warp_volume(v_small.to(dev), w_s2c, return_coords=True)
    assert maxabs(out, g["small"]) < 1e-4
    assert maxabs(coords, g["coords_small"]) < 1e-4   # reference coords via the three-ramp trick
    wide = (R.seeded_tensor((1, 3, 64, 64, 64), 105) + 1.0) * 9.0 - 2.0
    assert maxabs(M.apply_warping_field(v_small.to(dev), wide.to(dev)), g["wide"]) <= 1e-6
    vc = M.apply_warping_field(inp["vs"].to(dev), w_s2c)
    assert maxabs(vc[:, :, ::2, ::4, ::4], g["full_s4"]) < 1e-4
    assert np.abs(vc.double().sum(dim=(2, 3, 4)).cpu().numpy() - g["full_chan_sum"]).max() < 0.5


# ------------------------------------------------------------------------------- K4 / K5
CONV_CASES = [
    # N, Ci, Co, D, H, W, k
    (1, 96, 96, 4, 8, 8, 3),
    (2, 96, 192, 4, 8, 8, 3),
    (1, 192, 96, 2, 4, 4, 3),
    (2, 384, 768, 2, 8, 8, 3),
    (1, 768, 384, 1, 1, 1, 3),
    (2, 512, 256, 4, 1, 1, 3),
    (2, 64, 32, 16, 8, 8, 3),
    (2, 32, 3, 16, 16, 16, 3),
    (1, 5, 7, 3, 5, 6, 3),       # odd channel counts, ragged tiles
    (2, 96, 192, 4, 8, 8, 1),
    (2, 512, 256, 4, 1, 1, 1),
    (1, 96, 96, 16, 64, 64, 3),  # the 60%-of-FLOPs layer at full size
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3d(ops, dev, case):
    N, Ci, Co, D, H, W, k = case
    x = R.seeded_tensor((N, Ci, D, H, W), 401, scale=1.7)
    fan = Ci * k ** 3
    wt = R.seeded_tensor((Co, Ci, k, k, k), 402, scale=fan ** -0.5)
    bias = R.seeded_tensor((Co,), 403, scale=fan ** -0.5)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    want = F.conv3d(x, wt, bias, padding=k // 2)
    assert maxabs(ops.conv3d(x.to(dev), pc, precision=0), want) < 2e-5      # exact fp32 MFMA
    assert maxabs(ops.conv3d(x.to(dev), pc, precision=1), want) < 2e-5      # f16x3 where supported, else fp32


F16X3_CASES = [(2, 96, 96, 4, 8, 8), (1, 96, 192, 8, 16, 16), (2, 192, 96, 2, 8, 8), (1, 768, 768, 2, 8, 8),
               (1, 384, 192, 4, 16, 16), (1, 96, 96, 16, 64, 64)]


@pytest.mark.parametrize("stress", [False, True], ids=["plain", "outliers"])
@pytest.mark.parametrize("case", F16X3_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3d_f16x3_is_fp32_class(ops, _libmod, dev, case, stress):
    """The split-f16 kernel must be fp32-class against the fp64 truth.
    plain:    O(1) data -> error no worse than the exact-fp32 MFMA kernel's own rounding (same order).
    outliers: a 300.0 activation, a 1.5 weight (75x the rest), f16-subnormal-lo values and zeros in one
              receptive field.  The f16 MFMA aligns the 16 products of an instruction to the largest one,
              so — like a running fp32 sum — the error scales with the largest partial sum: bounded
              relative to max|y| (2^-20), not per term."""
    N, Ci, Co, D, H, W = case
    assert _libmod.load().mphip_conv3d_supported(N, Ci, Co, D, H, W, 3, 1) == 1
    x = R.seeded_tensor((N, Ci, D, H, W), 421, scale=1.7)
    wt = R.seeded_tensor((Co, Ci, 3, 3, 3), 422, scale=(Ci * 27) ** -0.5)
    if stress:
        x[0, 0, 0, 0, :4] = torch.tensor([300.0, -1e-4, 3e-6, 0.0])
        wt[0, 0, 1, 1, :3] = torch.tensor([1.5, -2e-5, 0.0])
    bias = R.seeded_tensor((Co,), 423, scale=0.1)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    truth = F.conv3d(x.double(), wt.double(), bias.double(), padding=1)
    e32 = maxabs(ops.conv3d(x.to(dev), pc, precision=0), truth)
    e16 = maxabs(ops.conv3d(x.to(dev), pc, precision=1), truth)
    scale = truth.abs().max().item()
    print(f"max-abs vs fp64: fp32-MFMA {e32:.2e}, f16x3 {e16:.2e} (max|y| = {scale:.1f})")
    if stress:
        assert e16 / scale < 1e-6 and e32 / scale < 1e-6
    else:
        assert e16 < 2 * e32 + 1e-6 and e16 < 1e-5


WINO_CASES = [(1, 96, 96, 16, 64, 64), (8, 96, 192, 8, 32, 32), (8, 192, 192, 8, 32, 32), (8, 192, 96, 8, 32, 32), (3, 96, 96, 16, 64, 64),
              (1, 256, 96, 16, 64, 64)]


@pytest.mark.parametrize("case", WINO_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3d_f16x3_winograd_domain_is_fp32_class(ops, _libmod, dev, case):
    """The launches that fill the chip run the split-f16 arithmetic in the 1-D Winograd F(2,3) domain (conv3d_f16x3_wino.hip: 2/3 of the
    MFMAs; G3d's levels 0-1 at the graded batch, Eapp's 3-D tail).  Same bar as the direct kernel: against the fp64 truth no worse than
    twice the exact-fp32 MFMA kernel's own rounding; the GroupNorm statistics its epilogue leaves (the partials of its two plane pairs
    per tile) against float64 statistics of the truth; the direct kernel (MPHIP_WINOGRAD=0) beside it; and — bwd-data is the same kernel
    on the transposed pack — the input gradient against conv_transpose3d in float64."""
    N, Ci, Co, D, H, W = case
    lib = _libmod.load()
    assert lib.mphip_conv3d_kernel_variant(N, Ci, Co, D, H, W, 3, 1) == 5      # the F(2,3) kernel takes this shape
    x = R.seeded_tensor((N, Ci, D, H, W), 431, scale=1.7)
    wt = R.seeded_tensor((Co, Ci, 3, 3, 3), 432, scale=(Ci * 27) ** -0.5)
    bias = R.seeded_tensor((Co,), 433, scale=0.1)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    truth = F.conv3d(x.double(), wt.double(), bias.double(), padding=1)
    xd = x.to(dev)
    e32 = maxabs(ops.conv3d(xd, pc, precision=0), truth)
    y, st = ops.conv3d(xd, pc, precision=1, gn_groups=32)
    ew = maxabs(y, truth)
    os.environ["MPHIP_WINOGRAD"] = "0"
    try:
        assert lib.mphip_conv3d_kernel_variant(N, Ci, Co, D, H, W, 3, 1) in (1, 2)
        ed = maxabs(ops.conv3d(xd, pc, precision=1), truth)
    finally:
        del os.environ["MPHIP_WINOGRAD"]
    print(f"max-abs vs fp64: fp32-MFMA {e32:.2e}, direct f16x3 {ed:.2e}, F(2,3) f16x3 {ew:.2e} (max|y| = {truth.abs().max().item():.1f})")
    assert ew < 2 * e32 + 1e-6 and ew < 2e-5
    tr = truth.reshape(N, 32, -1)
    assert maxabs(st[:, 0], tr.mean(-1).reshape(-1)) < 1e-6
    assert maxabs(st[:, 1], (1.0 / torch.sqrt(tr.var(-1, unbiased=False) + 1e-5)).reshape(-1)) < 1e-5
    # bwd-data: dy [N,Co,..] -> dx [N,Ci,..] when that launch fills the chip too
    if lib.mphip_conv3d_kernel_variant(N, Co, Ci, D, H, W, 3, 1) == 5:
        dy = R.seeded_tensor((N, Co, D, H, W), 434, scale=3e-3)
        dy[:, :, : D // 2] *= 1e-3                                            # a gradient's dynamic range
        want = F.conv_transpose3d(dy.double(), wt.double(), padding=1)
        _, scale = ops.grad_prep(dy.to(dev), want_bias=False)
        dx = ops.conv3d_bwd_data(dy.to(dev), ops.PackedConv(wt.to(dev), None, transposed=True), scale)
        assert maxabs(dx, want) / want.abs().max().item() < 3e-6


ROLE_SPLIT_CASES = [(1, 96, 96, 16, 64, 64), (8, 192, 192, 8, 32, 32), (2, 96, 96, 4, 8, 8), (3, 16, 96, 4, 16, 8), (8, 384, 192, 4, 16, 16),
                    (1, 256, 96, 8, 24, 40), (5, 96, 96, 4, 16, 16)]


@pytest.mark.parametrize("case", ROLE_SPLIT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3d_f16x3_winograd_role_split_and_lockstep_schedules_agree(ops, dev, case, monkeypatch):
    """The F(2,3) kernel has two schedules of the same arithmetic: the default role-split one (conv3d_f16x3_wino_pp.hip: the two waves of a
    SIMD alternate MFMA and load segments, the K loop walks 8-channel chunks) and the lockstep one it replaced (MPHIP_WINO_PP=0).  They
    sum in a different order, so they are not bitwise equal; both must be fp32-class against float64 and agree with each other to that
    class — full launches, split-K launches (2x96x96@4x8x8: 6 splits), a single 16-channel period, multi-frame fused GroupNorm + ReLU
    inputs (the per-frame table is reloaded by LDS-DMA), and the GroupNorm statistics the epilogue leaves."""
    N, Ci, Co, D, H, W = case
    monkeypatch.setenv("MPHIP_WINOGRAD_MIN_TILES", "1")     # (the kernel wherever its tiling applies, also below a full chip)
    x = R.seeded_tensor((N, Ci, D, H, W), 441, scale=1.7)
    wt = R.seeded_tensor((Co, Ci, 3, 3, 3), 442, scale=(Ci * 27) ** -0.5)
    bias = R.seeded_tensor((Co,), 443, scale=0.1)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    truth = F.conv3d(x.double(), wt.double(), bias.double(), padding=1)
    g, be = R.seeded_tensor((Ci,), 444, scale=0.3) + 1.0, R.seeded_tensor((Ci,), 445, scale=0.2)
    groups = 32 if Ci % 32 == 0 else 16
    truth_gn = F.conv3d(F.relu(F.group_norm(x.double(), groups, g.double(), be.double(), 1e-5)), wt.double(), bias.double(), padding=1)
    xd = x.to(dev)
    st_in = ops.groupnorm_stats(xd, groups)
    out = {}
    for pp in ("1", "0"):
        monkeypatch.setenv("MPHIP_WINO_PP", pp)
        y, st = ops.conv3d(xd, pc, precision=1, gn_groups=32)
        out[pp] = (y, st, ops.conv3d_gn_in(xd, st_in, g.to(dev), be.to(dev), groups, pc))
    monkeypatch.delenv("MPHIP_WINO_PP")
    e32 = maxabs(ops.conv3d(xd, pc, precision=0), truth)
    for pp in ("1", "0"):
        assert maxabs(out[pp][0], truth) < 2 * e32 + 1e-6, pp
        assert maxabs(out[pp][2], truth_gn) < 1e-5, pp
    scale = truth.abs().max().item()
    assert maxabs(out["1"][0], out["0"][0].cpu().double()) < 4e-6 * max(scale, 1.0)
    assert maxabs(out["1"][1], out["0"][1].cpu().double()) < 1e-5
    assert maxabs(out["1"][2], out["0"][2].cpu().double()) < 4e-6 * max(truth_gn.abs().max().item(), 1.0)


@pytest.mark.parametrize("case", ROLE_SPLIT_CASES + [(8, 384, 384, 4, 16, 16), (2, 96, 192, 8, 32, 32)], ids=lambda c: "x".join(map(str, c)))
def test_conv3d_f16x3_winograd_big_tile_kernel_is_bitwise_the_role_split_one(ops, dev, case, monkeypatch):
    """r06's third schedule of the F(2,3) conv (conv3d_f16x3_wino_bt.hip, MPHIP_WINO_PP=2: one wave per SIMD, 96 x 128 accumulators, both
    staging roles in every thread) keeps the role-split kernel's accumulation order per output element: outputs, GroupNorm statistics
    and fused-GroupNorm-input results must be torch.equal — full launches, split-K, a single period, several frames per workgroup."""
    N, Ci, Co, D, H, W = case
    monkeypatch.setenv("MPHIP_WINOGRAD_MIN_TILES", "1")
    x = R.seeded_tensor((N, Ci, D, H, W), 471, scale=1.7).to(dev)
    pc = ops.PackedConv(R.seeded_tensor((Co, Ci, 3, 3, 3), 472, scale=(Ci * 27) ** -0.5).to(dev), R.seeded_tensor((Co,), 473, scale=0.1).to(dev))
    g, be = (R.seeded_tensor((Ci,), 474, scale=0.3) + 1.0).to(dev), R.seeded_tensor((Ci,), 475, scale=0.2).to(dev)
    groups = 32 if Ci % 32 == 0 else 16
    st_in = ops.groupnorm_stats(x, groups)
    out = {}
    for pp in ("1", "2"):
        monkeypatch.setenv("MPHIP_WINO_PP", pp)
        y, st = ops.conv3d(x, pc, precision=1, gn_groups=32)
        out[pp] = (y, st, ops.conv3d_gn_in(x, st_in, g, be, groups, pc))
    monkeypatch.delenv("MPHIP_WINO_PP")
    for a, b in zip(out["1"], out["2"]):
        a, b = (a[0], b[0]) if isinstance(a, tuple) else (a, b)
        assert torch.equal(a, b)


D2_CASES = [(8, 384, 768, 8, 8), (8, 768, 768, 8, 8), (8, 768, 384, 8, 8), (8, 384, 384, 8, 8), (3, 96, 96, 8, 16), (1, 96, 192, 16, 8), (5, 192, 96, 8, 8)]


@pytest.mark.parametrize("case", D2_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3d_f16x3_winograd_two_frame_mode_at_depth_2(ops, _libmod, dev, case, monkeypatch):
    """G3d's 2x8x8 level (model.py:576-589: ResBlock3D(384,768), ResBlock3D(768,384)) in the F(2,3) domain ("a D = 2 form of
    the fast conv"): the big-tile kernel's two-frame mode — a tile = two frames x 2 x 8 x 8, halo-plane slots [zero, n:d0, n:d1, zero,
    n+1:d0, n+1:d1].  Against float64 it must be fp32-class (<= 2e-5 of max|y|, <= 2x the exact-fp32 MFMA kernel's error) plain and with
    the input GroupNorm + ReLU fused (its table comes from global memory per halo row in this mode), for even and odd batches (the
    last tile of an odd batch has one frame), split-K launches, and agree with the direct f16x3 kernel (MPHIP_WINOGRAD_D2=0) to that
    class; the GroupNorm statistics of the output come from the separate pass and must agree too."""
    N, Ci, Co, H, W = case
    monkeypatch.setenv("MPHIP_WINOGRAD_MIN_TILES", "1")
    lib = _libmod.load()
    x = R.seeded_tensor((N, Ci, 2, H, W), 481, scale=1.7)
    wt = R.seeded_tensor((Co, Ci, 3, 3, 3), 482, scale=(Ci * 27) ** -0.5)
    bias = R.seeded_tensor((Co,), 483, scale=0.1)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    truth = F.conv3d(x.double(), wt.double(), bias.double(), padding=1)
    g, be = R.seeded_tensor((Ci,), 484, scale=0.3) + 1.0, R.seeded_tensor((Ci,), 485, scale=0.2)
    truth_gn = F.conv3d(F.relu(F.group_norm(x.double(), 32, g.double(), be.double(), 1e-5)), wt.double(), bias.double(), padding=1)
    xd = x.to(dev)
    st_in = ops.groupnorm_stats(xd, 32)
    out = {}
    for d2 in ("1", "0"):
        monkeypatch.setenv("MPHIP_WINOGRAD_D2", d2)
        assert (lib.mphip_conv3d_kernel_variant(N, Ci, Co, 2, H, W, 3, 1) == 5) == (d2 == "1")
        y, st = ops.conv3d(xd, pc, precision=1, gn_groups=32)
        out[d2] = (y, st, ops.conv3d_gn_in(xd, st_in, g.to(dev), be.to(dev), 32, pc))
    monkeypatch.delenv("MPHIP_WINOGRAD_D2")
    e32 = maxabs(ops.conv3d(xd, pc, precision=0), truth)
    top, top_gn = truth.abs().max().item(), truth_gn.abs().max().item()
    for d2 in ("1", "0"):
        assert maxabs(out[d2][0], truth) < 2 * e32 + 1e-6 and maxabs(out[d2][0], truth) < 2e-5 * top, d2
        gn_out = out[d2][2][0] if isinstance(out[d2][2], tuple) else out[d2][2]
        assert maxabs(gn_out, truth_gn) < 2e-5 * max(top_gn, 1.0), d2
    assert maxabs(out["1"][0], out["0"][0].cpu().double()) < 4e-6 * max(top, 1.0)
    assert maxabs(out["1"][1], out["0"][1].cpu().double()) < 1e-5
    # bwd-data of this level is the same launch on the transposed pack
    dy = R.seeded_tensor((N, Co, 2, H, W), 486, scale=3e-3)
    xg = x.clone().requires_grad_(True)
    F.conv3d(xg, wt, None, padding=1).backward(dy)
    _, sc = ops.grad_prep(dy.to(dev), want_bias=False)
    dx = ops.conv3d_bwd_data(dy.to(dev), ops.PackedConv(wt.to(dev), None, transposed=True), sc)
    assert maxabs(dx, xg.grad.double()) < 2e-5 * xg.grad.abs().max().item()


HALF_CASES = [(1, 96, 96, 16, 64, 64), (8, 192, 192, 8, 32, 32), (2, 96, 192, 8, 32, 32)]


@pytest.mark.parametrize("case", HALF_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3d_half_products_follow_the_autocast_contract(ops, _libmod, dev, case, monkeypatch):
    """The reference's generator step runs under torch.cuda.amp.autocast() (train.py:145,188): conv3d multiplies f16 operands and
    accumulates in fp32.  ops.half_products() switches the F(2,3) conv launches to that policy — ONE f16 product per multiply (the
    transformed operands rounded to f16).
    THE GATE: oracle.hotpath_ref.conv3d_wino_f16_contract — the kernel's own arithmetic contract (t = Bt x in fp32 and
    u = G g in double, each rounded to f16 once, exact accumulation): <= 2e-5 of max|y|, i.e. nothing but the kernel's fp32 accumulation
    is left — a wrong tap, position or transform weighted 1/300 fails it.  Beside it, as a sanity bound only: 3e-3 of max|y| against
    conv3d_f16_operands (x and g rounded instead of t and u — the distance two correct f16 implementations of one conv, direct vs
    Winograd, have).  Outside the context nothing changes (bitwise), forward and bwd-data."""
    N, Ci, Co, D, H, W = case
    monkeypatch.setenv("MPHIP_WINOGRAD_MIN_TILES", "1")
    lib = _libmod.load()
    assert lib.mphip_conv3d_kernel_variant(N, Ci, Co, D, H, W, 3, 1) == 5
    x = R.seeded_tensor((N, Ci, D, H, W), 451, scale=1.7)
    wt = R.seeded_tensor((Co, Ci, 3, 3, 3), 452, scale=(Ci * 27) ** -0.5)
    bias = R.seeded_tensor((Co,), 453, scale=0.1)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    xd = x.to(dev)
    truth = F.conv3d(x.double(), wt.double(), bias.double(), padding=1)
    want = R.conv3d_f16_operands(x, wt, bias, padding=1)
    full = ops.conv3d(xd, pc, precision=1)
    with ops.half_products(True):
        half = ops.conv3d(xd, pc, precision=1)
    again = ops.conv3d(xd, pc, precision=1)
    scale = truth.abs().max().item()
    contract = R.conv3d_wino_f16_contract(x, wt, bias)
    e_gate = maxabs(half, contract) / scale
    e_half, e_full, e_oracle = maxabs(half, want) / scale, maxabs(full, truth) / scale, maxabs(want, truth) / scale
    print(f"relative to max|y|: half products vs the F(2,3) f16 contract {e_gate:.2e} (gate 2e-5); vs the f16-operand oracle {e_half:.2e}; "
          f"f16-operand oracle vs fp64 {e_oracle:.2e}; f16x3 vs fp64 {e_full:.2e}")
    assert torch.equal(full, again)                      # the flag is scoped
    assert e_gate < 2e-5, e_gate
    assert e_half < 3e-3 and e_full < 1e-5 and not torch.equal(half, full)   # (sanity bound, not the gate)
    assert maxabs(half, truth) / scale < 2 * e_oracle + 3e-3
    # bwd-data is the same kernel on the transposed pack
    if lib.mphip_conv3d_kernel_variant(N, Co, Ci, D, H, W, 3, 1) == 5:
        dy = R.seeded_tensor((N, Co, D, H, W), 454, scale=3e-3)
        wt_t = wt.flip(2, 3, 4).transpose(0, 1).contiguous()
        _, sc = ops.grad_prep(dy.to(dev), want_bias=False)
        pct = ops.PackedConv(wt.to(dev), None, transposed=True)
        with ops.half_products(True):
            dx = ops.conv3d_bwd_data(dy.to(dev), pct, sc)
        want_dx = R.conv3d_f16_operands(dy, wt_t, None, padding=1)
        top = want_dx.abs().max().item()
        assert maxabs(dx, R.conv3d_wino_f16_contract(dy, wt_t)) / top < 2e-5     # the gate
        assert maxabs(dx, want_dx) / top < 3e-3                                  # sanity bound


def test_g3d_under_autocast_uses_half_products(ops, _libmod, dev, monkeypatch):
    """model.G3d inside torch.autocast(float16) runs its F(2,3) convs with f16 operands (the reference's policy), everything else — and
    everything outside the region — as before.  Oracle: the restatement's G3d with conv3d_f16_operands on exactly the layers the library
    reports the F(2,3) kernel for.  THE GATE: those layers on conv3d_wino_f16_contract (the kernel's own rounding points).
    One conv agrees with that contract to 2e-5 (test_conv3d_half_products_follow_the_autocast_contract); a STACK of 15 cannot be held to
    1e-4, and not because of the kernel: the contract oracle evaluated twice — activations between the layers kept in float64 / in float32
    (what the kernels exchange) — differs from ITSELF by ~7e-4 of max|y| on this case (an operand that sits within 1e-7 of an f16 rounding
    boundary flips, the flip is a 5e-4 relative change of that operand, and GroupNorm + ReLU carry it on).  So the bar is calibrated in the
    test: the kernel must be as close to the fp32-activation contract as the contract's two evaluations are to each other (x2, + 1e-4).
    The r05 oracle (conv3d_f16_operands: x and g rounded, not t and u) stays beside it at 1e-2 as a sanity bound.  The region must
    actually change the result."""
    from megaportrait_hack_amd import model as M

    monkeypatch.setenv("MPHIP_WINOGRAD_MIN_TILES", "1")
    lib = _libmod.load()
    g = M.G3d(96)
    sd = R.seeded_state_dict(R.g3d_shapes(96), 461, prefix="G3d.")
    g.load_state_dict({k[len("G3d."):]: v for k, v in sd.items()})
    g = g.to(dev).eval()
    x = R.seeded_tensor((2, 96, 16, 32, 32), 462)

    def conv(xx, w, b=None, padding=0):
        n, ci, d, h, ww = xx.shape
        if w.shape[2] == 3 and lib.mphip_conv3d_kernel_variant(n, ci, w.shape[0], d, h, ww, 3, 1) == 5:
            return R.conv3d_f16_operands(xx, w, b, padding=padding).to(xx.dtype)
        return F.conv3d(xx, w, b, padding=padding)

    monkeypatch.setattr(R, "CONV3D", conv)
    want = R.g3d(x.double(), {k: v.double() for k, v in sd.items()})

    def conv_contract(xx, w, b=None, padding=0):
        n, ci, d, h, ww = xx.shape
        if w.shape[2] == 3 and lib.mphip_conv3d_kernel_variant(n, ci, w.shape[0], d, h, ww, 3, 1) == 5:
            return R.conv3d_wino_f16_contract(xx, w, b, padding=padding).to(xx.dtype)
        return F.conv3d(xx, w, b, padding=padding)

    monkeypatch.setattr(R, "CONV3D", conv_contract)
    gate64 = R.g3d(x.double(), {k: v.double() for k, v in sd.items()})
    gate = R.g3d(x.float(), {k: v.float() for k, v in sd.items()}).double()
    monkeypatch.setattr(R, "CONV3D", F.conv3d)
    truth = R.g3d(x.double(), {k: v.double() for k, v in sd.items()})
    with torch.no_grad():
        plain = g(x.to(dev))
        with torch.autocast("cuda", dtype=torch.float16):
            half = g(x.to(dev))
        plain2 = g(x.to(dev))
    scale = truth.abs().max().item()
    sens = (gate - gate64).abs().max().item() / scale        # the contract against itself: fp32 vs fp64 activations between the layers
    print(f"relative to max|y|: autocast G3d vs the F(2,3) f16 contract {maxabs(half, gate) / scale:.2e} (the contract vs itself, fp32 / fp64 "
          f"activations: {sens:.2e}; gate 2x that + 1e-4); vs the f16-operand oracle {maxabs(half, want) / scale:.2e}; that oracle vs fp64 "
          f"{maxabs(want, truth) / scale:.2e}; default vs fp64 {maxabs(plain, truth) / scale:.2e}")
    assert half.dtype == torch.float32 and torch.equal(plain, plain2)
    assert maxabs(plain, truth) / scale < 1e-4
    assert sens < 3e-3 and maxabs(half, gate) / scale < 2 * sens + 1e-4
    assert maxabs(half, want) / scale < 1e-2 and not torch.equal(half, plain)   # (sanity bound, not the gate)


def test_conv3d_f16x3_winograd_propagates_non_finite(ops, _libmod, dev):
    """test_f16x3_propagates_non_finite at a shape the F(2,3) kernel takes: a NaN / Inf input poisons exactly the output voxels the
    reference's fp32 conv poisons (the transform mixes x[w-1..w+2] into one output pair, but a pair's two outputs use different
    products: no extra voxel turns non-finite), everything else stays fp32-class, and the diagnostic counter sees it."""
    x = R.seeded_tensor((1, 96, 16, 64, 64), 835, scale=1.7)
    w = R.seeded_tensor((96, 96, 3, 3, 3), 836, scale=0.02)
    assert _libmod.load().mphip_conv3d_kernel_variant(1, 96, 96, 16, 64, 64, 3, 1) == 5
    pc = ops.PackedConv(w.to(dev), None)
    for bad, pos in ((float("nan"), (0, 7, 1, 4, 9)), (float("inf"), (0, 50, 15, 63, 0)), (float("-inf"), (0, 3, 8, 17, 63))):
        xb = x.clone()
        xb[pos] = bad
        ops.f16x3_saturation_count(reset=True)
        got = ops.conv3d(xb.to(dev), pc, precision=1).cpu()
        want = F.conv3d(xb, w, None, padding=1)
        assert torch.equal(torch.isfinite(got), torch.isfinite(want))
        assert (got[torch.isfinite(want)] - want[torch.isfinite(want)]).abs().max().item() < 1e-4
        assert ops.f16x3_saturation_count(reset=True) >= 1


def test_conv3d_vs_c_oracle(ops, dev, oracle_c):
    x = R.seeded_tensor((1, 24, 3, 6, 5), 411, scale=1.7)
    wt = R.seeded_tensor((40, 24, 3, 3, 3), 412, scale=0.04)
    bias = R.seeded_tensor((40,), 413, scale=0.04)
    got = ops.conv3d(x.to(dev), ops.PackedConv(wt.to(dev), bias.to(dev)))
    assert maxabs(got, oracle_c.conv3d(x, wt, bias)) < 5e-6   # the C oracle accumulates in double


# ------------------------------------------------------------------------------- K6 / K7 / K8
@pytest.mark.parametrize("shape,groups", [((2, 96, 4, 8, 8), 32), ((1, 96, 16, 64, 64), 32), ((2, 32, 16, 8, 8), 32),
                                          ((3, 3, 16, 16, 16), 1), ((2, 64, 3, 5, 7), 32)])
def test_groupnorm(ops, dev, shape, groups):
    x = R.seeded_tensor(shape, 501, scale=2.0) + 0.3
    c = shape[1]
    g, b = R.seeded_tensor((c,), 502, scale=0.25, shift=1.0), R.seeded_tensor((c,), 503, scale=0.25)
    w2, b2 = R.seeded_tensor((1, c, 1, 1, 1), 504, scale=0.25, shift=1.0), R.seeded_tensor((1, c, 1, 1, 1), 505, scale=0.25)
    res = R.seeded_tensor(shape, 506)
    xd = x.to(dev)
    st = ops.groupnorm_stats(xd, groups)
    xr = x.reshape(shape[0], groups, -1).double()
    assert maxabs(st[:, 0], xr.mean(-1).reshape(-1)) < 1e-6
    assert maxabs(st[:, 1], (1.0 / torch.sqrt(xr.var(-1, unbiased=False) + 1e-5)).reshape(-1)) < 1e-5
    ref = F.group_norm(x, groups, g, b, 1e-5)
    assert maxabs(ops.groupnorm_apply(xd, st, g.to(dev), b.to(dev), groups), ref) < 1e-5
    full = F.relu(ref * w2 + b2 + res)
    got = ops.groupnorm_apply(xd, st, g.to(dev), b.to(dev), groups, w2=w2.to(dev), b2=b2.to(dev), residual=res.to(dev), relu=True)
    assert maxabs(got, full) < 1e-5
    assert maxabs(ops.groupnorm_apply(xd, st, g.to(dev), b.to(dev), groups, relu=True, tanh=True), torch.tanh(F.relu(ref))) < 1e-5
    if all(s % 2 == 0 for s in shape[2:]):
        got = ops.groupnorm_apply(xd, st, g.to(dev), b.to(dev), groups, residual=res.to(dev), relu=True, pool2=True)
        assert maxabs(got, F.avg_pool3d(F.relu(ref + res), 2, 2)) < 1e-5


def test_resample_bit_exact(ops, dev):
    x = R.seeded_tensor((2, 6, 4, 8, 6), 601)
    assert torch.equal(ops.avgpool2(x.to(dev)).cpu(), F.avg_pool3d(x, 2, 2))
    assert torch.equal(ops.upsample_trilinear2(x.to(dev)).cpu(),
                       F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=True))
    for sc in ((2, 2, 2), (1, 2, 2)):
        assert torch.equal(ops.upsample_nearest(x.to(dev), sc).cpu(), F.interpolate(x, scale_factor=sc, mode="nearest"))


def test_add_matmul(ops, dev):
    a, a2 = R.seeded_tensor((3, 512), 701, scale=1.7), R.seeded_tensor((3, 512), 702, scale=1.7)
    m = R.seeded_tensor((512, 512), 703, scale=1.7)
    assert maxabs(ops.add_matmul(a.to(dev), a2.to(dev), m.to(dev)), (a + a2).double() @ m.double()) < 2e-3  # |out| ~ 70
    w, b = R.seeded_tensor((2048, 512), 704, scale=0.04), R.seeded_tensor((2048,), 705, scale=0.04)
    assert maxabs(ops.add_matmul(a.to(dev), None, w.to(dev), b.to(dev), trans=True), F.linear(a, w, b)) < 2e-5


def test_split_aware_groupnorm_chain(ops, dev):
    """FlowField-sized tensors: conv left in split-K form, GroupNorm kernels sum the slabs themselves
    (stats_split / apply_split / small_fused) — all three against the plain reduce-then-normalise chain."""
    x = R.seeded_tensor((2, 256, 8, 2, 2), 801, scale=1.7)
    wt = R.seeded_tensor((128, 256, 3, 3, 3), 802, scale=(256 * 27) ** -0.5)
    bias = R.seeded_tensor((128,), 803, scale=0.1)
    res = R.seeded_tensor((2, 128, 8, 2, 2), 804)
    g, b = R.seeded_tensor((128,), 805, scale=0.25, shift=1.0), R.seeded_tensor((128,), 806, scale=0.25)
    w2, b2 = R.seeded_tensor((1, 128, 1, 1, 1), 807, scale=0.25, shift=1.0), R.seeded_tensor((1, 128, 1, 1, 1), 808, scale=0.25)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    co = ops.conv3d_split(x.to(dev), pc, precision=0)
    assert co.splits > 1, "this shape is meant to exercise split-K"
    y_ref = F.conv3d(x, wt, bias, padding=1)
    assert maxabs(ops._finish(co), y_ref) < 2e-5
    st = ops.groupnorm_stats(co, 32)
    yr = y_ref.reshape(2, 32, -1).double()
    assert maxabs(st[:, 0], yr.mean(-1).reshape(-1)) < 1e-5
    want = F.relu(F.group_norm(y_ref, 32, g, b, 1e-5) * w2 + b2 + res)
    args = dict(w2=w2.to(dev), b2=b2.to(dev), residual=res.to(dev), relu=True)
    assert maxabs(ops.groupnorm_apply(co, st, g.to(dev), b.to(dev), 32, **args), want) < 2e-5
    up = ops.groupnorm_apply(co, st, g.to(dev), b.to(dev), 32, up=(1, 2, 2), **args)
    assert maxabs(up, F.interpolate(want, scale_factor=(1, 2, 2), mode="nearest")) < 2e-5
    assert ops.groupnorm_fused_ok(co, 32)
    one = ops.groupnorm_small(co, g.to(dev), b.to(dev), 32, 1e-5, up=(2, 2, 2), **args)
    assert maxabs(one, F.interpolate(want, scale_factor=2, mode="nearest")) < 2e-5
    # residual that is itself a split conv output (FlowField's 1x1 residual_conv)
    w1 = R.seeded_tensor((128, 256, 1, 1, 1), 809, scale=256 ** -0.5)
    rco = ops.conv3d_split(x.to(dev), ops.PackedConv(w1.to(dev), bias.to(dev)), precision=0)
    want2 = F.relu(F.group_norm(y_ref, 32, g, b, 1e-5) + F.conv3d(x, w1, bias))
    assert maxabs(ops.groupnorm_small(co, g.to(dev), b.to(dev), 32, 1e-5, residual=rco, relu=True), want2) < 2e-5


def test_groupnorm_folded_into_conv(ops, dev):
    """conv(relu(GN(x))) as one launch (mphip_groupnorm_affine_table + mphip_conv3d_gnin_fwd) vs the unfused ops,
    including AdaptiveGroupNorm's second affine and the zero padding (which must stay 0, not relu(shift))."""
    x = R.seeded_tensor((2, 96, 4, 8, 16), 811, scale=1.7) + 0.5
    wt = R.seeded_tensor((96, 96, 3, 3, 3), 812, scale=(96 * 27) ** -0.5)
    bias = R.seeded_tensor((96,), 813, scale=0.1)
    g, b = R.seeded_tensor((96,), 814, scale=0.25, shift=1.0), R.seeded_tensor((96,), 815, scale=0.25, shift=0.5)
    w2, b2 = R.seeded_tensor((1, 96, 1, 1, 1), 816, scale=0.25, shift=1.0), R.seeded_tensor((1, 96, 1, 1, 1), 817, scale=0.25)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    ops.set_conv_precision("f16x3")
    assert ops.gn_in_conv_ok(tuple(x.shape), pc)
    st = ops.groupnorm_stats(x.to(dev), 32)
    got = ops.conv3d_gn_in(x.to(dev), st, g.to(dev), b.to(dev), 32, pc)
    want = F.conv3d(F.relu(F.group_norm(x, 32, g, b, 1e-5)), wt, bias, padding=1)
    assert maxabs(got, want) < 2e-5
    got = ops.conv3d_gn_in(x.to(dev), st, g.to(dev), b.to(dev), 32, pc, w2=w2.to(dev), b2=b2.to(dev))
    want = F.conv3d(F.relu(F.group_norm(x, 32, g, b, 1e-5) * w2 + b2), wt, bias, padding=1)
    assert maxabs(got, want) < 2e-5


@pytest.mark.parametrize("shape", [(2, 96, 96, 8, 16, 32), (1, 96, 192, 4, 16, 16), (1, 192, 384, 4, 8, 16), (2, 384, 768, 4, 8, 8),
                                   # unsplit launches: the statistics come from the conv kernel's epilogue (per-tile partials + finalize),
                                   # one shape per kernel variant: F(2,3) / 4x8x8 tiles / 2x8x8 tiles on four waves
                                   (2, 96, 96, 16, 64, 32), (4, 96, 192, 8, 32, 64), (4, 96, 96, 2, 64, 128)])
def test_conv_with_groupnorm_statistics(ops, dev, shape):
    """conv + the following GroupNorm's (mean, rstd) in one call (mphip_conv3d_gn_fwd / mphip_conv3d_gnin_gn_fwd): same
    numbers as the separate statistics pass over the stored output, for the plain conv and for the conv with the
    previous norm folded into its input."""
    n, ci, co, d, h, w = shape
    x = R.seeded_tensor((n, ci, d, h, w), 821, scale=1.7) + 0.3
    wt = R.seeded_tensor((co, ci, 3, 3, 3), 822, scale=(ci * 27) ** -0.5)
    bias = R.seeded_tensor((co,), 823, scale=0.5)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    y, st = ops.conv3d(x.to(dev), pc, precision=1, gn_groups=32)
    want = ops.groupnorm_stats(y, 32)
    assert torch.equal(y, ops.conv3d(x.to(dev), pc, precision=1))
    assert maxabs(st[:, 0], want[:, 0].cpu()) < 1e-6 and (st[:, 1] / want[:, 1] - 1).abs().max().item() < 1e-5
    ref = F.conv3d(x, wt, bias, padding=1).view(n, 32, -1)
    assert maxabs(st[:, 0], ref.mean(dim=2).reshape(-1)) < 2e-5
    if ops.gn_in_conv_ok(tuple(x.shape), pc) and ci == co:
        g, b = R.seeded_tensor((ci,), 824, scale=0.25, shift=1.0), R.seeded_tensor((ci,), 825, scale=0.25)
        sx = ops.groupnorm_stats(x.to(dev), 32)
        y2, st2 = ops.conv3d_gn_in(x.to(dev), sx, g.to(dev), b.to(dev), 32, pc, out_gn_groups=32)
        want2 = ops.groupnorm_stats(y2, 32)
        assert maxabs(st2[:, 0], want2[:, 0].cpu()) < 1e-6 and (st2[:, 1] / want2[:, 1] - 1).abs().max().item() < 1e-5


@pytest.mark.parametrize("level", [(512, 256, 4, 1, 1, (2, 2, 2)), (256, 128, 8, 2, 2, (2, 2, 2)), (128, 64, 16, 4, 4, (1, 2, 2))],
                         ids=["512-256@4x1x1", "256-128@8x2x2", "128-64@16x4x4"])
def test_flowfield_block_in_two_launches(ops, M, dev, level):
    """FlowField's first three ResBlock3D_Adaptive levels (model.py:369-408 at 439-471) through mphip_flowfield_conv_gn — one workgroup per
    (frame, GroupNorm group) runs conv + statistics + both affines (+ residual 1x1x1 conv) + ReLU + nearest upsample — vs the same block
    evaluated with ATen on the CPU in float64, next to the five-launch path's error; and the module takes that path by itself."""
    ci, co, d, h, w, up = level
    torch.manual_seed(77)
    blk = M.ResBlock3D_Adaptive(ci, co)
    with torch.no_grad():   # non-trivial affines
        for nrm in (blk.norm1, blk.norm2):
            nrm.group_norm.weight.uniform_(0.5, 1.5); nrm.group_norm.bias.uniform_(-0.5, 0.5)
            nrm.weight.uniform_(0.5, 1.5); nrm.bias.uniform_(-0.5, 0.5)
    x = R.seeded_tensor((3, ci, d, h, w), 861, scale=1.7)

    def ref(dt):
        c = lambda t: t.detach().to(dt)
        agn = lambda y, nrm: F.group_norm(y, 32, c(nrm.group_norm.weight), c(nrm.group_norm.bias), 1e-5) * c(nrm.weight) + c(nrm.bias)
        y = F.relu(agn(F.conv3d(x.to(dt), c(blk.conv1.weight), c(blk.conv1.bias), padding=1), blk.norm1))
        y = agn(F.conv3d(y, c(blk.conv2.weight), c(blk.conv2.bias), padding=1), blk.norm2)
        y = F.relu(y + F.conv3d(x.to(dt), c(blk.residual_conv.weight), c(blk.residual_conv.bias)))
        return F.interpolate(y, scale_factor=up, mode="nearest")

    truth, cpu32 = ref(torch.float64), ref(torch.float32).double()
    blk = blk.to(dev).eval()
    assert ops.flowfield_conv_gn_ok(tuple(x.shape), blk.conv1) and ops.flowfield_conv_gn_ok((3, co, d, h, w), blk.conv2, blk.residual_conv)
    with torch.no_grad():
        a = ops.flowfield_conv_gn(x.to(dev), blk.conv1, blk.norm1, relu=True)
        got = ops.flowfield_conv_gn(a, blk.conv2, blk.norm2, res_x=x.to(dev), res_conv=blk.residual_conv, relu=True, up=up).cpu().double()
        assert torch.equal(blk(x.to(dev), _up=up).cpu().double(), got)   # the module's own inference path
        old = ops._FF_FUSED
        ops._FF_FUSED = False
        try:
            five = blk(x.to(dev), _up=up).cpu().double()
        finally:
            ops._FF_FUSED = old
    scale = truth.abs().max().item()
    e_new, e_old, e_cpu = (got - truth).abs().max().item(), (five - truth).abs().max().item(), (cpu32 - truth).abs().max().item()
    print(f"{ci}->{co}: two launches {e_new:.2e}, five launches {e_old:.2e}, ATen fp32 {e_cpu:.2e} (|y|max {scale:.2f})")
    assert got.shape == truth.shape and e_new < max(3.0 * e_cpu, 1e-5 * scale)
    with pytest.raises(RuntimeError):   # not a FlowField level: refused, never computed some other way
        wrong = M.ResBlock3D_Adaptive(64, 32).to(dev)
        ops.flowfield_conv_gn(torch.zeros(1, 64, 16, 8, 8, device=dev), wrong.conv1, wrong.norm1)


def test_flowfield_output_head(ops, M, dev):
    """FlowField's output head (model.py:458-465: Conv3d(32, 3, 3) -> GroupNorm(1, 3) -> ReLU -> tanh) through mphip_flowfield_out (a direct
    3-channel conv + one normalising pass) vs ATen on the CPU in float64, next to the split-K conv + one-launch GroupNorm it replaces."""
    torch.manual_seed(78)
    ff = M.FlowField()
    with torch.no_grad():
        ff.gn.weight.uniform_(0.5, 1.5); ff.gn.bias.uniform_(-0.5, 0.5)
    x = R.seeded_tensor((3, 32, 16, 16, 16), 871, scale=1.7)
    ref = lambda dt: torch.tanh(F.relu(F.group_norm(F.conv3d(x.to(dt), ff.conv3x3x3.weight.detach().to(dt), ff.conv3x3x3.bias.detach().to(dt),
                                                             padding=1), 1, ff.gn.weight.detach().to(dt), ff.gn.bias.detach().to(dt), 1e-5)))
    truth, cpu32 = ref(torch.float64), ref(torch.float32).double()
    ff = ff.to(dev).eval()
    assert ops.flowfield_out_ok(tuple(x.shape), ff.conv3x3x3)
    with torch.no_grad():
        got = ops.flowfield_out(x.to(dev), ff.conv3x3x3, ff.gn).cpu().double()
        y = ops.conv3d_split(x.to(dev), M._packs.get(ff.conv3x3x3))
        old = ops.groupnorm_small(y, ff.gn.weight, ff.gn.bias, 1, ff.gn.eps, relu=True, tanh=True).cpu().double()
    e_new, e_old, e_cpu = (got - truth).abs().max().item(), (old - truth).abs().max().item(), (cpu32 - truth).abs().max().item()
    print(f"output head: two launches {e_new:.2e}, split-K conv + GroupNorm {e_old:.2e}, ATen fp32 {e_cpu:.2e}")
    assert got.shape == truth.shape and e_new < max(3.0 * e_cpu, 1e-6)
    assert (got >= 0).all() and (got < 1).all()   # [0, 1): what makes the reference's warps sample the low corner


def test_cross_reenactment_equals_pairwise(M, dev, hot):
    """BASELINE config 5 (1 source x N drivers, dp.cross_reenact): the source-side half is computed once,
    results must equal running the hot slice on every (source, driver) pair."""
    from megaportrait_hack_amd import dp

    n_drv = 5
    src = {k: v.to(dev) for k, v in R.seeded_hot_inputs(1, 31).items()}
    drv = {k: v.to(dev) for k, v in R.seeded_hot_inputs(n_drv, 32).items()}
    with torch.no_grad():
        fast = dp.cross_reenact(hot, src["vs"], src["es"], src["Rs"], src["ts"], src["zs"], drv["Rd"], drv["td"], drv["zd"], chunk=2)
        rep = lambda t: t.expand(n_drv, *t.shape[1:]).contiguous()
        slow = hot(vs=rep(src["vs"]), es=rep(src["es"]), Rs=rep(src["Rs"]), ts=rep(src["ts"]), zs=rep(src["zs"]),
                   Rd=drv["Rd"], td=drv["td"], zd=drv["zd"])
        assert fast.shape == slow.shape == (n_drv, 96, 64, 64)
        assert (fast - slow).abs().max().item() < 2e-4
        # sharded by driver frame over 2 ranks: concatenation of the shards == unsharded
        parts = [dp.cross_reenact(hot, src["vs"], src["es"], src["Rs"], src["ts"], src["zs"], drv["Rd"], drv["td"], drv["zd"],
                                  rank=r, world=2) for r in range(2)]
        assert (torch.cat(parts, dim=0) - fast).abs().max().item() < 2e-4


def test_config5_cross_reenactment_1024_drivers_8_ranks(M, dev, hot, sd):
    """BASELINE config 5 at its own size: 1 source x 1024 driver frames sharded by driver frame over 8 (virtual) ranks.
    (a) concatenating the 8 rank shards == the unsharded run, bit for bit (same kernels, same chunking grid);
    (b) sampled drivers across the range (incl. shard boundaries) against the CPU ORACLE run pairwise on
        (source, driver) — not against another HIP path."""
    from megaportrait_hack_amd import dp

    n_drv, world = 1024, 8
    src = {k: v.to(dev) for k, v in R.seeded_hot_inputs(1, 31).items()}
    drv_cpu = R.seeded_hot_inputs(n_drv, 33, D=1, H=1, W=1)      # only Rd/td/zd are used (tiny volumes keep this cheap)
    drv = {k: drv_cpu[k].to(dev) for k in ("Rd", "td", "zd")}
    args = (hot, src["vs"], src["es"], src["Rs"], src["ts"], src["zs"], drv["Rd"], drv["td"], drv["zd"])
    full = dp.cross_reenact(*args, chunk=16)
    assert full.shape == (n_drv, 96, 64, 64) and torch.isfinite(full).all()
    parts = [dp.cross_reenact(*args, rank=r, world=world, chunk=16) for r in range(world)]
    assert [p.shape[0] for p in parts] == [128] * 8
    assert torch.equal(torch.cat(parts, dim=0), full)
    src_cpu = R.seeded_hot_inputs(1, 31)
    for i in (0, 127, 128, 517, 1023):
        want = R.hot_slice(vs=src_cpu["vs"], es=src_cpu["es"], Rs=src_cpu["Rs"], ts=src_cpu["ts"], zs=src_cpu["zs"],
                           Rd=drv_cpu["Rd"][i:i + 1], td=drv_cpu["td"][i:i + 1], zd=drv_cpu["zd"][i:i + 1], sd=sd)
        err = maxabs(full[i:i + 1], want)
        assert err < 1e-3, (i, err)


# ------------------------------------------------------------------------------- blocks / graph
def test_resblocks_golden(M, dev, hot):
    g = gold("resblocks")
    x8 = R.seeded_tensor((1, 96, 8, 8, 8), 106, scale=1.7).to(dev)
    with torch.no_grad():
        assert maxabs(hot.G3d.downsampling[0](x8), g["rb_96_96"]) < 1e-4
        assert maxabs(hot.G3d.downsampling[2](x8), g["rb_96_192"]) < 1e-4
        x64 = R.seeded_tensor((1, 64, 8, 8, 8), 107, scale=1.7).to(dev)
        assert maxabs(hot.warp_generator_s2c.flowfield.resblock4(x64), g["rba_64_32"]) < 1e-4


def test_flowfield_golden(dev, hot):
    zsum = R.seeded_tensor((2, 512), 103, scale=20.0).to(dev)
    with torch.no_grad():
        got = hot.warp_generator_s2c.flowfield(zsum.unsqueeze(-1).unsqueeze(-1), 0, 0)
    assert got.shape == (2, 3, 16, 16, 16)
    assert maxabs(got, gold("flowfield")["out"]) < 1e-4


def test_warp_generators_golden(dev, hot):
    g = gold("warp_generator")
    inp = {k: v.to(dev) for k, v in R.seeded_hot_inputs(1, INPUT_SEED).items()}
    with torch.no_grad():
        w1 = hot.warp_generator_s2c(inp["Rs"], inp["ts"], inp["zs"], inp["es"])
        w2 = hot.warp_generator_c2d(inp["Rd"], inp["td"], inp["zd"], inp["es"])
    assert w1.shape == (1, 3, 64, 64, 64)
    assert maxabs(w1[:, :, ::4, ::4, ::4], g["s2c_s4"]) < 1e-4
    assert maxabs(w2[:, :, ::4, ::4, ::4], g["c2d_s4"]) < 1e-4


def test_g3d_golden(dev, hot, sd):
    g = gold("g3d")
    with torch.no_grad():
        x8 = R.seeded_tensor((1, 96, 8, 8, 8), 106, scale=1.7)
        assert maxabs(hot.G3d(x8.to(dev)), g["small"]) < 1e-3
        x16 = R.seeded_tensor((2, 96, 16, 16, 16), 108, scale=1.7)
        got = hot.G3d(x16.to(dev))
        assert maxabs(got[:, :, ::2, ::2, ::2], g["mid_s2"]) < 1e-3
        assert maxabs(got, R.g3d(x16, sd)) < 1e-3


def _sha1(t):
    import hashlib

    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def test_full_size_goldens_of_the_reference(dev, hot, ops):
    """The full-size (96x16x64x64) fixtures oracle/make_golden.py captured from the imported reference, through the
    HIP path end to end (HIP S2C generator -> K2 -> G3d): warp #1 vs the strided samples / per-channel sums (and the
    reference's sha1 whenever the HIP generator happens to reproduce the reference field's bits), G3d vs `full_s4`,
    the per-channel means and the per-channel abs-max of the reference's output."""
    ga, gg, gw = gold("apply_warping_field"), gold("g3d"), gold("warp_generator")
    inp = {k: v.to(dev) for k, v in R.seeded_hot_inputs(1, INPUT_SEED).items()}
    with torch.no_grad():
        w1 = hot.warp_generator_s2c(inp["Rs"], inp["ts"], inp["zs"], inp["es"])
        vc = ops.warp_volume(inp["vs"], w1)
        # the HIP field and the reference's differ by fp32 rounding of FlowField's convs (~5e-6, each ~2-4e-6 from a float64 evaluation:
        # tools/ff_accuracy.py); a sample of |vs| <= 3 moves by that times the local slope — 1e-5 was inside that noise (r03: 1.1e-5 with one
        # summation order of the fused blocks, 0.9e-5 with another)
        assert maxabs(vc[:, :, ::2, ::4, ::4], ga["full_s4"]) < 3e-5
        assert np.abs(vc.double().sum(dim=(2, 3, 4)).cpu().numpy() - ga["full_chan_sum"]).max() < 1e-2  # sums of 65 536 values
        field_bits_equal = _sha1(w1) == str(gw["s2c_sha1"])
        if field_bits_equal:   # FlowField's convs reproduce ATen's bits only by luck; the warp itself is bit-exact (below)
            assert _sha1(vc) == str(ga["full_sha1"])
        vc2d = hot.G3d(vc)
        assert maxabs(vc2d[:, :, ::2, ::4, ::4], gg["full_s4"]) < 1e-3
        assert np.abs(vc2d.double().mean(dim=(2, 3, 4)).cpu().numpy() - gg["full_chan_mean"]).max() < 1e-4
        assert np.abs(vc2d.abs().amax(dim=(2, 3, 4)).cpu().numpy() - gg["full_chan_absmax"]).max() < 1e-3


def test_k2_full_size_bit_exact_vs_reference_sha1(dev, ops, sd):
    """`apply_warping_field.npz["full_sha1"]` = sha1 of the REFERENCE's apply_warping_field(vs, w_s2c) at 96x16x64x64.
    Feeding K2 the bit-identical field (the oracle restatement's S2C field — torch.equal to the reference's in the build
    container, tests/test_oracle.py) must reproduce every output bit when this host's ATen CPU kernels produce the
    golden's field bits; on hosts whose oneDNN/ATen rounds FlowField's convs differently the field sha1 differs and the
    test falls back to bit-equality with the C oracle's warp of that same field."""
    ga, gw = gold("apply_warping_field"), gold("warp_generator")
    inp = R.seeded_hot_inputs(1, INPUT_SEED)
    with torch.no_grad():
        w1 = R.warp_generator(inp["Rs"], inp["ts"], inp["zs"], inp["es"], sd, "warp_generator_s2c.", invert=True)
        vc = ops.warp_volume(inp["vs"].to(dev), w1.to(dev))
    if _sha1(w1) == str(gw["s2c_sha1"]):
        assert _sha1(vc) == str(ga["full_sha1"]), "K2 differs from the reference's apply_warping_field at full size"
    else:
        assert torch.equal(vc.cpu(), R.apply_warping_field(inp["vs"], w1)) or maxabs(vc, R.apply_warping_field(inp["vs"], w1)) < 1e-6
    # (this host's field differs from the golden's in the last bits when its ATen rounds FlowField's convs differently)
    assert maxabs(vc[:, :, ::2, ::4, ::4], ga["full_s4"]) < 1e-4


def test_eapp_tail_golden_and_full_size(M, dev):
    """Scope row f1: Eapp's 3D tail (model.py:271-290) through the same HIP kernels, reference key names."""
    sd_t = R.seeded_state_dict(R.eapp_tail_shapes(), WEIGHT_SEED + 10, "appearanceEncoder.")
    tail = M.Eapp3DTail()
    tail.load_state_dict({k[len("appearanceEncoder."):]: v for k, v in sd_t.items()}, strict=True)
    tail = tail.to(dev).eval()
    feat = R.seeded_tensor((1, 1536, 16, 16), 110, scale=1.7)
    with torch.no_grad():
        got = tail(feat.to(dev))
        assert got.shape == (1, 96, 16, 16, 16)
        assert maxabs(got[:, :, ::2, ::2, ::2], gold("eapp_tail")["out_s2"]) < 1e-3
        # full 512^2 size: [1,1536,64,64] -> 96x16x64x64 volume, 391 GFLOP, vs the ATen-CPU oracle
        feat_full = R.seeded_tensor((1, 1536, 64, 64), 111, scale=1.7)
        err = maxabs(tail(feat_full.to(dev)), R.eapp_tail3d(feat_full, sd_t))
        print(f"Eapp 3D tail full size max-abs vs oracle = {err:.3e}")
        assert err < 1e-3


def test_g2d_head_fused_golden(M, dev):
    """Row f3: G2d's two stacked 1x1 convs (model.py:756-757) as one 96->512 product vs the reference's own modules
    (golden), vs the oracle at the full 64x64 map, and vs the unfused differentiable path."""
    sd = R.seeded_state_dict(R.g2d_head_shapes(), WEIGHT_SEED + 20, "G2d.")
    head = M.G2dHead()
    head.load_state_dict({k[len("G2d."):]: v for k, v in sd.items()})
    head = head.to(dev).eval()
    x = R.seeded_tensor((2, 96, 16, 16), 120, scale=2.0)
    with torch.no_grad():
        got = head(x.to(dev))
    assert got.shape == (2, 512, 16, 16)
    assert maxabs(got, gold("g2d_head")["out"]) < 1e-4       # reassociated (W2 W1) x: not bitwise, far inside 1e-3
    xf = R.seeded_tensor((2, 96, 64, 64), 121, scale=2.0)
    with torch.no_grad():
        fused = head(xf.to(dev))
    assert maxabs(fused, R.g2d_head(xf, sd)) < 1e-4
    xg = xf.to(dev).requires_grad_(True)
    unfused = head(xg)                                        # autograd on: the two convs run separately
    assert maxabs(unfused, fused.cpu()) < 1e-4
    cpu = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xc = xf.clone().requires_grad_(True)
    dy = R.seeded_tensor((2, 512, 64, 64), 122)
    R.g2d_head(xc, cpu).backward(dy)
    unfused.backward(dy.to(dev))
    rel = lambda a, b: (a.detach().cpu().double() - b.double()).abs().max().item() / b.abs().max().item()
    assert rel(xg.grad, xc.grad) < 1e-4
    for n, p in head.named_parameters():
        assert rel(p.grad, cpu["G2d." + n].grad) < 1e-4, n


def test_hot_slice_small_golden(dev, hot):
    inp = {k: v.to(dev) for k, v in R.seeded_hot_inputs(1, INPUT_SEED + 1, D=16, H=16, W=16).items()}
    with torch.no_grad():
        got = hot.forward_any_size(**inp)
    assert maxabs(got, gold("hot_slice")["small16"]) < 1e-3


def test_hot_slice_256px_config(dev, hot, sd):
    """BASELINE config 1 (256x256 frames -> 96x16x32x32 volume): the reference's Gbase.forward trips its 512^2-only
    assert there (model.py:1157); `forward_any_size` runs the same graph, checked against the CPU oracle."""
    inp = R.seeded_hot_inputs(2, 41, D=16, H=32, W=32)
    with torch.no_grad():
        got = hot.forward_any_size(**{k: v.to(dev) for k, v in inp.items()})
    want = R.hot_slice(sd=sd, **inp)
    assert got.shape == (2, 96, 32, 32)
    assert maxabs(got, want) < 1e-3


def test_hot_slice_batches_beyond_one_pass(dev, hot, M, monkeypatch):
    """Maximum sizes: the conv kernels address their input through one 2 GiB buffer resource (85 frames of the BASELINE volume);
    a larger inference batch runs as consecutive passes (`max_frames_per_pass`, default 64) with the same results — here with the
    limit lowered to 2 on a 5-frame batch; under autograd the batch is never split."""
    inp = {k: v.to(dev) for k, v in R.seeded_hot_inputs(5, 47, D=16, H=16, W=16).items()}
    with torch.no_grad():
        whole = hot.forward_any_size(**inp)
        monkeypatch.setattr(type(hot), "max_frames_per_pass", 2)
        split = hot.forward_any_size(**inp)
    assert split.shape == whole.shape
    assert maxabs(split, whole.cpu()) < 2e-4    # (not bitwise: the split-K plan of the small-volume convs depends on the batch size)
    tail = M.Eapp3DTail().to(dev).eval()
    x = R.seeded_tensor((3, 96, 4, 8, 8), 48).to(dev)
    with torch.no_grad():
        a = tail(x)
        monkeypatch.setattr(M.Eapp3DTail, "max_frames_per_pass", 1)
        b = tail(x)
    assert maxabs(a, b.cpu()) < 2e-4
    grad_in = {k: v.clone().requires_grad_(True) for k, v in inp.items()}
    out = hot.forward_any_size(**grad_in)       # autograd: one pass, gradients for all 5 frames
    out.sum().backward()
    assert grad_in["vs"].grad.shape == inp["vs"].shape and float(grad_in["vs"].grad[4].abs().max()) > 0


def test_hot_slice_accepts_strided_and_half_inputs(dev, hot):
    """What upstream PyTorch modules hand over: non-contiguous views (a channels_last-style permute, an expanded batch) and
    fp16 / bf16 tensors from an autocast region (train.py:188) — made contiguous fp32 at the boundary, same results."""
    inp = {k: v.to(dev) for k, v in R.seeded_hot_inputs(2, 49, D=16, H=16, W=16).items()}
    with torch.no_grad():
        want = hot.forward_any_size(**inp)
        strided = dict(inp)
        strided["vs"] = inp["vs"].permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)      # same values, channel-last strides
        strided["es"] = inp["es"][:1].expand(2, -1) * 0 + inp["es"]                               # a fresh, contiguous-by-accident copy
        strided["zs"] = torch.stack([inp["zs"], inp["zs"]], dim=2)[:, :, 0]                        # stride-2 view
        assert not strided["vs"].is_contiguous() and not strided["zs"].is_contiguous()
        got = hot.forward_any_size(**strided)
        assert torch.equal(got, want)
        half = {k: v.half() for k, v in inp.items()}
        got16 = hot.forward_any_size(**half)
        ref16 = hot.forward_any_size(**{k: v.float() for k, v in half.items()})
        assert got16.dtype == torch.float32 and torch.equal(got16, ref16)


def test_hot_slice_full_golden(dev, hot):
    """BASELINE config: 512^2 frame = 96x16x64x64 volume, reference output [1,96,64,64]."""
    g = gold("hot_slice")
    inp = {k: v.to(dev) for k, v in R.seeded_hot_inputs(1, INPUT_SEED).items()}
    with torch.no_grad():
        got = hot(**inp)
    assert got.shape == (1, 96, 64, 64)
    err = maxabs(got, g["full"])
    print(f"full hot slice max-abs vs reference = {err:.3e} (|ref|max = {np.abs(g['full']).max():.2f})")
    assert err < 1e-3


def test_hot_slice_full_size_batch8_vs_oracle(dev, hot):
    """the GRADED batch (B=8 frames of 96x16x64x64) against the CPU oracle DIRECTLY, all eight frames — not
    through properties.  (~7 s of ATen-CPU work on the GPU box's host cores.)"""
    B = 8
    inp = R.seeded_hot_inputs(B, 23)
    with torch.no_grad():
        got = hot(**{k: v.to(dev) for k, v in inp.items()}).cpu()
        want = R.hot_slice(sd=R.seeded_gbase_hot_state_dict(WEIGHT_SEED), **inp)
    assert got.shape == want.shape == (B, 96, 64, 64)
    per_frame = (got - want).abs().flatten(1).max(dim=1).values
    print(f"B=8 full size vs the CPU oracle: per-frame max-abs {[f'{v:.2e}' for v in per_frame.tolist()]} (|ref|max {want.abs().max():.2f})")
    assert per_frame.max().item() < 1e-3


def test_full_size_properties(ops, M, dev, hot):
    """Size-independent properties at BASELINE batch size (B=8, 96x16x64x64)."""
    B = 8
    inp = {k: v.to(dev) for k, v in R.seeded_hot_inputs(B, 21).items()}
    with torch.no_grad():
        out = hot(**inp)
        # (1) frames are independent (no cross-batch op): batch of 8 == 8 batches of 1
        #     (not bitwise: the split-K plan of the small-volume convs depends on the batch size)
        one = hot(**{k: v[3:4] for k, v in inp.items()})
        assert (out[3:4] - one).abs().max().item() < 2e-4
        # (2) the warp is linear in the volume: warp(a*v1 + v2) == a*warp(v1) + warp(v2)
        w = hot.warp_generator_c2d(inp["Rd"], inp["td"], inp["zd"], inp["es"])
        v1, v2 = inp["vs"], torch.flip(inp["vs"], dims=[1])
        lhs = ops.warp_volume_dsum(2.0 * v1 + v2, w)
        rhs = 2.0 * ops.warp_volume_dsum(v1, w) + ops.warp_volume_dsum(v2, w)
        assert (lhs - rhs).abs().max().item() < 2e-4
        # (3) K3 == K2 followed by a depth sum
        assert (ops.warp_volume(v1, w).sum(dim=2) - ops.warp_volume_dsum(v1, w)).abs().max().item() < 2e-4
        # (4) a constant volume is a fixed point of the (border-clamped, partition-of-unity) warp
        const = torch.full_like(v1[:1], 0.75)
        assert (ops.warp_volume(const, w[:1]) - 0.75).abs().max().item() < 1e-6
        # (5) deterministic: same inputs, same bits
        assert torch.equal(out, hot(**inp))


def test_errors_are_loud(ops, M, dev):
    with pytest.raises(RuntimeError):
        ops.warp_volume(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4))       # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        ops.conv3d(torch.zeros(1, 5, 4, 4, 4, device=dev), ops.PackedConv(torch.zeros(4, 6, 3, 3, 3, device=dev), None))
    hot = M.GbaseHotSlice().to(dev)
    bad = {k: v.to(dev) for k, v in R.seeded_hot_inputs(1, 1, D=8, H=8, W=8).items()}
    with torch.no_grad(), pytest.raises(AssertionError):
        hot(**bad)                                       # model.py:1157 shape assert is preserved


def test_empty_frame_shard(hot, dev):
    """More ranks than frames: a rank's shard is empty; the slice returns an empty projection instead of launching."""
    inp = {k: v.to(dev)[:0] for k, v in R.seeded_hot_inputs(1, 3).items()}
    with torch.no_grad():
        out = hot(**inp)
    assert out.shape == (0, 96, 64, 64)


@pytest.mark.parametrize("shape", [(2, 96, 192, 8, 32, 32), (16, 768, 384, 2, 8, 8), (3, 192, 96, 4, 16, 16)])
def test_conv3d_k1_f16x3(ops, dev, shape):
    """The 1x1x1 shortcut convs of G3d (model.py:510) on the split-f16 GEMM kernel (conv3d_k1_f16x3_kernel): forward and
    bwd-data vs float64, no worse than twice the exact fp32 kernel's own rounding; bias; a planted outlier."""
    n, ci, co, d, h, w = shape
    x = R.seeded_tensor((n, ci, d, h, w), 841, scale=1.7)
    x[0, 3, 0, 1, 2] = 3.0e4
    wt = R.seeded_tensor((co, ci, 1, 1, 1), 842, scale=1.0 / ci ** 0.5)
    b = R.seeded_tensor((co,), 843, scale=0.3)
    pc = ops.PackedConv(wt.to(dev), b.to(dev))
    assert ops._lib.load().mphip_conv3d_supported(n, ci, co, d, h, w, 1, 1) == 1
    truth = F.conv3d(x.double(), wt.double(), b.double())
    got = ops.conv3d(x.to(dev), pc, precision=1)
    exact = ops.conv3d(x.to(dev), pc, precision=0)
    scale = truth.abs().max().item()
    e1 = (got.cpu().double() - truth).abs().max().item() / scale
    e0 = (exact.cpu().double() - truth).abs().max().item() / scale
    assert e1 < max(2.0 * e0, 2e-6), (e1, e0)
    dy = R.seeded_tensor((n, co, d, h, w), 844, scale=1e-3)
    _, gs = ops.grad_prep(dy.to(dev), want_bias=False)
    dx = ops.conv3d_bwd_data(dy.to(dev), ops.PackedConv(wt.to(dev), None, transposed=True), gs, precision=1)
    want = torch.nn.grad.conv3d_input(x.shape, wt.double(), dy.double())
    assert (dx.cpu().double() - want).abs().max().item() / want.abs().max().item() < 2e-6


def test_resblock_upsample_branch(ops, M, dev):
    """`upsample=True` of ResBlock3D / ResBlock3D_Adaptive (model.py:404-405, 525-526: F.interpolate(scale_factor, 'trilinear',
    align_corners=False)) — no module of Gbase sets it; covered for constructor parity.  Forward vs the block without the flag
    + ATen's interpolate on the CPU, and the gradient through it vs CPU autograd."""
    x = R.seeded_tensor((1, 96, 4, 8, 8), 851, scale=1.7)
    torch.manual_seed(851)   # (the blocks' default init is random: unseeded, the 1e-6 bar below met |y| > 16 once in ~20 runs)
    for cls, sf in ((M.ResBlock3D, (2, 2, 2)), (M.ResBlock3D_Adaptive, (1, 2, 3))):
        plain, up = cls(96, 96), cls(96, 96, upsample=True, scale_factors=sf)
        up.load_state_dict(plain.state_dict())
        plain, up = plain.to(dev).eval(), up.to(dev).eval()
        with torch.no_grad():
            base = plain(x.to(dev))
            got = up(x.to(dev))
        want = F.interpolate(base.cpu(), scale_factor=sf, mode="trilinear", align_corners=False)
        assert got.shape == want.shape and maxabs(got, want) < 1e-6 + 2.4e-7 * want.abs().max().item()   # <= 2 ulp of the largest value
    y = R.seeded_tensor((2, 8, 3, 4, 6), 852).requires_grad_(True)
    dy = R.seeded_tensor((2, 8, 6, 8, 18), 853)
    F.interpolate(y, scale_factor=(2, 2, 3), mode="trilinear", align_corners=False).backward(dy)
    assert maxabs(ops.upsample_trilinear_bwd(dy.to(dev), (2, 2, 3)), y.grad) < 1e-5
    with pytest.raises(ValueError):
        ops.upsample_trilinear(x.to(dev), (1.5, 2, 2))


def test_f16x3_accepts_any_magnitude(ops, dev):
    """The f16x3 conv scales every operand tensor by its own power of two (range descriptors, include/mphip.h): planted
    outliers far beyond the old fixed-scale cliff (|x| >= 4062), tiny tensors and huge tensors all stay fp32-class, and
    nothing is clamped (saturation count 0) — like the reference's fp32 nn.Conv3d, which has no range cliff."""
    x = R.seeded_tensor((1, 96, 4, 8, 16), 831, scale=1.7)
    w = R.seeded_tensor((96, 96, 3, 3, 3), 832, scale=0.02)
    pc = ops.PackedConv(w.to(dev), None)
    ops.f16x3_saturation_count(reset=True)

    def check(xin, label):
        got = ops.conv3d(xin.to(dev), pc, precision=1)
        truth = F.conv3d(xin.double(), w.double(), None, padding=1)
        exact = ops.conv3d(xin.to(dev), pc, precision=0)
        scale = truth.abs().max().item()
        e1 = (got.cpu().double() - truth).abs().max().item() / scale
        e0 = (exact.cpu().double() - truth).abs().max().item() / scale
        assert e1 < max(2.0 * e0, 2e-6), (label, e1, e0)        # no worse than twice the exact fp32 kernel's own rounding
        return got

    check(x, "O(1)")
    big = x.clone()
    big[0, 5, 2, 3, 7] = 1.0e5                                   # 25x beyond where the fixed scale used to clamp
    check(big, "planted 1e5")
    check(x * 1.0e-6, "tiny tensor")                             # a fixed scale would push the lo halves into f16 subnormals
    check(x * 3.0e7, "huge tensor")
    assert ops.f16x3_saturation_count() == 0
    # a stale range is never used: an in-place write bumps the tensor's version and the descriptor is re-measured
    xd = x.to(dev)
    ops.conv3d(xd, pc, precision=1)
    r0 = ops.tensor_range(xd)
    assert r0 is not None
    xd.mul_(1.0e4)
    assert ops.tensor_range(xd) is None
    y = ops.conv3d(xd, pc, precision=1)
    assert torch.isfinite(y).all() and ops.f16x3_saturation_count() == 0


def test_range_descriptors_are_correct_bounds(ops, dev):
    """What the producers leave in a range descriptor: max over [2] and the partial maxima must equal max|tensor| (K2's fused
    note — staged tiles, the column walk and the direct gather alike —, GroupNorm apply, mphip_absmax_range) or bound it (K2 with
    more tiles than partial slots falls back to the SOURCE volume's maximum — a warp is a convex combination; the affine-table bound of a folded GroupNorm)."""
    def desc_max(r):
        r = r.cpu()
        n = int(r[3:4].view(torch.int32).item())
        assert 0 <= n <= 4096
        return max(r[2].item(), r[4:4 + n].max().item() if n else 0.0)

    x = R.seeded_tensor((2, 96, 4, 8, 16), 861, scale=3.0).to(dev)
    assert desc_max(ops.absmax_range(x)) == x.abs().max().item()
    field = (R.seeded_tensor((2, 3, 64, 64, 64), 862, scale=1.3) + 0.4).to(dev)
    v = R.seeded_tensor((2, 8, 16, 64, 64), 863, scale=2.0).to(dev)
    out = ops.warp_volume(v, field)
    assert desc_max(ops.tensor_range(out)) == out.abs().max().item()          # fused into the gather kernels
    vb = R.seeded_tensor((14, 8, 16, 64, 64), 864, scale=2.0).to(dev)           # 14*16*2 = 448 tiles: one partial slot each
    fb = (R.seeded_tensor((14, 3, 64, 64, 64), 865, scale=1.3) + 0.4).to(dev)
    ob = ops.warp_volume(vb, fb)
    assert desc_max(ops.tensor_range(ob)) == ob.abs().max().item()
    travelling = fb.clone()                                                     # the follow-up kernels fold into the same slots
    travelling[:7, 0] += torch.linspace(0, 50, 64, device=dev).view(1, 1, 1, 64)             # smooth: the column walk
    travelling[7:] = (R.seeded_tensor((7, 3, 64, 64, 64), 868).to(dev) + 1.0) * 30.0         # incoherent: the direct gather
    ot = ops.warp_volume(vb, travelling)
    assert desc_max(ops.tensor_range(ot)) == ot.abs().max().item()
    vc = R.seeded_tensor((129, 2, 16, 64, 64), 869, scale=2.0).to(dev)          # 129*16*2 tiles (32 x 64 positions each) > 4096 partial slots
    fc = (R.seeded_tensor((1, 3, 64, 64, 64), 870, scale=1.3) + 0.4).to(dev).expand(129, -1, -1, -1, -1).contiguous()
    oc = ops.warp_volume(vc, fc)
    m = desc_max(ops.tensor_range(oc))
    assert oc.abs().max().item() <= m == vc.abs().max().item()                 # the source's maximum bounds the warp
    st = ops.groupnorm_stats(x, 32)
    g, b = R.seeded_tensor((96,), 866, scale=0.5, shift=1.0).to(dev), R.seeded_tensor((96,), 867, scale=0.5).to(dev)
    for kw in (dict(relu=True), dict(relu=True, pool2=True), dict(residual=x, relu=False)):
        y = ops.groupnorm_apply(x, st, g, b, 32, **kw)
        assert desc_max(ops.tensor_range(y)) == y.abs().max().item(), kw
    up = ops.upsample_trilinear2(y)
    assert ops.tensor_range(up) is ops.tensor_range(y) and up.abs().max().item() <= desc_max(ops.tensor_range(y)) + 1e-6
    # the folded GroupNorm's data-independent bound really bounds the normalised tensor
    pc = ops.PackedConv(R.seeded_tensor((96, 96, 3, 3, 3), 868, scale=0.02).to(dev), None)
    lib = ops._lib.load()
    table = torch.empty((2, 96, 2), device=dev)
    rng = ops.new_range(dev)
    ops._lib.check(lib.mphip_groupnorm_affine_table(ops._ptr(st), ops._ptr(g), ops._ptr(b), None, None, ops._ptr(table), ops._ptr(rng), 2, 96,
                                                    4 * 8 * 16, 32, ops._stream()), "affine_table")
    normed = ops.groupnorm_apply(x, st, g, b, 32, relu=False)
    assert normed.abs().max().item() <= desc_max(rng) and desc_max(rng) < 1e3
    del pc


def test_f16x3_propagates_non_finite(ops, dev):
    """Inf / NaN inputs are not clamped to finite values: they reach the output as Inf/NaN exactly where the
    fp32 reference conv puts them, forward and backward (an overflowed gradient must stay visible to GradScaler,
    train.py:145,318-320), and the diagnostic counter sees them."""
    x = R.seeded_tensor((1, 96, 4, 8, 16), 833, scale=1.7)
    w = R.seeded_tensor((96, 96, 3, 3, 3), 834, scale=0.02)
    pc = ops.PackedConv(w.to(dev), None)
    for bad in (float("nan"), float("inf")):
        xb = x.clone()
        xb[0, 7, 1, 4, 9] = bad
        ops.f16x3_saturation_count(reset=True)
        got = ops.conv3d(xb.to(dev), pc, precision=1).cpu()
        want = F.conv3d(xb, w, None, padding=1)
        assert torch.equal(torch.isfinite(got), torch.isfinite(want))          # the same voxels are poisoned, no others
        assert (got[torch.isfinite(want)] - want[torch.isfinite(want)]).abs().max().item() < 1e-4
        assert ops.f16x3_saturation_count(reset=True) >= 1
        # backward: a non-finite dy poisons dx and dw instead of being clamped
        dyb = x.clone()
        dyb[0, 3, 2, 2, 2] = bad
        _, scale = ops.grad_prep(dyb.to(dev), want_bias=False)
        dw = ops.conv3d_bwd_weight(x.to(dev), dyb.to(dev), 3, dy_scale=scale, precision=1)
        assert not torch.isfinite(dw[3]).all() and torch.isfinite(dw[4]).all()
        pt = ops.PackedConv(w.to(dev), None, transposed=True)
        dx = ops.conv3d_bwd_data(dyb.to(dev), pt, scale, precision=1)
        assert not torch.isfinite(dx).all()


def test_hot_slice_with_framework_initialisation(dev, M, ops):
    """VERDICT r2 "what's weak" (ii): every other fixture draws its weights from the integer PRNG at O(1) magnitude.  Here the modules
    keep PyTorch's own initialisation — kaiming-uniform convs of magnitude 1/sqrt(fan_in), unit GroupNorm affines: what the reference
    starts training from (its constructors, model.py:369-408, 500-523, 927-957) — and the inputs have the small magnitudes of encoder
    outputs.  Full size, one frame, against the CPU oracle in fp32 (the bar) and in float64 (whose rounding is whose)."""
    torch.manual_seed(20240917)
    hot = M.GbaseHotSlice()
    sd = {k: v.detach().clone() for k, v in hot.state_dict().items()}
    hot = hot.to(dev).eval()
    g = torch.Generator().manual_seed(5)
    inp = dict(vs=0.3 * torch.randn(1, 96, 16, 64, 64, generator=g), es=0.5 * torch.randn(1, 512, generator=g),
               zs=0.5 * torch.randn(1, 512, generator=g), zd=0.5 * torch.randn(1, 512, generator=g),
               Rs=torch.rand(1, 3, generator=g) * 40 - 20, Rd=torch.rand(1, 3, generator=g) * 40 - 20,
               ts=0.05 * torch.randn(1, 3, generator=g), td=0.05 * torch.randn(1, 3, generator=g))
    ops.f16x3_saturation_count(reset=True)
    with torch.no_grad():
        got = hot(**{k: v.to(dev) for k, v in inp.items()}).cpu().double()
        cpu32 = R.hot_slice(sd=sd, **inp).double()
        truth = R.hot_slice(sd={k: v.double() for k, v in sd.items()}, **{k: v.double() for k, v in inp.items()})
    scale = truth.abs().max().item()
    e_bar, e_hip, e_cpu = (got - cpu32).abs().max().item(), (got - truth).abs().max().item(), (cpu32 - truth).abs().max().item()
    print(f"default init: |out|max {scale:.3e}; HIP vs fp32 oracle {e_bar:.3e}; vs float64: HIP {e_hip:.3e}, fp32 oracle {e_cpu:.3e}")
    assert scale > 1e-3, "degenerate output: the test would be vacuous"
    assert e_bar < 1e-3
    assert e_hip < max(3.0 * e_cpu, 2e-5 * scale)
    assert ops.f16x3_saturation_count() == 0


def test_hot_slice_with_unnormalised_activations(dev, hot, sd, M, ops):
    """G3d's first conv and Eapp's tail see UN-normalised activations of a trained checkpoint.  Plant 1e5
    in `vs` (inside the 4^3 corner the reference's warp samples) and scale Eapp's input by 1e4: the f16x3 path stays within
    the fp32 reference's own rounding of these ill-scaled problems (both measured against a float64 evaluation of the
    oracle) and never saturates."""
    inp = R.seeded_hot_inputs(1, INPUT_SEED)
    inp["vs"] = inp["vs"].clone()
    inp["vs"][0, 5, 1, 2, 3] = 1.0e5
    ops.f16x3_saturation_count(reset=True)
    with torch.no_grad():
        got = hot(**{k: v.to(dev) for k, v in inp.items()}).cpu().double()
        truth = R.hot_slice(sd={k: v.double() for k, v in sd.items()}, **{k: v.double() for k, v in inp.items()})
        cpu32 = R.hot_slice(sd=sd, **inp).double()
    e_hip, e_cpu = (got - truth).abs().max().item(), (cpu32 - truth).abs().max().item()
    print(f"planted 1e5 in vs: HIP {e_hip:.3e}  fp32 CPU oracle {e_cpu:.3e} vs float64 (|out|max {truth.abs().max():.2f})")
    assert e_hip < max(1e-3, 3.0 * e_cpu)
    assert ops.f16x3_saturation_count() == 0
    sd_t = R.seeded_state_dict(R.eapp_tail_shapes(), WEIGHT_SEED + 10, "appearanceEncoder.")
    tail = M.Eapp3DTail()
    tail.load_state_dict({k[len("appearanceEncoder."):]: v for k, v in sd_t.items()}, strict=True)
    tail = tail.to(dev).eval()
    feat = R.seeded_tensor((1, 1536, 16, 16), 110, scale=1.7) * 1.0e4
    with torch.no_grad():
        got = tail(feat.to(dev)).cpu().double()
        truth = R.eapp_tail3d(feat.double(), {k: v.double() for k, v in sd_t.items()})
        cpu32 = R.eapp_tail3d(feat, sd_t).double()
    e_hip, e_cpu = (got - truth).abs().max().item(), (cpu32 - truth).abs().max().item()
    print(f"Eapp tail on 1e4-scaled input: HIP {e_hip:.3e}  fp32 CPU oracle {e_cpu:.3e} vs float64")
    assert e_hip < max(1e-3, 3.0 * e_cpu)
    assert ops.f16x3_saturation_count() == 0


def test_hot_slice_invariant_to_a_groupnorm_offset(dev, hot, sd, M, monkeypatch):
    """Metamorphic: one constant c added to the bias of every conv whose output goes straight into a GroupNorm / AdaptiveGroupNorm (G3d's
    ResBlock3D conv1/conv2, the generators' ResBlock3D_Adaptive conv1/conv2, FlowField's output conv) leaves the reference's output
    unchanged in exact arithmetic.  c puts those layers at |mean| / sigma ~ 100, where a one-pass fp32 E[x^2] - mean^2 loses the
    variance.  HIP(shifted) must match the float64 oracle of the shifted slice and HIP(unshifted) to the fp32 oracle's own class."""
    import re

    keys = [k for k in sd if re.search(r"(G3d\.(down|up)sampling\.\d+\.conv[12]|flowfield\.resblock\d\.conv[12]|flowfield\.conv3x3x3)\.bias$", k)]
    assert len(keys) == 32
    inp = R.seeded_hot_inputs(2, INPUT_SEED)
    record = {}

    def run_oracle(sd_, dt):
        targets = {id(sd_[k]): k for k in keys}
        conv = R._conv3d

        def spy(x, w, b=None, *a, **kw):
            y = conv(x, w, b, *a, **kw)
            if b is not None and id(b) in targets:
                yr = y.detach().double().reshape(y.shape[0] * (1 if y.shape[1] == 3 else 32), -1)
                record[targets[id(b)]] = (yr.mean(-1).abs() / yr.std(-1, unbiased=False)).median().item(), yr.std(-1, unbiased=False).median().item()
            return y

        monkeypatch.setattr(R, "_conv3d", spy)
        try:
            with torch.no_grad():
                return R.hot_slice(sd=sd_, **{k: v.to(dt) for k, v in inp.items()})
        finally:
            monkeypatch.setattr(R, "_conv3d", conv)

    base32 = run_oracle(sd, torch.float32)
    c = 100.0 * max(sig for _, sig in record.values())
    sd_s = dict(sd)
    for k in keys:
        sd_s[k] = sd[k] + c
    cpu32 = run_oracle(sd_s, torch.float32).double()
    truth = run_oracle({k: v.double() for k, v in sd_s.items()}, torch.float64)
    print(f"offset c = {c:.3g}; |mean|/sigma per layer: " + ", ".join(f"{k.replace('.bias', '')} {r:.0f}" for k, (r, _) in sorted(record.items())))
    shifted = M.GbaseHotSlice()
    M.load_hot_state_dict(shifted, sd_s)
    shifted = shifted.to(dev).eval()
    with torch.no_grad():
        got = shifted(**{k: v.to(dev) for k, v in inp.items()}).cpu().double()
        plain = hot(**{k: v.to(dev) for k, v in inp.items()}).cpu().double()
    e_hip, e_cpu, e_inv = (got - truth).abs().max().item(), (cpu32 - truth).abs().max().item(), (got - plain).abs().max().item()
    print(f"shifted slice: HIP {e_hip:.3e}, fp32 CPU oracle {e_cpu:.3e} vs float64; HIP shifted vs unshifted {e_inv:.3e}; fp32 oracle shifted vs "
          f"unshifted {(cpu32 - base32.double()).abs().max().item():.3e} (|out|max {truth.abs().max():.2f})")
    assert min(r for r, _ in record.values()) > 30
    assert e_hip <= max(3.0 * e_cpu, 1e-5)
    assert e_inv <= max(3.0 * e_cpu, 1e-5)


def test_c_abi_from_plain_c(c_abi_exe):
    """tests/c_abi/c_abi_smoke.c: a C99 program (gcc; HIP runtime for memory, no Python/torch) drives libmphip.so through
    include/mphip.h — conv + pool vs host references computed in the C file, and the error-code convention."""
    import subprocess

    r = subprocess.run([c_abi_exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "C ABI OK" in r.stdout


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs on the node (the gpurun boxes have one)")
def test_bench_two_ranks_over_rccl():
    """`bench.py --gpus 2` end to end over RCCL (self-launch, one rank per GPU, barrier + MAX over ranks):
    runs wherever a node has two GPUs; the 1-GPU boxes of this pool skip it (the launch path itself is covered on the
    CPU with gloo: tests/test_host.py::test_bench_self_launches_ranks)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--no-extras",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and line["scaling"] == "weak"
    assert line["config"]["global_batch"] == 16 and line["value"] > 0


def test_end_to_end_autocast_leg_has_a_floor():
    """the `end_to_end_autocast_fp16` leg of the bench line (gbase.Gbase.forward under torch.autocast(float16), B = 8) read 114
    frames/s in r04 and 71 in r05.  Root cause (profiles/NOTES_r06.md §1): GPU_MAX_HW_QUEUES=8, which bench.py / the reenact CLI used to
    request — a plan whose side stream landed on a hardware queue that goes idle between steps paid a scheduling delay on each of its 36
    dependent generator launches, +28 ms per step; which plan did depended on the legs run before.  Nothing in the repository raises the
    variable any more.  This test runs the legs of the slow sequence (a graphed training step, then the fp32 leg) in a fresh process with
    the default environment and holds the autocast leg to >= 100 frames/s (68 ms per step = 118 measured)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import os, sys, json, torch; sys.path.insert(0, %r); import bench; dev = torch.device('cuda:0'); "
            "assert 'GPU_MAX_HW_QUEUES' not in os.environ; bench.train_leg(dev, autocast=True); bench.end_to_end(dev, 8, steps=3, warmup=1); "
            "assert 'GPU_MAX_HW_QUEUES' not in os.environ; print('LEG ' + json.dumps(bench.end_to_end(dev, 8, steps=5, warmup=2, fp16=True)))" % root)
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    leg = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")][-1][4:])
    print("end_to_end_autocast_fp16:", leg["value"], "frames/s,", leg["ms_per_step"], "ms per step")
    assert leg["value"] >= 100.0, leg


def test_bench_line_contract_on_one_gpu():
    """`python bench.py --gpus 1 --steps K --warmup W --full` (the driver's call with --full, and a small K): ONE JSON line with the
    contract's keys, the default loop (two batches in flight, one plan per stream), the dominant kernel's roofline quoted from the
    one-stream leg of the same run with the two-batch reading beside it, and the legs a one-second extras budget still admits."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--full",
                        "--no-cpu-baseline", "--extras-budget", "1", "--repeats", "2"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline"):
        assert key in line, key
    assert line["n_gpus"] == 1 and line["steps"] == 4 and line["warmup"] == 2 and line["unit"] == "frames/s" and line["value"] > 0
    assert abs(line["value"] - 8 * 4 / (line["ms_per_step"] * 4e-3)) / line["value"] < 1e-2      # value = frames of the K steps / their time
    assert line["higher_is_better"] is True and line["scaling"] == "weak" and line["vs_baseline"] is None and line["data"] == "synthetic"
    assert "workload" in line["config"] and line["config"]["batches_in_flight"] == 2 and line["config"]["frames_per_gpu_per_step"] == 8
    roof = line["roofline"]
    assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and roof["peak"] == 2500.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3 and 0.05 < roof["frac"] < 0.5
    assert abs(roof["achieved"] - roof["flops_per_launch"] / (roof["launch_ms"] * 1e-3) / 1e12) / roof["achieved"] < 1e-2
    one = line["one_in_flight"]
    # (the events of the timed region come from ONE of the two plans: its 2 of the 4 steps, two full-size launches each)
    # the line's primary figures are those of the loop `value` was measured in; the one-stream (isolated) launch stands beside them
    assert roof["in_two_batch_loop"]["launches_timed"] == 4 and roof["in_two_batch_loop"]["launch_ms"] == roof["launch_ms"]
    assert one["dominant_conv"]["launch_ms"] == roof["isolated_one_stream"]["launch_ms"] <= roof["launch_ms"] * 1.05
    assert one["value"] > 0 and one["step_ms"]["min"] <= one["step_ms"]["median"] <= one["step_ms"]["max"]
    assert roof["demand_driven_launch"]["launches_timed"] == 2
    # the graded shape runs in the F(2,3) domain: 2 f16 FLOPs issued per algorithmic FLOP (3 split products x 2/3)
    assert "wino" in roof["kernel"] and roof["f16_flops_issued_per_algorithmic_flop"] == 2.0
    # counters are quoted only when stamped with the sources of this build (tools/collect_profiles.sh)
    assert (roof["traffic"] is None) == bool(roof["stale"])
    reps = line["repeats"]
    assert len(reps["ms_per_step"]) == 2 and reps["min"] <= reps["median"] <= reps["max"]
    assert "hot_slice_tflops" not in line and line["hot_slice_tflops_executed"] < line["hot_slice_tflops_reference_graph"]


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain `python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: the headline line and nothing that needs runs of its
    own (no repeat blocks, side legs or CPU baseline: those are --full's), and DIR/hot_slice.npy = what the last of the K steps
    returned — the same bits on a second run with the same arguments (seeded inputs and weights)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["unit"] == "frames/s"
        assert abs(line["value"] - 8 * 3 / (line["ms_per_step"] * 3e-3)) / line["value"] < 1e-2
        assert line["repeats"] is None and "roofline" in line
        assert not {"one_in_flight", "cpu_baseline", "fp32_exact", "end_to_end", "leg_seconds"} & set(line)
        assert sorted(os.listdir(tmp_path / run)) == ["hot_slice.npy"]
        out = np.load(tmp_path / run / "hot_slice.npy")
        assert out.dtype == np.float32 and out.shape == (8, 96, 64, 64) and np.isfinite(out).all()
        outs.append(out)
    assert np.array_equal(outs[0], outs[1])
