"""Every branch of the warps' backward (csrc/warp_bwd.hip, K10 of include/mphip.h, through the wrappers ops.warp_volume_bwd,
ops.warp_sample_box, ops.warp_field_compose_bwd and ops.rt_theta_bwd) and K2's forward with more than one tile column, each reached
on purpose.  A case id names the branch it reaches.

Reference and bar of every gradient (and of the forward values the autograd Functions return):
 * g64 = CPU autograd of the operation restated in float64 (`_warp_op`, `_compose_op`, `_theta_op`: the lines of oracle/hotpath_ref.py's
   apply_warping_field / warp_generator / affine_theta, whose fp32 constants — torch.linspace, torch.eye — would pull a double input back
   to fp32).  The linspace tables are INPUTS of the kernels (lin_d / lin_h / lin_w), so the float64 restatement uses the same fp32 table
   values, widened.
 * g32 = the same restatement in fp32 on the CPU: ATen's own gradient, what the reference computes.
 * max|got - g64| <= 4 * max|g32 - g64| + 2^-22 * max|g64|.  4 is the project's rule for a different summation order
   (tests/test_gpu_conv2d_f16x3.py); 2^-22 is four fp32 roundings per product (three weight factors and the product), the floor where
   ATen happens to be exact.  No constant here was tuned against the kernels.
The three numbers are printed per case; with MPHIP_PARITY_JSON=<file> the worst err / bound of every test goes to that file
(profiles/warp_bwd_branches.json holds one MI355X run).

Quiet inputs (a condition on the inputs, not a tolerance): the field gradient is discontinuous where a sample crosses an integer plane, so
every warp case first asserts on the CPU that the fp32 and the float64 evaluation of the coordinates agree at every sample and axis on
the floor index and on the clip decision, and that no unclipped coordinate lies within 1e-3 of an integer.  No sample is left out of a
comparison.  A field of the volume's own size makes the align_corners=True resize the identity, so `target - linspace` puts every
coordinate where the case wants it: an integer base plus a seeded fraction in [0.25, 0.75]; at or below -0.5 / at or above S - 0.5 for
clipped samples; exactly 0.0 or S - 1 for border hits (S - 1 only where linspace is -1 or 1, so that linspace + field is exact).  Resized
fields are an affine field (which the resize reproduces) plus seeded noise of bounded amplitude.

A size-1 axis (D = 1): the reference's chain divides by S - 1 = 0; ATen's forward clips the NaN to coordinate 0 and so do the kernels,
but ATen's backward keeps the NaN (every gradient of the frame comes out 0 or NaN).  The restatement states the limit instead: the
normalised coordinate of such an axis is the constant -1 — the only plane, clipped, no gradient on that axis — which is what the kernels
compute.

Proof of the class: each case states the path of every frame (3 / 4 / 5 = the dense kernels' E, 0 = the tiled scatter) and asserts it
from ops.warp_sample_box on ops.warp_coords with the rule of include/mphip.h: E = max(ex, ey, ez, 3) <= 5, H*W % 4 == 0 and
D*H*W % 32 == 0 (>= 32).  The box itself is compared with the one of the CPU's float64 coordinates.

Ragged volumes (D*H*W % 32 != 0).  Before the shape rule asked for whole groups of 32, frames with a small box on such volumes went to
warp_bwd_dense_dv_kernel, which (a) never summed the outputs past the last whole group when floor(vol / 32) is a multiple of 256 and
(b) fed a clamped prefetch into a wave's last, partial iteration.  With that library (MI355X) the ragged-* cases of test_warp_volume_bwd
gave max|dv - g64| of 0.87 / 0.49 (4x36x57, volume / dsum), 0.96 / 0.93 (7x36x36) and 0.57 / 0.58 (6x68x23) against max|g64| of 17 to 31,
3600 to 8300 times the bar; 6x10x14 (its one partial iteration is a wave's first, loaded unclamped) passed at 0.12 / 0.15 of the bar.
On the scatter all eight are within 0.38 of it."""
import functools
import json
import math
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FLOOR = 2.0 ** -22
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from megaportrait_hack_amd import _lib, ops

    _lib.load()
    return ops


@pytest.fixture(scope="module")
def ag():
    from megaportrait_hack_amd import autograd

    return autograd


# ------------------------------------------------------------------ the bar and its record
_RECORD = {}


def _note(test, case, ratio):
    """worst err / bound per test; rewritten on every call when MPHIP_PARITY_JSON names a file"""
    cur = _RECORD.setdefault(test, {"worst_err_over_bound": -1.0, "at": None, "checks": 0})
    cur["checks"] += 1
    if ratio > cur["worst_err_over_bound"]:
        cur["worst_err_over_bound"], cur["at"] = float(f"{ratio:.4g}"), case
    out = os.environ.get("MPHIP_PARITY_JSON")
    if out:
        with open(out, "w") as f:
            json.dump({"what": "tests/test_gpu_warp_bwd_branches.py: worst max|got - g64| / (4 * max|g32 - g64| + 2^-22 * max|g64|) per test "
                               "(the K3 check: its own elementwise bound), and the case it occurred at",
                       "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "tests": _RECORD}, f, indent=1)
            f.write("\n")


def _bar(test, case, what, got, g64, g32):
    """max|got - g64| <= 4 * max|g32 - g64| + 2^-22 * max|g64|; prints the three numbers.  Returns None, or the failure as text (the
    caller asserts once every quantity of the case is printed and recorded)."""
    got = got.detach().cpu().double()
    assert got.shape == g64.shape, (what, got.shape, g64.shape)
    err = (got - g64).abs().max().item()
    ref = (g32.double() - g64).abs().max().item()
    top = g64.abs().max().item()
    bound = 4.0 * ref + FLOOR * top
    ratio = 0.0 if err == 0.0 else err / max(bound, 1e-300)
    print(f"{test}[{case}] {what}: max|got-g64| {err:.3e}  max|g32-g64| {ref:.3e}  max|g64| {top:.3e}  err/bound {ratio:.3f}")
    _note(test, f"{case} {what}", ratio)
    return None if err <= bound and math.isfinite(err) else f"{what}: err {err:.3e} > bound {bound:.3e} (x{ratio:.3g})"


# ------------------------------------------------------------------ the operation restated (dtype of its inputs)
def _lins(ops, dhw):
    """the tables the kernels are handed (ops.linspace_table), on the CPU"""
    return tuple(ops.linspace_table(n, CPU) for n in dhw)


def _normalized(field, lins, dhw):
    """model.py:1036-1058 in field.dtype: the [B,D,H,W,3] grid handed to grid_sample, components (x, y, z).  An axis of size 1: the
    constant -1 (see the file's docstring)."""
    D, H, W = dhw
    dt = field.dtype
    f = F.interpolate(field, size=(D, H, W), mode="trilinear", align_corners=True)
    gd, gh, gw = torch.meshgrid(*(t.to(dt) for t in lins), indexing="ij")
    warped = torch.stack((gw, gh, gd), dim=-1).unsqueeze(0) + f.permute(0, 2, 3, 4, 1)
    n = [2.0 * warped[..., a] / float(s - 1) - 1.0 if s > 1 else torch.full_like(warped[..., a], -1.0) for a, s in enumerate((W, H, D))]
    return torch.stack(n, dim=-1)


def _warp_op(v, field, lins, dsum):
    """apply_warping_field (model.py:1028-1065) and, dsum, torch.sum(dim=2) (model.py:1171) in the dtype of v / field"""
    out = F.grid_sample(v, _normalized(field, lins, tuple(v.shape[2:])), mode="bilinear", padding_mode="border", align_corners=True)
    return out.sum(dim=2) if dsum else out


def _quiet(field, lins, dhw):
    """The quiet-input assertions.  Returns (floor indices [B,D,H,W,3] int64, clipped mask) of the float64 evaluation."""
    D, H, W = dhw
    res = []
    for dt in (torch.float32, torch.float64):
        sz = torch.tensor([W - 1, H - 1, D - 1], dtype=dt)
        c = ((_normalized(field.to(dt), lins, dhw) + 1.0) / 2.0) * sz      # grid_sampler_unnormalize, align_corners=True
        lo, hi = c <= 0.0, c >= sz                                        # clip_coordinates_set_grad: no gradient through these
        res.append((c, lo, hi, torch.minimum(sz, c.clamp_min(0.0)).floor().to(torch.int64)))
    (_, lo32, hi32, fl32), (c64, lo64, hi64, fl64) = res
    assert torch.equal(lo32, lo64) and torch.equal(hi32, hi64), "fp32 and float64 disagree on a clip decision"
    assert torch.equal(fl32, fl64), "fp32 and float64 disagree on a floor index"
    free = ~(lo64 | hi64)
    if bool(free.any()):
        gap = (c64 - c64.round()).abs()[free].min().item()
        assert gap >= 1e-3, f"an unclipped coordinate lies {gap:.2e} from an integer"
    return fl64, lo64 | hi64


def _boxes(fl, dhw):
    """{lx, ly, lz, ex, ey, ez} per frame from the floor indices [B,D,H,W,3] (x, y, z), as ops.warp_sample_box defines them"""
    D, H, W = dhw
    top = torch.tensor([W - 1, H - 1, D - 1])
    lo, hi = fl.amin(dim=(1, 2, 3)), fl.amax(dim=(1, 2, 3))
    return torch.cat([lo, torch.minimum(hi + 1, top) - lo + 1], dim=1)


def _path(box_row, dhw):
    """the rule of include/mphip.h (K10): the dense kernels' E, or 0 = tiled scatter"""
    D, H, W = dhw
    e = max(int(box_row[3]), int(box_row[4]), int(box_row[5]), 3)
    return e if e <= 5 and (H * W) % 4 == 0 and D * H * W >= 32 and (D * H * W) % 32 == 0 else 0


def _scatter_tile_boxes(fl_frame, dhw):
    """source-box voxels of every 4 x 16 x 16 tile of warp_bwd_tiled_kernel, from one frame's floor indices [D,H,W,3]"""
    D, H, W = dhw
    pd, ph, pw = -D % 4, -H % 16, -W % 16
    lo = F.pad(fl_frame.permute(3, 0, 1, 2), (0, pw, 0, ph, 0, pd), value=1 << 30)
    hi = F.pad(fl_frame.permute(3, 0, 1, 2), (0, pw, 0, ph, 0, pd), value=-1)
    shp = (3, (D + pd) // 4, 4, (H + ph) // 16, 16, (W + pw) // 16, 16)
    lo, hi = lo.reshape(shp).amin(dim=(2, 4, 6)), hi.reshape(shp).amax(dim=(2, 4, 6))
    top = torch.tensor([W - 1, H - 1, D - 1]).view(3, 1, 1, 1)
    return (torch.minimum(hi + 1, top) - lo + 1).prod(dim=0)


# ------------------------------------------------------------------ fields that put every sample where the case wants it
def _u01(shape, seed):
    return (R.seeded_tensor(tuple(shape), seed).double() + 1.0) * 0.5


def _placed_field(target, lins):
    """field [B,3,D,H,W] (the volume's own size) = target - linspace: sample (b, d, h, w) lands at target[b, :, d, h, w] (x, y, z)"""
    ld, lh, lw = (t.double() for t in lins)
    D, H, W = len(ld), len(lh), len(lw)
    lin = torch.stack([lw.view(1, 1, W).expand(D, H, W), lh.view(1, H, 1).expand(D, H, W), ld.view(D, 1, 1).expand(D, H, W)])
    return (target - lin).float().contiguous()


def _axis_index(dhw, a):
    """the output index along axis a (0 = x / W, 1 = y / H, 2 = z / D) of every voxel, [D,H,W]"""
    D, H, W = dhw
    shape = [(1, 1, W), (1, H, 1), (D, 1, 1)][a]
    return torch.arange((W, H, D)[a]).view(shape).expand(D, H, W)


def _frame_target(kind, arg, dhw, seed):
    """float64 targets [3,D,H,W] of one frame.
    low / high / mid E: floor indices in a box of the dense class E in that corner of the volume; a floor index S - 1 exists only as a
        clipped sample, so the `high` box has its +1 corner clipped away (extent 2 on x, E on y, 2 on z);
    flow:  the identity flow (sample o lands in voxel o): smooth and travelling, a 17 x 17 x 5 box per 4 x 16 x 16 tile;
    wild:  incoherent, every sample anywhere in the volume;
    clip:  a quarter of the samples clipped below 0 and a quarter above S - 1 on each axis, some exactly on 0.0 and on S - 1."""
    D, H, W = dhw
    S = (W, H, D)
    out = []
    for a, s in enumerate(S):
        u, fr = _u01(dhw, seed * 100 + a), 0.25 + 0.5 * _u01(dhw, seed * 100 + 10 + a)
        if kind in ("low", "high", "mid"):
            lo, n = {"low": [(0, max(1, min(arg - 1, s - 1)))] * 3,
                     "high": [(W - 2, 2), (H - arg, arg), (D - 2, 2)],
                     "mid": [(3, arg - 1), (2, arg - 1), (1, 2)]}[kind][a]
            fl = lo + (u * n).floor().clamp(max=n - 1)
        elif kind == "flow":
            fl = _axis_index(dhw, a).double().clamp(max=max(s - 2, 0))
        else:
            fl = (_u01(dhw, seed * 100 + 20 + a) * (s - 1)).floor().clamp(max=max(s - 2, 0))
        t = torch.where(fl >= s - 1, s - 0.5 + fr, fl + fr)               # floor S - 1: past the border, clipped to it
        if kind == "clip":
            edge = (_axis_index(dhw, a) == 0) | (_axis_index(dhw, a) == s - 1)
            t = torch.where(u < 0.25, -0.5 - fr, t)
            t = torch.where(u < 0.06, torch.zeros_like(t), t)
            t = torch.where(u > 0.75, s - 0.5 + fr, t)
            t = torch.where((u > 0.90) & edge, torch.full_like(t, float(s - 1)), t)
        out.append(t)
    return torch.stack(out)


def _affine_field(fdhw, dhw, gamma, delta, amp, seed, B=2):
    """field [B,3,fD,fH,fW] whose align_corners=True resize to dhw puts sample o of axis a at gamma[a] * o + delta[a] + noise, |noise| <= amp
    (trilinear resizing reproduces an affine field and is a convex combination of the noise).  An axis with fS == 1 carries a constant:
    there the coordinate is linspace + constant = 2 o / (S - 1) + delta[a] whatever gamma[a] says."""
    fD, fH, fW = fdhw
    D, H, W = dhw
    f = torch.zeros(B, 3, fD, fH, fW, dtype=torch.float64)
    for a, (s, fs) in enumerate(zip((W, H, D), (fW, fH, fD))):
        i = _axis_index(fdhw, a).double()
        o = i * (s - 1) / (fs - 1) if fs > 1 else torch.zeros_like(i)
        slope = gamma[a] - (2.0 / (s - 1) if s > 1 else 0.0)
        f[:, a] = slope * o + delta[a] + 1.0
    return (f + amp * R.seeded_tensor((B, 3, fD, fH, fW), seed).double()).float().contiguous()


# ------------------------------------------------------------------ the cases of ops.warp_volume_bwd
# name -> (C, (D,H,W), frames, paths): frames = [(kind, arg)] for _frame_target, or ("resized", fdhw, gamma, delta, amp); paths = what
# every frame must take (3 / 4 / 5: dense E, 0: tiled scatter)
V = (4, 8, 12)      # 384 voxels = 12 groups of 32
TRAVEL, STILL = (0.5, 0.5, 0.5), (0.0, 0.0, 0.0)
WARP_CASES = {}
for _e in (3, 4, 5):
    WARP_CASES[f"dense-E{_e}-low-corner"] = (12, V, [("low", _e), ("low", _e)], [_e, _e])
    WARP_CASES[f"dense-E{_e}-high-corner-clipped-plus-one"] = (12, V, [("high", _e), ("high", _e)], [_e, _e])
    WARP_CASES[f"dense-E{_e}-mid-volume"] = (12, V, [("mid", _e), ("mid", _e)], [_e, _e])
WARP_CASES["dense-E3-and-E5-in-one-batch"] = (12, V, [("low", 3), ("mid", 5)], [3, 5])
# dense reduction ranges (vol % 32 == 0): per_wave = ceil(vol / 32 / 256) * 32 outputs for each of the frame's 256 waves
WARP_CASES["dense-vol32-1x4x8-one-wave"] = (5, (1, 4, 8), [("low", 3), ("low", 4)], [3, 4])
WARP_CASES["dense-vol32-2x4x4-one-wave"] = (5, (2, 4, 4), [("low", 3), ("low", 4)], [3, 4])
WARP_CASES["dense-3x8x12-9-of-256-waves"] = (5, (3, 8, 12), [("low", 3), ("low", 4)], [3, 4])
WARP_CASES["dense-5x32x60-two-iterations-150-waves"] = (5, (5, 32, 60), [("low", 3), ("mid", 5)], [3, 5])
WARP_CASES["dense-16x16x32-one-iteration-every-wave"] = (5, (16, 16, 32), [("low", 3), ("mid", 4)], [3, 4])
# ragged volumes with dense-class boxes: vol % 32 != 0 keeps them on the scatter
WARP_CASES["ragged-4x36x57-vol8208-small-box"] = (5, (4, 36, 57), [("low", 3), ("mid", 5)], [0, 0])
WARP_CASES["ragged-7x36x36-vol9072-small-box"] = (5, (7, 36, 36), [("low", 3), ("mid", 5)], [0, 0])
WARP_CASES["ragged-6x68x23-vol9384-small-box"] = (5, (6, 68, 23), [("low", 4), ("mid", 3)], [0, 0])
WARP_CASES["ragged-6x10x14-vol840-small-box"] = (5, (6, 10, 14), [("low", 3), ("mid", 4)], [0, 0])
# channel blocks: the dense kernels' 96-channel blocks (clamped rows of the last one, two LDS passes of the coordinate gradient for
# C > 96) and the scatter's 8-channel slices (C % 8 != 0)
for _c in (5, 32, 96, 97, 100, 200):
    WARP_CASES[f"channels-C{_c}-dense-and-tiled-frame"] = (_c, V, [("low", 4), ("flow", None)], [4, 0])
# small boxes that must stay on the scatter
WARP_CASES["scatter-HW35-not-multiple-of-4"] = (5, (4, 5, 7), [("low", 3), ("low", 4)], [0, 0])
WARP_CASES["scatter-vol8-below-32"] = (5, (1, 2, 4), [("low", 3), ("low", 3)], [0, 0])
# tiled scatter
WARP_CASES["tiled-staged-box-travelling-field"] = (12, (8, 16, 24), [("flow", None), ("flow", None)], [0, 0])
WARP_CASES["tiled-unstaged-box-incoherent-field"] = (12, (8, 16, 24), [("wild", None), ("wild", None)], [0, 0])
WARP_CASES["tiled-ragged-tiles-5x18x20-staged"] = (12, (5, 18, 20), [("flow", None), ("flow", None)], [0, 0])
WARP_CASES["tiled-ragged-tiles-5x18x28-unstaged"] = (12, (5, 18, 28), [("wild", None), ("wild", None)], [0, 0])
WARP_CASES["mixed-dense-and-tiled-frame-1-and-2-slabs"] = (12, (8, 16, 24), [("low", 3), ("flow", None)], [3, 0])
# the clip rule
WARP_CASES["clip-dense-4x4x4"] = (12, (4, 4, 4), [("clip", None), ("clip", None)], [4, 4])
WARP_CASES["clip-tiled-6x10x14"] = (12, (6, 10, 14), [("clip", None), ("clip", None)], [0, 0])
# field sizes (same size: every case above)
WARP_CASES["field-up-5x7x9-to-6x10x14-tiled"] = (12, (6, 10, 14), ("resized", (5, 7, 9), TRAVEL, (0.25, 0.25, 0.25), 0.1), [0, 0])
WARP_CASES["field-up-3x5x7-to-4x8x12-dense"] = (12, V, ("resized", (3, 5, 7), STILL, (1.5, 0.5, 1.5), 0.2), [3, 3])
WARP_CASES["field-down-64x64x64-to-8x16x24-tiled"] = (12, (8, 16, 24), ("resized", (64, 64, 64), TRAVEL, (0.25, 0.25, 0.25), 0.1), [0, 0])
WARP_CASES["field-down-64x64x64-to-8x16x24-dense"] = (12, (8, 16, 24), ("resized", (64, 64, 64), STILL, (1.5, 0.5, 1.5), 0.2), [3, 3])
WARP_CASES["field-fD1-to-5x8x12-dense"] = (12, (5, 8, 12), ("resized", (1, 8, 12), STILL, (1.5, 0.5, 0.25), 0.1), [4, 4])
WARP_CASES["field-fD1-to-5x8x12-tiled"] = (12, (5, 8, 12), ("resized", (1, 8, 12), TRAVEL, (0.25, 0.25, 0.25), 0.1), [0, 0])


@functools.lru_cache(maxsize=None)
def _warp_inputs(name):
    """(v, field, lins, floor indices, clipped mask, CPU boxes) of a case; the quiet-input and class assertions that need no GPU"""
    from megaportrait_hack_amd import ops

    C, dhw, frames, paths = WARP_CASES[name]
    seed = 1000 + zlib.crc32(name.encode()) % 9000
    lins = _lins(ops, dhw)
    if frames[0] == "resized":
        _, fdhw, gamma, delta, amp = frames
        field = _affine_field(fdhw, dhw, gamma, delta, amp, seed)
    else:
        field = _placed_field(torch.stack([_frame_target(kind, arg, dhw, seed + 1 + b) for b, (kind, arg) in enumerate(frames)]), lins)
    B = field.shape[0]
    v = R.seeded_tensor((B, C) + dhw, seed + 5, scale=1.7)
    fl, clipped = _quiet(field, lins, dhw)
    boxes = _boxes(fl, dhw)
    assert [_path(boxes[b], dhw) for b in range(B)] == paths, (name, boxes.tolist(), paths)
    return v, field, lins, fl, clipped, boxes


@functools.lru_cache(maxsize=None)
def _warp_reference(name, dsum):
    """(dout, {32, 64: (out, dv, dfield)}): computed once per (case, dsum), shared and left unchanged"""
    v, field, lins, _, _, _ = _warp_inputs(name)
    res, dout = {}, None
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        vv, ff = v.to(dt).clone().requires_grad_(True), field.to(dt).clone().requires_grad_(True)
        out = _warp_op(vv, ff, lins, dsum)
        if dout is None:
            dout = R.seeded_tensor(tuple(out.shape), 4242 + len(name))
        out.backward(dout.to(dt))
        res[bits] = (out.detach(), vv.grad, ff.grad)
    return dout, res


def _check_class(ops, dev, name):
    """the stated path of every frame, from ops.warp_sample_box on ops.warp_coords; the box itself against the CPU's"""
    _, field, _, _, _, boxes = _warp_inputs(name)
    _, dhw, _, paths = WARP_CASES[name]
    got = ops.warp_sample_box(ops.warp_coords(field.to(dev), *dhw)).cpu()
    assert torch.equal(got[:, :6].to(torch.int64), boxes), (name, got.tolist(), boxes.tolist())
    assert [_path(got[b], dhw) for b in range(got.shape[0])] == paths, (name, got.tolist(), paths)


@pytest.mark.parametrize("dsum", [False, True], ids=["volume", "dsum"])
@pytest.mark.parametrize("name", list(WARP_CASES))
def test_warp_volume_bwd(ops, ag, dev, name, dsum):
    """out, dv and dfield of WarpVolumeFn (K2 / K3 forward, ops.warp_volume_bwd) at every branch of the host code, the per-tile choice
    and the per-channel-block choice.
    Worst err / bound on an MI355X: 0.38 (dv of ragged-6x68x23, volume); what the ragged-* cases gave before the vol % 32 rule is in the
    file's docstring and in profiles/warp_bwd_branches.json."""
    v, field, lins, fl, clipped, _ = _warp_inputs(name)
    _, dhw, frames, paths = WARP_CASES[name]
    # the case contains what its name says
    tiles = [_scatter_tile_boxes(fl[b], dhw) for b in range(fl.shape[0])]
    if "unstaged" in name:
        assert all(bool((t * 8 > 16384).any()) for t in tiles), [t.max().item() for t in tiles]
    elif name.startswith("tiled-") or name.startswith("mixed-"):
        assert all(bool((t * 8 <= 16384).all()) for t in tiles), [t.max().item() for t in tiles]
    if name.startswith("tiled-ragged"):
        assert dhw[0] % 4 and dhw[1] % 16 and dhw[2] % 16
    if "high-corner" in name:
        assert bool((_boxes(fl, dhw)[:, 3] < torch.tensor(paths)).all())      # ex < E: the fold kernel's skip
    if name.startswith("clip-"):
        target = field.double() + torch.stack([lins[2].view(1, 1, -1).expand(dhw), lins[1].view(1, -1, 1).expand(dhw),
                                               lins[0].view(-1, 1, 1).expand(dhw)]).double()
        for a, s in enumerate((dhw[2], dhw[1], dhw[0])):
            assert int((target[:, a] == 0.0).sum()) > 0 and int((target[:, a] == float(s - 1)).sum()) > 0
            frac = clipped[..., a].double().mean().item()
            assert 0.35 < frac < 0.65, frac
    _check_class(ops, dev, name)
    dout, ref = _warp_reference(name, dsum)
    vg, fg = v.to(dev).requires_grad_(True), field.to(dev).requires_grad_(True)
    out = ag.WarpVolumeFn.apply(vg, fg, dsum)
    out.backward(dout.to(dev))
    test = "test_warp_volume_bwd"
    case = f"{name}-{'dsum' if dsum else 'volume'}"
    bad = [_bar(test, case, what, got, ref[64][i], ref[32][i]) for i, (what, got) in enumerate((("out", out), ("dv", vg.grad), ("dfield", fg.grad)))]
    if name.startswith("clip-"):
        # ATen's rule: a clipped coordinate (border hits included) passes no gradient — exactly none; the same-size resize adds nothing
        assert bool((fg.grad.cpu().permute(0, 2, 3, 4, 1)[clipped] == 0.0).all())
        assert bool((ref[64][2].permute(0, 2, 3, 4, 1)[clipped] == 0.0).all())
    assert not any(bad), [b for b in bad if b]


@pytest.mark.parametrize("dsum", [False, True], ids=["volume", "dsum"])
@pytest.mark.parametrize("name", ["dense-E4-mid-volume", "tiled-staged-box-travelling-field"])
def test_warp_volume_bwd_one_gradient_alone(ops, dev, name, dsum):
    """want_v=False and want_field=False, one at a time: the gradient that is produced equals the one of the call that asks for both —
    bit for bit on the dense path and for the coordinate gradient of the scatter; the scatter's dv (fp32 atomics, no fixed order) is
    held to the bar instead."""
    v, field, _, _, _, _ = _warp_inputs(name)
    dout, ref = _warp_reference(name, dsum)
    vg, fg, dg = v.to(dev), field.to(dev), dout.to(dev)
    dv, df = ops.warp_volume_bwd(vg, fg, dg, dsum)
    dv_only, none_f = ops.warp_volume_bwd(vg, fg, dg, dsum, want_v=True, want_field=False)
    none_v, df_only = ops.warp_volume_bwd(vg, fg, dg, dsum, want_v=False, want_field=True)
    assert none_f is None and none_v is None
    assert torch.equal(df_only, df)
    test, case = "test_warp_volume_bwd_one_gradient_alone", f"{name}-{'dsum' if dsum else 'volume'}"
    if name.startswith("dense"):
        assert torch.equal(dv_only, dv)
    bad = [_bar(test, case, "dv alone", dv_only, ref[64][1], ref[32][1]), _bar(test, case, "dfield alone", df_only, ref[64][2], ref[32][2])]
    assert not any(bad), [b for b in bad if b]


# ------------------------------------------------------------------ ops.warp_sample_box
def _offset_view(t, dev):
    """A contiguous device copy of `t` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("dhw,offset", [
    ((6, 52, 56), False),    # vol % 4 == 0: the 16-byte path, 17472 voxels = two steps of 4 x 1024 groups, the second clamped
    ((2, 4, 6), False),      # ... and fewer groups (12) than threads
    ((5, 41, 43), False),    # vol % 4 != 0: dword loads, 8815 voxels = two steps of 8 x 1024 voxels, the second clamped
    ((3, 5, 7), False),      # ... and fewer voxels (105) than threads
    ((6, 52, 56), True),     # vol % 4 == 0 in a buffer that starts 4 bytes past a 16-byte boundary: dword loads
], ids=["vol-multiple-of-4-two-steps", "vol-multiple-of-4-12-groups", "vol-odd-two-steps", "vol-odd-105-voxels", "misaligned-buffer"])
def test_warp_sample_box(ops, dev, dhw, offset):
    """box[b] = {lx, ly, lz, ex, ey, ez} of three frames against the same quantities from the coordinates on the CPU.  Each frame has its
    own range; its extreme samples sit in the last voxel and in the first one, where a wrong tail or a wrong frame offset loses them."""
    D, H, W = dhw
    top = torch.tensor([W - 1, H - 1, D - 1], dtype=torch.float32)
    lo = torch.tensor([[0.2, 0.3, 0.1], [0.45, 0.1, 0.3], [0.0, 0.5, 0.6]])
    hi = torch.tensor([[0.5, 0.6, 0.5], [0.7, 0.35, 0.9], [1.0, 0.9, 1.0]])
    u = (R.seeded_tensor((3, D, H, W, 3), 77 + D).float() + 1.0) * 0.5
    coords = (lo.view(3, 1, 1, 1, 3) + 0.05 + u * (hi - lo - 0.1).view(3, 1, 1, 1, 3)) * top
    coords[:, -1, -1, -1] = lo * top          # the minimum of every axis: the last voxel of the frame
    coords[:, 0, 0, 0] = hi * top             # the maximum: the first
    coords = coords.contiguous()
    cg = _offset_view(coords, dev) if offset else coords.to(dev)
    assert offset or cg.data_ptr() % 16 == 0
    got = ops.warp_sample_box(cg).cpu()
    want = _boxes(coords.floor().to(torch.int64), dhw)
    assert torch.equal(got[:, :6].to(torch.int64), want), (got.tolist(), want.tolist())
    assert len({tuple(r) for r in want.tolist()}) == 3


# ------------------------------------------------------------------ ops.warp_field_compose_bwd
def _compose_op(theta, em, G):
    """rt + em64 of the warp generators (model.py:804-806, 971-973) in the dtype of its inputs"""
    return F.affine_grid(theta, (theta.shape[0], 1, G, G, G), align_corners=False).permute(0, 4, 1, 2, 3) \
        + F.interpolate(em, size=(G, G, G), mode="trilinear", align_corners=False)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", [(16, 16, 16, 64), (3, 5, 7, 24), (20, 20, 20, 20), (24, 12, 6, 12)],
                         ids=["16x16x16-to-64-the-models", "3x5x7-to-24-two-chunks-second-partial", "20x20x20-to-20-same-size-one-partial-chunk",
                              "24x12x6-to-12-em-larger-on-two-axes"])
def test_warp_field_compose_bwd(ops, dev, shape, B):
    """dtheta (8192-output chunks summed in double) and dem (the separable align_corners=False adjoint), both together and each alone"""
    eD, eH, eW, G = shape
    theta = R.seeded_tensor((B, 3, 4), 201 + G)
    em = (R.seeded_tensor((B, 3, eD, eH, eW), 202 + G) + 1.0) * 0.5
    dw = R.seeded_tensor((B, 3, G, G, G), 203 + G)
    ref = {}
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        t, e = theta.to(dt).clone().requires_grad_(True), em.to(dt).clone().requires_grad_(True)
        _compose_op(t, e, G).backward(dw.to(dt))
        ref[bits] = (t.grad, e.grad)
    dwg = dw.to(dev)
    both = ops.warp_field_compose_bwd(dwg, tuple(em.shape))
    theta_only = ops.warp_field_compose_bwd(dwg, tuple(em.shape), want_theta=True, want_em=False)
    em_only = ops.warp_field_compose_bwd(dwg, tuple(em.shape), want_theta=False, want_em=True)
    assert theta_only[1] is None and em_only[0] is None
    assert torch.equal(theta_only[0], both[0]) and torch.equal(em_only[1], both[1])    # no atomics anywhere: bit for bit
    test, case = "test_warp_field_compose_bwd", f"{eD}x{eH}x{eW}-to-{G}-B{B}"
    bad = [_bar(test, case, "dtheta", both[0], ref[64][0], ref[32][0]), _bar(test, case, "dem", both[1], ref[64][1], ref[32][1])]
    assert not any(bad), [b for b in bad if b]


# ------------------------------------------------------------------ ops.rt_theta_bwd
def _theta_op(rot, tr, invert):
    """affine_theta (model.py:790-804) in the dtype of its inputs"""
    a = torch.eye(4, dtype=rot.dtype).repeat(rot.shape[0], 1, 1)
    a[:, :3, :3] = R.rotation_matrix(rot)
    a[:, :3, 3] = tr
    if invert:
        a = torch.inverse(a)
    return a[:, :3].contiguous()


@pytest.mark.parametrize("invert", [False, True], ids=["forward", "inverted"])
def test_rt_theta_bwd(ops, dev, invert):
    """B = 70: two workgroups of 64, the second partial; angles from +-180 degrees, and rows with angles exactly 0, 90 and -90"""
    B = 70
    rot = R.seeded_tensor((B, 3), 111, scale=180.0)
    exact = torch.tensor([[0.0, 0.0, 0.0], [90.0, 90.0, 90.0], [-90.0, -90.0, -90.0], [0.0, 90.0, -90.0], [90.0, 0.0, 0.0], [0.0, -90.0, 0.0],
                          [-90.0, 0.0, 90.0], [180.0, -180.0, 0.0]])
    rot[:4], rot[62:66] = exact[:4], exact[4:]         # in both workgroups
    tr = R.seeded_tensor((B, 3), 112, scale=0.17)
    dth = R.seeded_tensor((B, 3, 4), 113)
    ref = {}
    for bits, dt in ((64, torch.float64), (32, torch.float32)):
        r, t = rot.to(dt).clone().requires_grad_(True), tr.to(dt).clone().requires_grad_(True)
        _theta_op(r, t, invert).backward(dth.to(dt))
        ref[bits] = (r.grad, t.grad)
    drot, dtr = ops.rt_theta_bwd(rot.to(dev), tr.to(dev), dth.to(dev), invert)
    test, case = "test_rt_theta_bwd", "inverted" if invert else "forward"
    bad = [_bar(test, case, "drot", drot, ref[64][0], ref[32][0]), _bar(test, case, "dtr", dtr, ref[64][1], ref[32][1])]
    assert not any(bad), [b for b in bad if b]


# ------------------------------------------------------------------ K2 with more than one tile column (and ragged tiles)
def _k2_marks_ragged(coords):
    """What warp_gather_kernel decides per 32 x 64 tile of a (frame, slice) — tests/test_gpu_half_models.py's _k2_marks for maps that are
    no multiple of the tile: [B,D,tiles_h,tiles_w], 0 = in the corner image, 1 = column walk (box <= 16384 voxels), 2 = direct gather."""
    b, d, h, w, _ = coords.shape
    ph, pw = -h % 32, -w % 64
    fl = coords.floor().to(torch.int64).permute(0, 1, 4, 2, 3)                       # [B,D,3,H,W]
    shp = (b, d, 3, (h + ph) // 32, 32, (w + pw) // 64, 64)
    lo = F.pad(fl, (0, pw, 0, ph), value=1 << 30).reshape(shp).amin(dim=(4, 6))
    hi = F.pad(fl, (0, pw, 0, ph), value=-1).reshape(shp).amax(dim=(4, 6))
    top = torch.tensor([w - 1, h - 1, d - 1], device=coords.device).view(1, 1, 3, 1, 1)
    ext = torch.minimum(hi + 1, top) - lo + 1
    corner = ((lo + ext) <= 6).all(dim=2)
    return torch.where(corner, 0, torch.where(ext.prod(dim=2) <= 16384, 1, 2))


def _k2_field(kind, dhw, seed):
    """[2,3,D,H,W] (a sample lands at linspace + field, clipped).  corner: the reference's kind, every sample in the low corner;
    travelling: smooth, x runs through the volume; incoherent: every sample anywhere."""
    D, H, W = dhw
    f = R.seeded_tensor((2, 3, D, H, W), seed)
    if kind == "travelling":
        f[:, 0] += torch.linspace(0.0, 0.7 * W, W).view(1, 1, 1, W)
    elif kind == "incoherent":
        f = (f + 1.0) * 0.5 * torch.tensor([W - 2.0, H - 2.0, D - 2.0]).view(1, 3, 1, 1, 1) + 1.0
    return f.contiguous()


@pytest.mark.parametrize("kind", ["corner", "travelling", "incoherent"])
@pytest.mark.parametrize("shape", [(8, 5, 40, 72), (8, 6, 36, 136)], ids=["5x40x72-two-tile-columns", "6x36x136-three-tile-columns"])
def test_k2_k3_forward_with_several_tile_columns(ops, dev, oracle_c, shape, kind):
    """K2 (tiles of 32 x 64 positions) on maps wider than one tile, with ragged last tiles in both directions: bit for bit the plain-C
    oracle, as test_warp_volume_indices_bit_exact asks at one tile column.  The class of every tile is recomputed from the coordinates
    and the case must contain the one it is named after — the corner gather for `corner`, the column walk for `travelling`, and for
    `incoherent` the direct gather where a tile's box can exceed 16384 voxels (6 x 36 x 136 = 29376) and the column walk where it
    cannot (5 x 40 x 72 = 14400).  K3 on the same inputs against the float64 sum over depth of that volume: K3 adds D values of eight
    taps each, so |err| <= (D + 20) * 2^-24 * (the same warp and sum of |v|) elementwise — D - 1 additions, and up to 10 roundings per
    tap on either side should its tap order differ from K2's."""
    C, D, H, W = shape
    field = _k2_field(kind, (D, H, W), 610 + W)
    v = R.seeded_tensor((2, C, D, H, W), 620 + W, scale=1.7)
    out, coords, idx = ops.warp_volume(v.to(dev), field.to(dev), return_coords=True)
    c_ref, i_ref = oracle_c.warp_coords(field, D, H, W)
    assert torch.equal(coords.cpu(), c_ref) and torch.equal(idx.cpu(), i_ref)
    marks = _k2_marks_ragged(c_ref)
    assert marks.shape[2:] == (2, (W + 63) // 64)
    want_mark = {"corner": 0, "travelling": 1, "incoherent": 2 if D * H * W > 16384 else 1}[kind]
    counts = torch.bincount(marks.flatten(), minlength=3).tolist()
    assert counts[want_mark] > 0 and (kind != "corner" or counts[1] + counts[2] == 0), counts
    for col in range(marks.shape[3]):          # ... in every tile column
        assert bool((marks[..., col] == want_mark).any()), (col, counts)
    want = oracle_c.apply_warping_field(v, field)
    assert torch.equal(out.cpu(), want)
    got_sum = ops.warp_volume_dsum(v.to(dev), field.to(dev)).cpu().double()
    err = (got_sum - want.double().sum(dim=2)).abs()
    bound = (D + 20) * U * oracle_c.apply_warping_field(v.abs(), field).double().sum(dim=2)
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"test_k2_k3_forward_with_several_tile_columns[{D}x{H}x{W}-{kind}] K3: max|err| {err.max().item():.3e}  worst err/bound {ratio:.3f}")
    _note("test_k2_k3_forward_with_several_tile_columns", f"{D}x{H}x{W}-{kind} K3", ratio)
    assert bool((err <= bound).all()), ratio
