"""Every branch of the precision-1 ("f16x3") 3-D forward and bwd-data convs, exactly: the two direct kernels (csrc/conv3d_f16x3.hip), the
three F(2,3) schedules and the two-frame mode (conv3d_f16x3_wino*.hip), the four 1x1x1 instantiations, their split-K slabs, persistent
tile walks, fused input affine, GroupNorm epilogues, demand-driven launches and bwd-data launches.

Each case first asserts that the library takes the path its id claims: mphip_debug_conv3d_plan (kernel 0..5, splits, chunks per split,
logical grid) for the 3x3x3 launches, mphip_debug_conv3d_k1_plan ({ks, column tiles per wave, grid, workgroup size}, ABI 27) for the
1x1x1 ones, and every edge the id names (`edge_holds`).  ops.conv3d drops to precision 0 without a word where precision 1 is unsupported
and the planner moves a shape to another kernel when a threshold changes; a case whose claim no longer holds fails before it launches.
The per-call switches (MPHIP_WINOGRAD_MIN_TILES, MPHIP_WINO_PP, MPHIP_WINOGRAD, MPHIP_WINOGRAD_D2, MPHIP_F16X3_SPLITS) are set with
monkeypatch; the switches the library reads once per process are not relied on: their branches are reached by shape.
tests/test_conv_f16x3_branches_host.py checks every claim on the CPU and requires that the plan classes reachable on a fixed grid are
exactly the classes the tables below cover.

Why there is no tolerance (integer cases).  x (dy) and w are integers in [-4, 4] and both contain a 4; bias is integers in [-8, 8].
  - All operand scales are powers of two: 2^11 for x (max * scale = 2^13, inside [2^13, 2^14)), 2^12 for w (max * scale = 2^14).
  - With |x| <= X and |w| <= Wm integers every scaled x and w is an exact f16, so every `lo` half is 0.
  - Direct and 1x1x1 kernels: partial sums are integers of magnitude <= 27 * Ci * X * Wm (Ci * X * Wm for k = 1) times one power of
    two, below 2^24 for every case here.
  - F(2,3) kernels: t = Bt d (differences / sums of two inputs) is an integer of magnitude <= 2X; u = G g is a multiple of 1/2 of
    magnitude <= 1.5 Wm; both are exact f16 at the tensor scales (|t| * 2^11 <= 2^14, |u| * 2^12 = (2u) * 2^11 with |2u| <= 12).
    Products are multiples of half the unit, a position's sum over (ci, kd, kh) is <= 9 * Ci * 2X * 3Wm half units, and the output
    transform adds three positions: 3 * 9 * Ci * 2X * 3Wm < 2^24, which for X = Wm = 4 needs Ci < 6472.
  - The fused affine (integer scale in [-2, 2], shift in [-3, 3]) gives |x'| <= 11 with x_range = {0, 0, 11, 0}: the scale is 2^10,
    |t| <= 22, and every step is exact in the same way.
  - Any order of summation, any split and the ordered reduce therefore give the float64 answer's bits.
The float64 conv (F.conv3d / F.conv_transpose3d on the CPU) is THE answer and the kernels must be torch.equal to it.  Each case asserts its
bound, and that ATen's own fp32 CPU result equals the float64 one, before it touches the GPU.

Rounding (Gaussian cases; integer data says nothing about the `lo` planes): the project's rule of tests/test_gpu_conv2d_f16x3.py,
max|got - t64| <= 4 * max|t32 - t64| + 2^-21 * A, t32 = ATen's fp32 CPU result.  A = max over outputs of sum |x||w| for the direct and
1x1x1 kernels; for the F(2,3) kernels A is taken where they round, in the transformed domain: the maximum over outputs of the output
transform's absolute row sums ((1,1,1,0) and (0,1,1,1)) of sum |t_p||u_p|.  Each case also shows on the CPU that the bar can fail: the
one-product contract (operands rounded once to f16 at their scales; oracle.hotpath_ref.conv3d_wino_f16_contract for the F(2,3) kernels)
must exceed it 10x, the three-product emulation must stay under a tenth of it.  With MPHIP_PARITY_JSON=<file> the worst err / bar of
every test is written there (profiles/conv_f16x3_branches.json holds one MI355X run).

Magnitudes: x = ints * 2^p, w = ints * 2^q.  The kernels multiplied their accumulators by ONE float, 1/scale_w * 1/scale_x; at p = -100,
q = -30 that product is 2^-153, below the smallest fp32 subnormal, and every output (up to 2^-117, normal fp32 numbers) came out 0.
Predicted from the code, then observed on an MI355X; the two factors are applied one after the other now (split_unscale,
csrc/mphip_f16x3.h), bit-identical wherever the single product was representable.

Measured on an MI355X (one run, profiles/conv_f16x3_branches.json): worst err / bar 0.10 for test_rounding_bar, at the 1x1x1 <1,2> case
(1,48,96,1,1,65600); 0.03 to 0.08 for the 3x3x3 kernels.  The file's 193 cases take 8 s there."""
import collections
import ctypes
import functools
import json
import os
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as R

pytestmark = pytest.mark.gpu

EXACT = 2 ** 24
D2, D4, LOCKSTEP, ROLE, BIG, TWO = range(6)        # F16x3Kernel, as mphip_debug_conv3d_plan reports it
KERNEL_NAMES = ["direct2", "direct4", "lockstep", "rolesplit", "bigtile", "twoframe"]
MT = {"MPHIP_WINOGRAD_MIN_TILES": "1"}
PP0, PP2 = {"MPHIP_WINO_PP": "0"}, {"MPHIP_WINO_PP": "2"}
WINO_OFF, D2_OFF = {"MPHIP_WINOGRAD": "0"}, {"MPHIP_WINOGRAD_D2": "0"}
PER_CALL_SWITCHES = ("MPHIP_WINOGRAD_MIN_TILES", "MPHIP_WINO_PP", "MPHIP_WINOGRAD", "MPHIP_WINOGRAD_D2", "MPHIP_F16X3_SPLITS",
                     "MPHIP_F16X3_K1_KS", "MPHIP_F16X3_K1_MIN", "MPHIP_F16X3_TILE", "MPHIP_F16X3_NO_PERSIST")

# shape = (N, Ci, Co, D, H, W); claim = (kernel, splits, chunks per split, tiles = logical grid x); grid y is Co / 96, grid z the splits
Case = collections.namedtuple("Case", "shape kernel splits cps tiles env half edges")


def C(shape, kernel, splits, cps, tiles, env=None, half=False, edges=()):
    return Case(tuple(shape), kernel, splits, cps, tiles, tuple(sorted((env or {}).items())), half, tuple(edges))


def _join(*envs):
    out = {}
    for e in envs:
        out.update(e)
    return out


# ---- a. integer cases, forward --------------------------------------------------------------------------------------------------
DIRECT_CASES = [
    C((1, 16, 96, 2, 8, 8), D2, 1, 1, 1, edges=("one-tile", "one-chunk")),
    C((3, 48, 96, 2, 8, 16), D2, 3, 1, 6),
    C((5, 48, 192, 2, 8, 16), D2, 3, 1, 10, edges=("gridy2",)),
    C((1, 32, 96, 6, 16, 24), D2, 2, 1, 18, edges=("depth3", "cols3")),
    C((4, 784, 96, 2, 8, 8), D2, 49, 1, 4, edges=("ci>768",)),
    C((1, 768, 96, 6, 16, 16), D2, 24, 2, 12, edges=("depth3",)),                 # several splits of several chunks
    C((1, 48, 96, 2, 112, 112), D2, 1, 3, 196, edges=("cols3",)),                 # unsplit, several chunks, one resident round
    C((1, 16, 96, 4, 8, 8), D4, 1, 1, 1, edges=("one-tile", "one-chunk")),
    C((1, 48, 192, 4, 8, 16), D4, 3, 1, 2, edges=("gridy2",)),
    C((2, 32, 96, 8, 16, 24), D4, 2, 1, 24, edges=("cols3",)),
    C((1, 96, 96, 4, 8, 8), D4, 2, 3, 1, env={"MPHIP_F16X3_SPLITS": "2"}, edges=("one-tile",)),
    C((2, 768, 192, 4, 16, 16), D4, 16, 3, 8, edges=("gridy2",)),
    C((1, 48, 96, 4, 80, 80), D4, 1, 3, 100, edges=("cols3",)),
]
WINO_SHAPES = [   # (shape, splits, chunks per split, tiles, edges): the same five shapes on every 4-plane F(2,3) schedule
    ((1, 16, 96, 4, 8, 8), 1, 1, 1, ("one-tile", "one-chunk")),
    ((3, 16, 96, 4, 16, 8), 1, 1, 6, ()),
    ((2, 96, 96, 4, 8, 8), 6, 1, 2, ()),
    ((1, 384, 96, 4, 32, 32), 12, 2, 16, ("ci=384", "cols3")),
    ((1, 32, 96, 8, 24, 24), 2, 1, 18, ("cols3",)),
]
WINO_UNSPLIT = ((1, 48, 96, 4, 80, 80), 1, 3, 100, ("cols3",))     # unsplit, several chunks, one resident round (no switch needed)
SCHEDULES = [(ROLE, {}, False), (LOCKSTEP, PP0, False), (BIG, PP2, False), (ROLE, PP2, True)]   # last: half products, even with PP = 2
WINO_CASES = [C(s, kern, sp, cps, tiles, env=_join(MT, pp), half=half, edges=edges)
              for kern, pp, half in SCHEDULES for s, sp, cps, tiles, edges in WINO_SHAPES + [WINO_UNSPLIT]]
TWO_FRAME_CASES = [
    C((3, 32, 96, 2, 8, 8), TWO, 2, 1, 2, env=MT, edges=("odd-batch",)),
    C((5, 768, 192, 2, 8, 16), TWO, 16, 3, 6, env=MT, edges=("odd-batch", "gridy2")),
    C((4, 768, 768, 2, 8, 8), TWO, 16, 3, 2, edges=("no-switch",)),
    C((3, 32, 96, 2, 8, 8), D2, 2, 1, 3, env=_join(MT, D2_OFF)),                  # the two-frame shape, mode off: the direct kernel
    C((3, 16, 96, 2, 8, 8), TWO, 1, 1, 2, env=MT, edges=("odd-batch", "one-chunk")),
    C((5, 32, 96, 2, 64, 64), TWO, 1, 2, 192, env=MT, edges=("odd-batch", "cols3")),
]
# more logical workgroups than one resident round (256 per kernel, 512 for the (2,8,8) kernel): an uneven share of the tile walk
WALK_CASES = [
    C((1, 16, 96, 2, 184, 192), D2, 1, 1, 552, edges=("walk",)),
    C((1, 16, 96, 4, 136, 136), ROLE, 1, 1, 289, edges=("walk",)),
    C((1, 16, 96, 4, 136, 136), LOCKSTEP, 1, 1, 289, env=PP0, edges=("walk",)),
    C((1, 16, 96, 4, 136, 136), BIG, 1, 1, 289, env=PP2, edges=("walk",)),
    C((1, 16, 96, 4, 136, 136), ROLE, 1, 1, 289, env=PP2, half=True, edges=("walk",)),
    C((1, 16, 96, 4, 136, 136), D4, 1, 1, 289, env=WINO_OFF, edges=("walk",)),
    C((5, 16, 96, 2, 88, 96), TWO, 1, 1, 396, env=MT, edges=("walk", "odd-batch")),
    # ... and with two chunks per tile, so that the walk's second tile follows a chunk loop
    C((1, 32, 96, 2, 184, 192), D2, 1, 2, 552, edges=("walk",)),
    C((1, 32, 96, 4, 136, 136), ROLE, 1, 2, 289, edges=("walk",)),
    C((1, 32, 96, 4, 136, 136), LOCKSTEP, 1, 2, 289, env=PP0, edges=("walk",)),
    C((1, 32, 96, 4, 136, 136), BIG, 1, 2, 289, env=PP2, edges=("walk",)),
    C((1, 32, 96, 4, 136, 136), D4, 1, 2, 289, env=WINO_OFF, edges=("walk",)),
    C((5, 32, 96, 2, 88, 96), TWO, 1, 2, 396, env=MT, edges=("walk", "odd-batch")),
]
FWD_CASES = DIRECT_CASES + WINO_CASES + TWO_FRAME_CASES + WALK_CASES

# ---- b. fused input affine: (case, in_relu values, also with the GroupNorm epilogue) ---------------------------------------------------
GNIN_CASES = [
    (C((3, 48, 96, 2, 8, 16), D2, 3, 1, 6), True),
    (C((2, 32, 96, 8, 16, 24), D4, 2, 1, 24), False),
    (C((3, 16, 96, 4, 16, 8), LOCKSTEP, 1, 1, 6, env=_join(MT, PP0)), False),
    (C((3, 16, 96, 4, 16, 8), ROLE, 1, 1, 6, env=MT), True),
    (C((3, 16, 96, 4, 16, 8), BIG, 1, 1, 6, env=_join(MT, PP2)), False),
    (C((3, 32, 96, 2, 8, 8), TWO, 2, 1, 2, env=MT, edges=("odd-batch",)), False),       # the first tile holds two frames, two tables
    (C((1, 384, 96, 4, 32, 32), ROLE, 12, 2, 16, env=MT, edges=("ci=384",)), False),    # the 4-plane kernels' LDS table is full
    (C((2, 768, 96, 2, 8, 8), D2, 48, 1, 2), False),
    (C((2, 768, 96, 2, 8, 8), TWO, 48, 1, 1, env=MT), False),
]
# ---- c. gn_groups = 32: one per kernel ---------------------------------------------------------------------------------------------
GN_CASES = [
    C((3, 48, 96, 2, 8, 16), D2, 3, 1, 6),
    C((1, 48, 96, 2, 112, 112), D2, 1, 3, 196),
    C((2, 32, 96, 8, 16, 24), D4, 2, 1, 24),
    C((1, 48, 96, 4, 80, 80), D4, 1, 3, 100, env=WINO_OFF),
    C((3, 16, 96, 4, 16, 8), LOCKSTEP, 1, 1, 6, env=_join(MT, PP0)),
    C((3, 16, 96, 4, 16, 8), ROLE, 1, 1, 6, env=MT),
    C((3, 16, 96, 4, 16, 8), BIG, 1, 1, 6, env=_join(MT, PP2)),
    C((2, 96, 96, 4, 8, 8), ROLE, 6, 1, 2, env=MT),
    C((3, 32, 96, 2, 8, 8), TWO, 2, 1, 2, env=MT, edges=("odd-batch",)),
]
# ---- d. demand-driven launches (mphip_conv3d_fwd_roi): (case planned with roi = 1, box lists) ------------------------------------------
ALL_LISTS = ("tile-edges", "corner+volume", "empty+straddle")
ROI_CASES = [
    (C((2, 16, 96, 8, 16, 24), D4, 1, 1, 24, edges=("cols3",)), ALL_LISTS),                       # "thirds" of a (4,8,8) tile
    (C((2, 16, 96, 2, 16, 24), D2, 1, 1, 12, edges=("cols3",)), ALL_LISTS),
    (C((2, 16, 96, 6, 16, 24), D2, 1, 1, 36, edges=("cols3", "depth3")), ALL_LISTS),
    (C((2, 16, 96, 8, 16, 24), LOCKSTEP, 1, 1, 24, env=_join(MT, PP0), edges=("cols3",)), ALL_LISTS),
    (C((2, 16, 96, 8, 16, 24), ROLE, 1, 1, 24, env=MT, edges=("cols3",)), ALL_LISTS),
    (C((2, 16, 96, 8, 16, 24), BIG, 1, 1, 24, env=_join(MT, PP2), edges=("cols3",)), ALL_LISTS),
    (C((1, 16, 96, 8, 16, 24), D4, 1, 1, 12, edges=("cols3",)), ("frames3",)),                    # roi_frames = 3 on an N = 1 volume
    (C((1, 16, 96, 8, 16, 24), ROLE, 1, 1, 12, env=MT, edges=("cols3",)), ("frames3",)),
    # split launches (the ordered reduce writes every voxel: only the listed tiles are checked), with one and several chunks per split
    (C((2, 32, 96, 8, 16, 24), D4, 2, 1, 24), ("corner+volume",)),
    (C((2, 768, 192, 4, 16, 16), D4, 16, 3, 8), ("corner+volume",)),
    (C((3, 48, 96, 2, 8, 16), D2, 3, 1, 6), ("corner+volume",)),
    (C((1, 768, 96, 6, 16, 16), D2, 24, 2, 12), ("frames3",)),
    # unsplit launches with several chunks
    (C((1, 48, 96, 2, 112, 112), D2, 1, 3, 196), ("frames3",)),
    (C((1, 48, 96, 4, 80, 80), D4, 1, 3, 100, env=WINO_OFF), ("frames3",)),
    # the whole volume of a walk shape: the tile list is longer than the grid
    (C((1, 16, 96, 2, 184, 192), D2, 1, 1, 552, edges=("walk",)), ("volume",)),
    (C((1, 32, 96, 2, 184, 192), D2, 1, 2, 552, edges=("walk",)), ("volume",)),
    (C((1, 16, 96, 4, 136, 136), D4, 1, 1, 289, env=WINO_OFF, edges=("walk",)), ("volume",)),
    (C((1, 32, 96, 4, 136, 136), D4, 1, 2, 289, env=WINO_OFF, edges=("walk",)), ("volume",)),
] + [(C(s, kern, sp, cps, tiles, env=_join(MT, pp), edges=edges), ("corner+volume" if s[0] > 1 else "frames3",))
     for kern, pp, half in SCHEDULES[:3] for s, sp, cps, tiles, edges in WINO_SHAPES[2:] + [WINO_UNSPLIT]] + \
    [(C((1, ci, 96, 4, 136, 136), kern, 1, ci // 16, 289, env=pp, edges=("walk",)), ("volume",))
     for kern, pp, half in SCHEDULES[:3] for ci in (16, 32)]
# a D = 2 shape that takes the two-frame kernel as a full launch plans the direct kernel with roi = 1
ROI_TWO_FRAME = (C((3, 32, 96, 2, 8, 8), TWO, 2, 1, 2, env=MT), C((3, 32, 96, 2, 8, 8), D2, 2, 1, 3, env=MT))

# ---- e. bwd-data: shape = (N, channels of dy, channels of dx, D, H, W), the launch's own (N, Ci, Co, ...) -------------------------------
BWD_CASES = [
    C((1, 16, 96, 2, 8, 8), D2, 1, 1, 1),
    C((3, 48, 96, 2, 8, 16), D2, 3, 1, 6),
    C((1, 48, 192, 4, 8, 16), D4, 3, 1, 2),
    C((3, 16, 96, 4, 16, 8), LOCKSTEP, 1, 1, 6, env=_join(MT, PP0)),
    C((3, 16, 96, 4, 16, 8), ROLE, 1, 1, 6, env=MT),
    C((3, 16, 96, 4, 16, 8), BIG, 1, 1, 6, env=_join(MT, PP2)),
    C((1, 192, 96, 4, 8, 8), ROLE, 12, 1, 1, env=MT),
    C((3, 32, 96, 2, 8, 8), TWO, 2, 1, 2, env=MT, edges=("odd-batch",)),
]
BWD_ROI_CASES = [
    (C((2, 16, 96, 8, 16, 24), D4, 1, 1, 24), ALL_LISTS),
    (C((2, 16, 96, 8, 16, 24), ROLE, 1, 1, 24, env=MT), ALL_LISTS),
]

# ---- f. the 1x1x1 kernel: (shape, (ks, column tiles per wave, grid x, grid y, workgroup size)) ----------------------------------------
K1_CASES = [
    ((1, 256, 96, 2, 8, 64), (8, 2, 16, 1, 512)),
    ((1, 400, 96, 2, 8, 64), (8, 2, 16, 1, 512)),       # 25 chunks over 8 waves: an uneven channel share
    ((1, 128, 96, 2, 8, 64), (4, 2, 16, 1, 256)),
    ((1, 16, 96, 2, 8, 64), (1, 1, 8, 1, 256)),
    ((3, 48, 192, 2, 8, 64), (1, 1, 24, 2, 256)),       # three samples, grid y = 2
    ((1, 16, 96, 1, 1, 65600), (1, 2, 257, 1, 256)),    # 1025 wave tiles: the last workgroup has one live wave
]
K1_REFUSED = [(1, 16, 96, 1, 8, 120),      # 960 voxels: just below MPHIP_F16X3_K1_MIN's default of 1024
              (1, 16, 96, 2, 8, 65)]       # D*H*W % 64 != 0

# ---- g. power-of-two magnitudes: one single-tile case per kernel family -----------------------------------------------------------------
MAGNITUDE_CASES = [
    (3, C((1, 16, 96, 2, 8, 8), D2, 1, 1, 1, edges=("one-tile",))),
    (3, C((1, 16, 96, 4, 8, 8), ROLE, 1, 1, 1, env=MT, edges=("one-tile",))),
    (3, C((2, 16, 96, 2, 8, 8), TWO, 1, 1, 1, env=MT, edges=("one-tile",))),
    (1, ((1, 16, 96, 2, 8, 64), (1, 1, 8, 1, 256))),
]
X_EXPONENTS, W_EXPONENTS = (-100, -30, 30, 100), (-30, 30)

# ---- h. rounding: one Gaussian case per kernel and per 1x1x1 instantiation ---------------------------------------------------------------
ROUNDING_CASES = [
    (3, C((3, 48, 96, 2, 8, 16), D2, 3, 1, 6)),
    (3, C((1, 48, 192, 4, 8, 16), D4, 3, 1, 2)),
    (3, C((2, 96, 96, 4, 8, 8), LOCKSTEP, 6, 1, 2, env=_join(MT, PP0))),
    (3, C((2, 96, 96, 4, 8, 8), ROLE, 6, 1, 2, env=MT)),
    (3, C((2, 96, 96, 4, 8, 8), BIG, 6, 1, 2, env=_join(MT, PP2))),
    (3, C((3, 32, 96, 2, 8, 8), TWO, 2, 1, 2, env=MT)),
    (1, K1_CASES[0]), (1, K1_CASES[2]), (1, K1_CASES[4]), (1, ((1, 48, 96, 1, 1, 65600), (1, 2, 257, 1, 256))),
]


def case_id(case):
    if isinstance(case, tuple) and not isinstance(case, Case):
        if len(case) == 2 and isinstance(case[0], int):          # (k, case)
            return f"k{case[0]}-" + case_id(case[1])
        if isinstance(case[0], Case):                            # (case, extra)
            return case_id(case[0])
        shape, claim = case                                      # a 1x1x1 row
        n, ci, co, d, h, w = shape
        return f"k1<{claim[0]},{claim[1]}>-{n}x{ci}x{co}@{d}x{h}x{w}"
    n, ci, co, d, h, w = case.shape
    env = "".join("-" + k.replace("MPHIP_", "").lower() + v for k, v in case.env)
    return (f"{KERNEL_NAMES[case.kernel]}-{n}x{ci}x{co}@{d}x{h}x{w}-s{case.splits}-c{case.cps}-t{case.tiles}{env}"
            + ("-half" if case.half else "") + "".join(f"-{e}" for e in case.edges))


def set_switches(monkeypatch, env):
    """the per-call switches as the case wants them: the ones it names set, every other one unset"""
    for name in PER_CALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in dict(env).items():
        monkeypatch.setenv(name, value)


def conv3d_plan(lib, shape, roi=False, half=False):
    """mphip_debug_conv3d_plan under the half-products flag `half`; (0, ...) when the shape takes no precision-1 3x3x3 launch"""
    out = (ctypes.c_int * 12)()
    prev = lib.mphip_conv3d_set_half_products(int(half))
    try:
        ok = lib.mphip_debug_conv3d_plan(*shape, int(roi), out)
    finally:
        lib.mphip_conv3d_set_half_products(prev)
    return ok, tuple(out)


def k1_plan(lib, shape):
    out = (ctypes.c_int * 5)()
    return lib.mphip_debug_conv3d_k1_plan(*shape, out), tuple(out)


def resident(kernel):
    """workgroups of one resident round: 256 CUs, two workgroups each for the (2,8,8) kernel"""
    return 512 if kernel == D2 else 256


def edge_holds(edge, case, plan):
    n, ci, co, d, h, w = case.shape
    kern, td = plan[0], plan[1]
    gx, gy, gz = plan[9:12]
    if edge == "one-tile":
        return gx == 1
    if edge == "one-chunk":
        return ci == 16
    if edge == "gridy2":
        return gy == 2
    if edge == "cols3":                    # a middle tile column: halos on both sides
        return w // 8 >= 3
    if edge == "depth3":
        return kern != TWO and d // td >= 3
    if edge == "ci>768":                   # above every F(2,3) limit, the two-frame mode's included
        return ci > 768
    if edge == "ci=384":                   # the 4-plane F(2,3) kernels' limit
        return ci == 384 and plan[6] == 384
    if edge == "odd-batch":                # the two-frame mode's last tile holds one frame
        return kern == TWO and n % 2 == 1
    if edge == "no-switch":
        return not case.env
    if edge == "walk":                     # more logical workgroups than one resident round, and an uneven share of the tiles
        launched = min(gx, -(-resident(kern) // (gy * gz)))
        return gx * gy * gz > resident(kern) and gx % launched != 0
    raise AssertionError(f"unknown edge {edge}")


def claim_holds(lib, case, roi=False):
    """the library reports the plan the case claims (under the switches already set), precision 1 is supported, every named edge holds"""
    n, ci, co, d, h, w = case.shape
    assert lib.mphip_conv3d_supported(*case.shape, 3, 1) == 1, case_id(case)
    ok, plan = conv3d_plan(lib, case.shape, roi, case.half)
    assert ok == 1, case_id(case)
    got = (plan[0], plan[7], plan[8], plan[9], plan[10], plan[11])
    assert got == (case.kernel, case.splits, case.cps, case.tiles, co // 96, case.splits), (case_id(case), plan)
    assert case.splits * case.cps >= ci // 16 > (case.splits - 1) * case.cps
    for e in case.edges:
        assert edge_holds(e, case, plan), (case_id(case), e, plan)
    return plan


def k1_claim_holds(lib, row):
    shape, claimed = row
    assert lib.mphip_conv3d_supported(*shape, 1, 1) == 1
    ok, plan = k1_plan(lib, shape)
    assert ok == 1 and plan == claimed, (case_id(row), plan)
    return plan


def plan_class(plan, roi):
    """(kernel, splits > 1, chunks per split > 1, roi, logical workgroups beyond one resident round)"""
    return (plan[0], plan[7] > 1, plan[8] > 1, bool(roi), plan[9] * plan[10] * plan[11] > resident(plan[0]))


def covered_plan_rows():
    """every (case, roi) of the tables above that launches a 3x3x3 kernel: what the host file checks and classifies"""
    rows = [(c, False) for c in FWD_CASES + GN_CASES + BWD_CASES] + [(c, False) for c, _ in GNIN_CASES]
    rows += [(c, True) for c, _ in ROI_CASES + BWD_ROI_CASES]
    rows += [(ROI_TWO_FRAME[0], False), (ROI_TWO_FRAME[1], True)]
    rows += [(c, False) for k, c in MAGNITUDE_CASES + ROUNDING_CASES if k == 3]
    return rows


def covered_k1_rows():
    return K1_CASES + [c for k, c in MAGNITUDE_CASES + ROUNDING_CASES if k == 1]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from megaportrait_hack_amd import _lib, ops

    _lib.load()
    return ops


@pytest.fixture(scope="module")
def lib():
    from megaportrait_hack_amd import _lib

    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- references
def _ints(shape, gen, top=4):
    t = torch.randint(-top, top + 1, shape, generator=gen).float()
    t.view(-1)[0] = float(top)      # the maximum is `top` whatever the draw: the operand scale is fixed
    return t


def exactness_bound(k, ci, wino, X=4, Wm=4):
    """the largest partial sum, in units of the products' common power of two (module docstring); must stay below 2^24"""
    return 3 * 9 * ci * 2 * X * 3 * Wm if wino else k ** 3 * ci * X * Wm


@functools.lru_cache(maxsize=None)
def int_case(k, shape):
    """(x, w, bias, float64 conv without bias) of an integer case, computed once per shape and left unchanged"""
    n, ci, co, d, h, w = shape
    assert exactness_bound(k, ci, k == 3) < EXACT
    gen = torch.Generator().manual_seed(zlib.crc32(repr((k, shape)).encode()))
    x, wt = _ints((n, ci, d, h, w), gen), _ints((co, ci, k, k, k), gen)
    bias = torch.randint(-8, 9, (co,), generator=gen).float()
    assert x.abs().max().item() == 4 and wt.abs().max().item() == 4
    want = F.conv3d(x.double(), wt.double(), None, padding=k // 2)
    assert torch.equal(F.conv3d(x, wt, None, padding=k // 2).double(), want)      # a condition on the inputs: ATen's fp32 conv is exact on them
    assert want.abs().max().item() + 8 < EXACT
    return x, wt, bias, want


@functools.lru_cache(maxsize=None)
def bwd_case(k, shape):
    """(dy, forward weight [channels of dy, channels of dx, k, k, k], float64 dx) of an integer bwd-data case"""
    n, ci, co, d, h, w = shape
    assert exactness_bound(k, ci, k == 3) < EXACT
    gen = torch.Generator().manual_seed(zlib.crc32(repr(("bwd", k, shape)).encode()))
    dy, wt = _ints((n, ci, d, h, w), gen), _ints((ci, co, k, k, k), gen)
    want = F.conv_transpose3d(dy.double(), wt.double(), None, padding=k // 2)
    assert torch.equal(F.conv_transpose3d(dy, wt, None, padding=k // 2).double(), want)
    return dy, wt, want


def with_bias(want, bias):
    return (want + bias.double().view(1, -1, 1, 1, 1)).float()


def _loose_range(x, dev, factor=1000.0):
    """{0, 0, factor * max|x|, 0}: derive mode, no partial maxima, a rigorous but loose bound"""
    rng = torch.zeros(4100, dtype=torch.float32)
    rng[2] = factor * x.abs().max().item()
    return rng.to(dev)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(code, what):
    from megaportrait_hack_amd import _lib

    _lib.check(code, what)


_RECORD = {}


def _note(test, case, ratio):
    """worst err / bar per test; rewritten on every call when MPHIP_PARITY_JSON names a file"""
    cur = _RECORD.setdefault(test, {"worst_err_over_bar": -1.0, "at": None, "checks": 0})
    cur["checks"] += 1
    if ratio > cur["worst_err_over_bar"]:
        cur["worst_err_over_bar"], cur["at"] = float(f"{ratio:.4g}"), case
    out = os.environ.get("MPHIP_PARITY_JSON")
    if out:
        with open(out, "w") as f:
            json.dump({"what": "tests/test_gpu_conv_f16x3_branches.py: worst max|got - t64| / bar per test (bar = 4 * max|t32 - t64| + 2^-21 * A; A = "
                               "max sum |x||w|, in the transformed domain for the F(2,3) kernels), and the case it occurred at",
                       "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "tests": _RECORD}, f, indent=1)
            f.write("\n")


# ---------------------------------------------------------------------------------------------------------------- a. forward
def _split_slabs(ops, lib, xd, pc, shape, plan):
    """the launch's split-K slabs [splits, N, Co, D, H, W] (bias not added): ops.conv3d_split where it keeps them, else the entry it calls"""
    n, ci, co, d, h, w = shape
    if ops.conv3d_split_slabs(xd.shape, pc, 1) > 1:
        out = ops.conv3d_split(xd, pc, precision=1)
        assert out.splits == plan[7] and out.bias is pc.bias
        return out.data
    out = torch.full((plan[7], n, co, d, h, w), float("nan"), dtype=torch.float32, device=xd.device)
    _check(lib.mphip_conv3d_fwd_split(P(xd), P(ops.absmax_range(xd)), P(pc.packed(1)), P(pc.bias), P(out), n, ci, co, d, h, w, 3, 1, None, 0,
                                      _stream()), "mphip_conv3d_fwd_split")
    return out


@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_forward_bit_exact(ops, lib, dev, monkeypatch, case):
    set_switches(monkeypatch, case.env)
    with ops.half_products(case.half):
        plan = claim_holds(lib, case)
        n, ci, co, d, h, w = case.shape
        x, wt, bias, want = int_case(3, case.shape)
        want_b, want_0 = with_bias(want, bias), want.float()
        xd = x.to(dev)
        pc_b, pc_0 = ops.PackedConv(wt.to(dev), bias.to(dev)), ops.PackedConv(wt.to(dev), None)
        assert ops.tensor_range(xd) is None
        first = ops.conv3d(xd, pc_b, precision=1)                                  # the range is left to the library
        assert torch.equal(first.cpu(), want_b), "bias, library-measured range"
        assert torch.equal(ops.conv3d(xd, pc_b, precision=1), first), "second launch"
        assert torch.equal(ops.conv3d(xd, pc_0, precision=1).cpu(), want_0), "no bias"
        assert torch.equal(ops.conv3d(xd, pc_b, precision=1, x_range=ops.absmax_range(xd)).cpu(), want_b), "range of absmax_range"
        assert torch.equal(ops.conv3d(xd, pc_0, precision=1, x_range=_loose_range(x, dev)).cpu(), want_0), "explicit loose bound, no bias"
        assert torch.equal(ops.conv3d(xd, pc_b, precision=1, x_range=_loose_range(x, dev)).cpu(), want_b), "explicit loose bound"
        if case.splits > 1:
            # each slab is the conv of its own channels: pins the chunk-to-split mapping, which the sum alone does not
            slabs = _split_slabs(ops, lib, xd, pc_b, case.shape, plan).cpu()
            assert tuple(slabs.shape) == (case.splits, n, co, d, h, w)
            per = case.cps * 16
            for s in range(case.splits):
                lo, hi = s * per, min(ci, (s + 1) * per)
                part = F.conv3d(x[:, lo:hi].double(), wt[:, lo:hi].double(), None, padding=1)
                assert torch.equal(slabs[s].double(), part), f"slab {s}: channels [{lo}, {hi})"
            assert torch.equal((slabs.double().sum(0) + bias.double().view(1, -1, 1, 1, 1)).float(), want_b)


# ---------------------------------------------------------------------------------------------------------------- b. fused input affine
def _affine_table(n, ci, gen):
    """[N][Ci][2] = (scale in {-2..2}, shift in [-3, 3]), drawn per frame and channel: almost every channel's pair differs between frames"""
    scale = torch.randint(-2, 3, (n, ci), generator=gen).float()
    shift = torch.randint(-3, 4, (n, ci), generator=gen).float()
    scale[0, :5] = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0])
    shift[-1, :2] = torch.tensor([-3.0, 3.0])
    table = torch.stack([scale, shift], dim=-1).contiguous()
    for i in range(1, n):
        assert ((table[i] != table[0]).any(dim=-1)).float().mean().item() > 0.75      # the frames' tables differ
    return table


def _gnin_launch(lib, xd, table, rng, relu, pc, shape, gn_groups=0):
    n, ci, co, d, h, w = shape
    y = torch.full((n, co, d, h, w), float("nan"), dtype=torch.float32, device=xd.device)
    if gn_groups:
        ws_bytes = lib.mphip_conv3d_gn_workspace_bytes(n, ci, co, d, h, w, 3, 1, gn_groups)
        stats = torch.empty((n * gn_groups, 2), dtype=torch.float32, device=xd.device)
    else:
        ws_bytes = lib.mphip_conv3d_workspace_bytes(n, ci, co, d, h, w, 3, 1)
        stats = None
    ws = torch.empty((ws_bytes + 7) // 8 + 1, dtype=torch.float64, device=xd.device)
    if gn_groups:
        _check(lib.mphip_conv3d_gnin_gn_fwd(P(xd), P(table), P(rng), int(relu), P(pc.packed(1)), P(pc.bias), P(y), P(stats), n, ci, co, d, h, w,
                                            3, 1, gn_groups, 1e-5, P(ws), ws_bytes, _stream()), "mphip_conv3d_gnin_gn_fwd")
    else:
        _check(lib.mphip_conv3d_gnin_fwd(P(xd), P(table), P(rng), int(relu), P(pc.packed(1)), P(pc.bias), P(y), n, ci, co, d, h, w, 3, 1,
                                         P(ws), ws_bytes, _stream()), "mphip_conv3d_gnin_fwd")
    return y, stats


def _gn_stats_module():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_gpu_groupnorm_stats as GS          # its bars: fp32 rounding of the stored mean, 1e-5 relative on rstd

    return GS


@pytest.mark.parametrize("case,with_gn", GNIN_CASES, ids=[case_id(c) for c, _ in GNIN_CASES])
def test_fused_input_affine_bit_exact(ops, lib, dev, monkeypatch, case, with_gn):
    """conv(pad0(relu?(x * scale + shift))): the affine reaches every in-volume voxel with its own frame's and channel's pair, and the
    padding stays 0 (a shift that leaks into the halo shows)"""
    set_switches(monkeypatch, case.env)
    plan = claim_holds(lib, case)
    n, ci, co, d, h, w = case.shape
    assert ci <= plan[6] and exactness_bound(3, ci, case.kernel >= LOCKSTEP, X=11) < EXACT
    x, wt, bias, _ = int_case(3, case.shape)
    table = _affine_table(n, ci, torch.Generator().manual_seed(zlib.crc32(repr(case.shape).encode())))
    xd, td = x.to(dev), table.to(dev)
    rng = torch.zeros(4100, dtype=torch.float32)
    rng[2] = 11.0
    rng = rng.to(dev)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    for relu in (0, 1):
        xa = x.double() * table[:, :, 0].double().view(n, ci, 1, 1, 1) + table[:, :, 1].double().view(n, ci, 1, 1, 1)
        if relu:
            xa = xa.clamp_min(0.0)
        assert xa.abs().max().item() <= 11
        want = with_bias(F.conv3d(xa, wt.double(), None, padding=1), bias)
        assert torch.equal(F.conv3d(xa.float(), wt, bias, padding=1), want)
        y, _ = _gnin_launch(lib, xd, td, rng, relu, pc, case.shape)
        assert torch.equal(y.cpu(), want), f"in_relu = {relu}"
        if with_gn:
            y2, stats = _gnin_launch(lib, xd, td, rng, relu, pc, case.shape, gn_groups=32)
            assert torch.equal(y2.cpu(), want), f"in_relu = {relu}, GroupNorm epilogue"
            _gn_stats_module().check_stats(f"{case_id(case)} gnin relu {relu}", stats.cpu(), want, 32)


# ---------------------------------------------------------------------------------------------------------------- c. gn_groups = 32
@pytest.mark.parametrize("case", GN_CASES, ids=case_id)
def test_groupnorm_epilogue_bit_exact_y_and_statistics(ops, lib, dev, monkeypatch, case):
    set_switches(monkeypatch, case.env)
    claim_holds(lib, case)
    x, wt, bias, want = int_case(3, case.shape)
    want_b = with_bias(want, bias)
    y, stats = ops.conv3d(x.to(dev), ops.PackedConv(wt.to(dev), bias.to(dev)), precision=1, gn_groups=32)
    assert torch.equal(y.cpu(), want_b)
    _gn_stats_module().check_stats(case_id(case), stats.cpu(), want_b, 32)


# ---------------------------------------------------------------------------------------------------------------- d. demand-driven
def roi_boxes(name, shape, tile):
    """(boxes {lx, ly, lz, ex, ey, ez} , roi_frames) of a named list for this shape and tile"""
    n, _, _, d, h, w = shape
    td, th, tw = tile
    straddle = (tw - 2, th - 3, 0, min(4, w - tw + 2), min(6, h - th + 3), min(d, td // 2 + 1))      # crosses tile edges where the volume has them
    if name == "tile-edges":      # ends exactly on a tile edge in each axis (inner edges where the axis has one) / starts on one
        boxes = [(2, 3, 0, tw - 2, th - 3, td), (tw, th, td if d > td else 0, 1, 1, 1)]
        assert (boxes[0][0] + boxes[0][3]) % tw == 0 and boxes[0][0] + boxes[0][3] < w and (boxes[0][1] + boxes[0][4]) % th == 0
        assert (boxes[0][2] + boxes[0][5]) % td == 0 and boxes[1][0] % tw == 0 and boxes[1][1] % th == 0 and boxes[1][2] % td == 0
    elif name == "corner+volume":
        boxes = [(w - 1, h - 1, d - 1, 1, 1, 1), (0, 0, 0, w, h, d)]
    elif name == "empty+straddle":      # frame 0's box has zero extent: it lists no tile
        boxes = [(tw, 0, 0, 0, h, d), straddle]
        assert straddle[0] // tw != (straddle[0] + straddle[3] - 1) // tw and straddle[1] // th != (straddle[1] + straddle[4] - 1) // th
    elif name == "frames3":             # one volume, three boxes
        assert n == 1
        return [(0, 0, 0, 1, 1, 1), (w - 1, h - 1, d - 1, 1, 1, 1), straddle], 3
    elif name == "volume":
        return [(0, 0, 0, w, h, d)] * n, 0
    else:
        raise AssertionError(name)
    assert n >= 2
    return boxes + [straddle] * (n - 2), 0


def listed_voxels(shape, tile, boxes, roi_frames, dilate=0):
    """[N, D, H, W] bool: the voxels of the tiles roi_tile_list_kernel (csrc/conv3d_f16x3.hip) lists: a tile [t0, t0 + T) is listed when
    it overlaps its frame's box (grown by `dilate` voxels) on every axis; a box with no extent on a tile edge lists nothing"""
    n, _, _, d, h, w = shape
    td, th, tw = tile
    need = torch.zeros((n, d, h, w), dtype=torch.bool)
    for i in range(n):
        for lx, ly, lz, ex, ey, ez in (boxes if roi_frames else [boxes[i]]):
            for d0 in range(0, d, td):
                for h0 in range(0, h, th):
                    for w0 in range(0, w, tw):
                        if (w0 < lx + ex + dilate and w0 + tw > lx - dilate and h0 < ly + ey + dilate and h0 + th > ly - dilate
                                and d0 < lz + ez + dilate and d0 + td > lz - dilate):
                            need[i, d0:d0 + td, h0:h0 + th, w0:w0 + tw] = True
    return need


def _roi_tensor(boxes, dev):
    return torch.tensor([list(b) + [0, 0] for b in boxes], dtype=torch.int32).to(dev)


ROI_PARAMS = [(c, nm) for c, names in ROI_CASES for nm in names]


@pytest.mark.parametrize("case,name", ROI_PARAMS, ids=[f"{case_id(c)}-{nm}" for c, nm in ROI_PARAMS])
def test_demand_driven_launch_writes_the_listed_tiles_exactly_and_nothing_else(ops, lib, dev, monkeypatch, case, name):
    set_switches(monkeypatch, case.env)
    plan = claim_holds(lib, case, roi=True)
    assert plan[5] == 1                                                  # the kernel accepts a tile list
    n, ci, co, d, h, w = case.shape
    tile = (ctypes.c_int * 3)()
    assert lib.mphip_conv3d_roi_granule(n, ci, co, d, h, w, 3, 1, tile) == 1 and tuple(tile) == plan[1:4]
    boxes, frames = roi_boxes(name, case.shape, tuple(tile))
    need = listed_voxels(case.shape, tuple(tile), boxes, frames)
    if name == "empty+straddle":
        assert not bool(need[0].any())
    if name in ("corner+volume", "volume"):
        assert bool(need[-1].all())
    assert bool(need.any())
    x, wt, bias, want = int_case(3, case.shape)
    want_b = with_bias(want, bias)
    xd = x.to(dev)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    y = torch.full((n, co, d, h, w), float("nan"), dtype=torch.float32, device=dev)
    ws_bytes = lib.mphip_conv3d_roi_workspace_bytes(n, ci, co, d, h, w, 3, 1)
    ws = torch.empty((ws_bytes + 7) // 8 + 1, dtype=torch.float64, device=dev)
    _check(lib.mphip_conv3d_fwd_roi(P(xd), P(ops.absmax_range(xd)), P(pc.packed(1)), P(pc.bias), P(y), P(_roi_tensor(boxes, dev)), frames,
                                    n, ci, co, d, h, w, 3, 1, P(ws), ws_bytes, _stream()), "mphip_conv3d_fwd_roi")
    y = y.cpu()
    mask = need[:, None].expand_as(y)
    assert torch.equal(y[mask], want_b[mask]), "listed tiles"
    if case.splits == 1:
        assert bool(torch.isnan(y[~mask]).all()), "an unsplit launch wrote outside the listed tiles"


def test_a_two_frame_shape_plans_the_direct_kernel_on_demand(ops, lib, dev, monkeypatch):
    full, demand = ROI_TWO_FRAME
    set_switches(monkeypatch, full.env)
    assert claim_holds(lib, full)[5] == 0                                # the two-frame mode takes no tile list
    plan = claim_holds(lib, demand, roi=True)
    n, ci, co, d, h, w = demand.shape
    x, wt, bias, want = int_case(3, demand.shape)
    want_b = with_bias(want, bias)
    boxes, frames = roi_boxes("corner+volume", demand.shape, plan[1:4])
    need = listed_voxels(demand.shape, plan[1:4], boxes, frames)[:, None].expand_as(want_b)
    xd = x.to(dev)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    y = ops.conv3d_roi(xd, pc, _roi_tensor(boxes, dev)).cpu()
    assert torch.equal(y[need], want_b[need])
    assert torch.equal(ops.conv3d(xd, pc, precision=1).cpu(), want_b)    # the full launch (two-frame kernel): the same bits


# ---------------------------------------------------------------------------------------------------------------- e. bwd-data
def _bwd_launch(ops, dyd, wt, dev, roi=None):
    _, scale = ops.grad_prep(dyd, want_bias=False)
    assert scale.cpu().tolist()[:3] == [2.0 ** 11, 2.0 ** -11, 4.0]
    return ops.conv3d_bwd_data(dyd, ops.PackedConv(wt.to(dev), None, transposed=True), scale, precision=1, roi=roi)


@pytest.mark.parametrize("case", BWD_CASES, ids=case_id)
def test_bwd_data_bit_exact(ops, lib, dev, monkeypatch, case):
    set_switches(monkeypatch, case.env)
    claim_holds(lib, case)
    n, ci, co, d, h, w = case.shape
    assert ci != co
    dy, wt, want = bwd_case(3, case.shape)
    dyd = dy.to(dev)
    dx = _bwd_launch(ops, dyd, wt, dev)
    assert tuple(dx.shape) == (n, co, d, h, w) and torch.equal(dx.cpu(), want.float())
    assert torch.equal(_bwd_launch(ops, dyd, wt, dev), dx), "second launch"


@pytest.mark.parametrize("row", K1_CASES, ids=case_id)
def test_bwd_data_1x1x1_bit_exact(ops, lib, dev, monkeypatch, row):
    set_switches(monkeypatch, {})
    k1_claim_holds(lib, row)
    shape, _ = row
    assert shape[1] != shape[2]
    dy, wt, want = bwd_case(1, shape)
    dx = _bwd_launch(ops, dy.to(dev), wt, dev)
    assert torch.equal(dx.cpu(), want.float())


BWD_ROI_PARAMS = [(c, nm) for c, names in BWD_ROI_CASES for nm in names]


@pytest.mark.parametrize("case,name", BWD_ROI_PARAMS, ids=[f"{case_id(c)}-{nm}" for c, nm in BWD_ROI_PARAMS])
def test_bwd_data_roi_is_exact_inside_and_zero_outside(ops, lib, dev, monkeypatch, case, name):
    """dy is zero outside one box per frame: dx is exact in the tiles the boxes grown by one voxel touch and exactly 0 elsewhere"""
    set_switches(monkeypatch, case.env)
    plan = claim_holds(lib, case, roi=True)
    n, ci, co, d, h, w = case.shape
    boxes, frames = roi_boxes(name, case.shape, plan[1:4])
    assert frames == 0
    full, wt, _ = bwd_case(3, case.shape)
    dy = torch.zeros_like(full)
    for i, (lx, ly, lz, ex, ey, ez) in enumerate(boxes):
        dy[i, :, lz:lz + ez, ly:ly + ey, lx:lx + ex] = full[i, :, lz:lz + ez, ly:ly + ey, lx:lx + ex]
    dy[-1].view(-1)[dy[-1].view(-1).nonzero()[0]] = 4.0                  # (every list's last frame has a box with voxels) the maximum is 4
    want = F.conv_transpose3d(dy.double(), wt.double(), None, padding=1)
    assert torch.equal(F.conv_transpose3d(dy, wt, None, padding=1).double(), want)
    inside = listed_voxels(case.shape, plan[1:4], boxes, 0, dilate=1)[:, None].expand_as(want)
    assert not bool(want[~inside].any())                                 # (the gradient of a box reaches one voxel beyond it)
    if name != "corner+volume":
        assert not bool(inside.all())
    dx = _bwd_launch(ops, dy.to(dev), wt, dev, roi=_roi_tensor(boxes, dev)).cpu()
    assert torch.equal(dx[inside], want.float()[inside]), "inside the listed tiles"
    assert not bool(dx[~inside].any()), "dx is not 0 outside the listed tiles"


# ---------------------------------------------------------------------------------------------------------------- f. 1x1x1 forward
@pytest.mark.parametrize("row", K1_CASES, ids=case_id)
def test_forward_1x1x1_bit_exact(ops, lib, dev, monkeypatch, row):
    set_switches(monkeypatch, {})
    k1_claim_holds(lib, row)
    shape, _ = row
    x, wt, bias, want = int_case(1, shape)
    want_b = with_bias(want, bias)
    xd = x.to(dev)
    pc_b, pc_0 = ops.PackedConv(wt.to(dev), bias.to(dev)), ops.PackedConv(wt.to(dev), None)
    first = ops.conv3d(xd, pc_b, precision=1)
    assert torch.equal(first.cpu(), want_b)
    assert torch.equal(ops.conv3d(xd, pc_b, precision=1), first), "second launch"
    assert torch.equal(ops.conv3d(xd, pc_0, precision=1).cpu(), want.float()), "no bias"
    assert torch.equal(ops.conv3d(xd, pc_b, precision=1, x_range=ops.absmax_range(xd)).cpu(), want_b)
    assert torch.equal(ops.conv3d(xd, pc_b, precision=1, x_range=_loose_range(x, dev)).cpu(), want_b), "explicit loose bound"


@pytest.mark.parametrize("shape", K1_REFUSED, ids=lambda s: "x".join(map(str, s)))
def test_1x1x1_outside_the_supported_set_is_the_exact_fp32_kernel(ops, lib, dev, monkeypatch, shape):
    set_switches(monkeypatch, {})
    assert lib.mphip_conv3d_supported(*shape, 1, 1) == 0 and k1_plan(lib, shape) == (0, (0, 0, 0, 0, 0))
    x, wt, bias, want = int_case(1, shape)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    y = ops.conv3d(x.to(dev), pc, precision=1)
    assert torch.equal(y.cpu(), with_bias(want, bias))
    assert torch.equal(ops.conv3d(x.to(dev), pc, precision=0), y)


# ---------------------------------------------------------------------------------------------------------------- g. magnitudes
MAGNITUDE_PARAMS = [(k, c, p, q) for k, c in MAGNITUDE_CASES for p in X_EXPONENTS for q in W_EXPONENTS]


@pytest.mark.parametrize("k,case,p,q", MAGNITUDE_PARAMS,
                         ids=[f"{case_id((k, c)) if k == 3 else case_id(c)}-x2^{p}-w2^{q}" for k, c, p, q in MAGNITUDE_PARAMS])
def test_power_of_two_magnitudes_are_exact(ops, lib, dev, monkeypatch, k, case, p, q):
    """x = integers * 2^p, w = integers * 2^q: the result is the integer conv times 2^(p+q), rounded to fp32 (Inf at 2^130, fp32
    subnormals and small normals at 2^-130), bit for bit.  At (p, q) = (-100, -30) the kernels' single unscale factor 2^-153 was 0."""
    if k == 3:
        set_switches(monkeypatch, case.env)
        claim_holds(lib, case)
        shape = case.shape
    else:
        set_switches(monkeypatch, {})
        k1_claim_holds(lib, case)
        shape = case[0]
    x, wt, _, truth = int_case(k, shape)
    xs, ws = (x.double() * 2.0 ** p).float(), (wt.double() * 2.0 ** q).float()
    assert torch.equal(xs.double(), x.double() * 2.0 ** p) and torch.equal(ws.double(), wt.double() * 2.0 ** q)
    want = (truth * 2.0 ** (p + q)).float()                 # float64 holds truth * 2^(p+q) exactly; one rounding to fp32
    if abs(p + q) < 120:
        assert torch.equal(want.double(), truth * 2.0 ** (p + q)) and bool(torch.isfinite(want).all())
    xd = xs.to(dev)
    y = ops.conv3d(xd, ops.PackedConv(ws.to(dev), None), precision=1)
    assert torch.equal(y.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------- h. rounding
def _split_f16(t, top):
    """(hi, lo) of t at its power-of-two operand scale, unscaled, float64: what the three-product kernels multiply"""
    s = R.pow2_operand_scale(t.abs().max().item(), top)
    v = t.float() * s
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi.double() / s, lo.double() / s


def _wino_domain(x, wt):
    """(t[4] fp32, u[4] float64, sx * sw): the transformed operands at their scales, formed as conv3d_wino_f16_contract forms them"""
    x, wt = x.float(), wt.float()
    W = x.shape[-1]
    sx = R.pow2_operand_scale(x.abs().max().item(), 14)
    sw = R.pow2_operand_scale(wt.abs().max().item(), 15)
    xp = F.pad(x * sx, (1, 1))
    d = [xp[..., i:i + W:2] for i in range(4)]
    t = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]          # fp32, one rounding each
    g = wt.double()
    u = [g[..., 0], 0.5 * (g[..., 0] + g[..., 1] + g[..., 2]), 0.5 * (g[..., 0] - g[..., 1] + g[..., 2]), g[..., 2]]
    return t, [v * sw for v in u], sx * sw


def _wino_pos(tp, up):
    return F.conv3d(tp.double(), up.double().unsqueeze(-1), None, padding=(1, 1, 0))


def _wino_out(m, unit):
    return torch.stack([m[0] + m[1] + m[2], m[1] - m[2] - m[3]], dim=-1).flatten(-2) / unit


@functools.lru_cache(maxsize=None)
def rounding_case(k, shape, wino):
    """Gaussian data, its float64 conv, the bar, and the CPU evidence that the bar separates one product from three"""
    n, ci, co, d, h, w = shape
    gen = torch.Generator().manual_seed(zlib.crc32(repr(("gauss", k, shape)).encode()))
    x = torch.randn((n, ci, d, h, w), generator=gen) * 1.5
    wt = torch.randn((co, ci, k, k, k), generator=gen) * 0.05
    bias = torch.randn((co,), generator=gen)
    t64 = F.conv3d(x.double(), wt.double(), bias.double(), padding=k // 2)
    e32 = (F.conv3d(x, wt, bias, padding=k // 2).double() - t64).abs().max().item()
    b64 = bias.double().view(1, -1, 1, 1, 1)
    if wino:
        t, u, unit = _wino_domain(x, wt)
        M = [_wino_pos(tp.abs(), up.abs()) for tp, up in zip(t, u)]
        A = max((M[0] + M[1] + M[2]).max().item(), (M[1] + M[2] + M[3]).max().item()) / unit
        one = R.conv3d_wino_f16_contract(x, wt, bias)
        th = [tp.half() for tp in t]
        tl = [(tp - hp.float()).half() for tp, hp in zip(t, th)]
        uh = [up.float().half() for up in u]
        ul = [(up.float() - hp.float()).half() for up, hp in zip(u, uh)]
        three = _wino_out([_wino_pos(a, b) + _wino_pos(a, c) + _wino_pos(e, b) for a, e, b, c in zip(th, tl, uh, ul)], unit) + b64
    else:
        A = F.conv3d(x.double().abs(), wt.double().abs(), None, padding=k // 2).max().item()
        xh, xl = _split_f16(x, 14)
        wh, wl = _split_f16(wt, 15)
        assert torch.equal(xh, R.round_f16_at_scale(x)) and torch.equal(wh, R.round_f16_at_scale(wt, 15))
        conv = lambda a, b: F.conv3d(a, b, None, padding=k // 2)      # noqa: E731
        one = conv(xh, wh) + b64
        three = conv(xh, wh) + conv(xh, wl) + conv(xl, wh) + b64
    bar = 4 * e32 + 2.0 ** -21 * A
    return x, wt, bias, t64, bar, (one - t64).abs().max().item(), (three - t64).abs().max().item()


@pytest.mark.parametrize("k,case", ROUNDING_CASES, ids=[case_id((k, c)) if k == 3 else case_id(c) for k, c in ROUNDING_CASES])
def test_rounding_bar(ops, lib, dev, monkeypatch, k, case):
    """max|got - t64| <= 4 * max|t32 - t64| + 2^-21 * A on Gaussian data; the bar can fail: the one-product contract, emulated in float64,
    misses it by more than 10x, the three-product one keeps a tenth of it (no wrong kernel is involved)."""
    if k == 3:
        set_switches(monkeypatch, case.env)
        claim_holds(lib, case)
        shape, wino, name = case.shape, case.kernel >= LOCKSTEP, case_id(case)
    else:
        set_switches(monkeypatch, {})
        k1_claim_holds(lib, case)
        shape, wino, name = case[0], False, case_id(case)
    x, wt, bias, t64, bar, e1, e3 = rounding_case(k, shape, wino)
    print(f"{name}: CPU emulation, one product {e1 / bar:.1f} x bar, three products {e3 / bar:.4f} x bar")
    assert e1 >= 10 * bar, (e1, bar)
    assert e3 <= 0.1 * bar, (e3, bar)
    y = ops.conv3d(x.to(dev), ops.PackedConv(wt.to(dev), bias.to(dev)), precision=1)
    err = (y.cpu().double() - t64).abs().max().item()
    print(f"{name}: err {err:.3e}, bar {bar:.3e}, err / bar {err / bar:.4f}")
    _note("test_rounding_bar", name, err / bar)
    assert err <= bar, (err, bar)
