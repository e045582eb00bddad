"""Every branch of the 3-D f16x3 forward, 1x1x1, bwd-data and bwd-weight kernels, and of the 2-D backward kernels, exactly, on data whose
`lo` halves are NOT zero.  The three files that reach those branches on purpose (tests/test_gpu_conv_f16x3_branches.py,
tests/test_gpu_bwd_weight_f16x3_branches.py, tests/test_gpu_conv2d_bwd.py) do so on small integers, where every scaled operand is an exact
f16 and every lo half is 0: a lo fragment that is misplaced, dropped or doubled on one of those branches passes them.  This file runs their
own case tables (imported, not copied) on the method of tests/test_gpu_conv2d_exact.py: ONE operand gets fractional bits that only hi + lo
can hold, the other is a sparse integer operand, and every partial sum stays exact in fp32.

Each case first asserts the plan it claims with the helpers of the module it comes from (claim_holds / k1_claim_holds / edge_holds over
mphip_debug_conv3d_plan, mphip_debug_conv3d_k1_plan, mphip_debug_conv3d_bwd_weight_f16x3_plan, mphip_debug_conv2d_bwd_weight_plan, the
per-call switches through monkeypatch), then launches once and requires torch.equal with the float64 CPU answer cast ONCE to fp32.  There
is no tolerance in this file, and ops.f16x3_saturation_count() must be 0 after each case.

The data kinds (oracle.hotpath_ref lo_plane_operand, sparse_ints):
  forward     xlo   x = a + b*2^-11 (a integers in [-4, 4] containing a 4, |b| < 2^10), w ternary {-1, 0, 1}
              wlo   w = a + b*2^-12 (|b| < 2^11), x ternary
  bwd-data    dylo  dy = a + b*2^-11, w ternary;   wlo: w = a + b*2^-12 through the transposed pack (a pack routine of its own), dy ternary
  bwd-weight  xlo   x = a + b*2^-11, dy ternary;   dylo: dy = a + b*2^-11, x ternary
The fractional operand is dense.  The ternary one holds a 1 (its scale is fixed: 2^13 for x / dy, 2^14 for w), has non-zeros in every
16-channel K chunk, and its density is the lever: about NNZ[kind] non-zeros per output's reduction (27 * Ci weights or inputs of a 3x3x3
conv, Ci of a 1x1x1 one, N * D * H * W voxels of a weight gradient), dense where the reduction is shorter than that.

Why no tolerance, direct kernels (3x3x3 direct2 / direct4, 2-D bwd-data).  max|x| is in [4, 4.5): the x scale is 2^11 and x * 2^11 an
integer below 2^14 of up to 14 bits, which one f16 (11 bits) cannot hold and hi + lo holds exactly; lo != 0 for about half of the
elements.  The ternary w * 2^14 is an exact f16 and its lo is 0.  Every product is a whole number of units (2^-11 of the unscaled
result), and every partial sum, in any order, over any split and through the ordered reduce, is bounded by
sum (|whi| + |wlo|)(|xhi| + |xlo|) <= nnz * 2^14 units < 2^24: exact in fp32.  wlo: w * 2^12 is an integer below 2^15, the unit is
2^-12, the room half as large, so NNZ["wlo"] is half of NNZ["xlo"].  Both unscales are powers of two; bias is integers in [-8, 8] and
lin + bias is an fp32 number.

Why no tolerance, F(2,3) kernels (lockstep, rolesplit, bigtile, twoframe).  What is split is the TRANSFORMED pair: t = Bt d (one fp32
operation on two scaled inputs: an integer below 2^15, exact) and u = G g (halves of sums of three weights).  xlo: t has up to 15 bits,
hi + lo holds it; u * 2^14 is a multiple of 2^13 below 1.5 * 2^14: an exact f16, lo = 0.  wlo: u * 2^12 is a multiple of 1/2 below
1.5 * 2^15 (16 bits in half units), exact as hi + lo; t is in [-2, 2] * 2^13, an exact f16.  A position's sum runs over (ci, kd, kh); the
output transform adds three positions with rows (1,1,1,0) and (0,1,1,1) in absolute value, so the bound is taken there:
max over outputs of those row sums of sum (|thi| + |tlo|)(|uhi| + |ulo|) < 2^24 units.  The fused input affine (integer scale in {1, 2},
shift in [-3, 3], a descriptor that bounds the normalised map by 12) stages multiples of 1/2 below 2^14 at scale 2^10 (xlo): still
exact as hi + lo, and so is their t.

Why no tolerance, 1x1x1 kernels (all four instantiations, forward and bwd-data).  As the direct kernels with a reduction of Ci terms:
sum <= Ci * 2^14 units (xlo) or Ci * 2^15 (wlo), below 2^24 for Ci <= 400 with a ternary operand of NNZ non-zeros per output.

Why no tolerance, bwd-weight (3-D CONV3 / CONV1, 2-D VEC / MASKED).  x and dy are both split at the activations' scale (top 14) and the
kernels add xhi*dyhi + xhi*dylo + xlo*dyhi.  One of the two is a + b*2^-11 (scale 2^11, 14 bits, hi + lo exact), the other ternary
(scale 2^13, lo = 0), so the dropped xlo*dylo is 0 and the three products are x * dy exactly.  A dW element sums over N * D * H * W
voxels: sum (|xhi| + |xlo|)(|dyhi| + |dylo|) <= nnz * 2^14 units < 2^24, in any order, over any split of the tiles and through the slab
reduce.  dy's scale is what ops.grad_prep returns; each case asserts that it is the power of two the reference expects.

tests/test_f16x3_lo_planes_host.py asserts all of this per (case, kind) on the CPU, from the case's own data and not from these
formulas, and that a one-product emulation (or one with hi and lo swapped) is wrong on more than 90 % of the outputs, so each case can
fail.  Cases whose shape cannot meet those conditions are named, with the reason, in EXCLUDED; the host test bounds that table.

Not repeated here: the GroupNorm-epilogue cases (the statistics are taken from y and never see a lo plane) and the half=True schedule (one
product: no lo plane is read).  Measured on an MI355X: DESIGN.md 3.1c-sexies."""
import functools
import os
import sys
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_bwd_weight_f16x3_branches as WB  # noqa: E402
import test_gpu_conv2d_bwd as B2  # noqa: E402
import test_gpu_conv_f16x3_branches as FB  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT = 2 ** 24
# non-zeros of the ternary operand per output's reduction, by the kind of the FRACTIONAL operand (wlo: units of 2^15, half the room)
NNZ = {"xlo": 800, "dylo": 800, "wlo": 400}
FRAC_BITS = {"xlo": 11, "dylo": 11, "wlo": 12}

# (table, case id, kind) -> one line: why the shape cannot meet the host test's conditions with any density.  Such a case is left out of
# the parameter lists below.  Empty: the one shape that could not (the 2-D 1x1 map, three voxels per gradient element) takes the fractional
# operand whose lo halves are all odd instead (SHORT).
EXCLUDED = {}


def excluded(table, cid, kind):
    return (table, cid, kind) in EXCLUDED


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x3FFFFFFF


def _density(kind, reduction):
    return min(1.0, NNZ[kind] / float(reduction))


SHORT = 16      # a reduction of fewer terms than this takes the fractional operand whose lo halves are all odd (odd_lo_plane_operand)


def _frac(shape, kind, seed, reduction=SHORT):
    return (R.lo_plane_operand if reduction >= SHORT else R.odd_lo_plane_operand)(shape, FRAC_BITS[kind], seed)


# ------------------------------------------------------------------------------------------------------------------ conv data (CPU)
def _affine_table(n, ci, seed):
    """[N][Ci][2] = (scale in {1, 2}, shift in [-3, 3]) per frame and channel"""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(1, 3, (n, ci), generator=g).float(), torch.randint(-3, 4, (n, ci), generator=g).float()], dim=-1).contiguous()


def _box_mask(shape5, boxes):
    """[N, 1, D, H, W] bool: inside the frame's own box {lx, ly, lz, ex, ey, ez}"""
    n, _, d, h, w = shape5
    m = torch.zeros((n, 1, d, h, w), dtype=torch.bool)
    for i, (lx, ly, lz, ex, ey, ez) in enumerate(boxes):
        m[i, :, lz:lz + ez, ly:ly + ey, lx:lx + ex] = True
    return m


def _put_top(t, mask, top):
    """the first element inside the mask becomes `top`: the operand scale is fixed whatever the draw"""
    flat = (t * 0 + mask.float()).view(-1)
    t.view(-1)[flat.nonzero()[0]] = float(top)


@functools.lru_cache(maxsize=None)
def conv_data(tag, k, shape, kind, wino, dims=3, relu=None, boxes=None):
    """Everything a conv case needs, made once on the CPU and never changed.  shape = the launch's own (N, Ci, Co, [D,] H, W).
    tag "fwd": y = conv(x, w) + bias.  tag "bwd": the launch is the bwd-data conv of dy (Ci channels) through the transposed pack of the
    forward weight wt [Ci, Co, k..]; w_eq is the equivalent forward weight (flipped, transposed) the emulations multiply.
    relu not None: a fused input affine (table, ReLU or not) and the descriptor bound of the normalised map.
    boxes: (bwd) dy is zero outside one box per frame."""
    n, ci, co = shape[:3]
    vol = tuple(shape[3:])
    assert len(vol) == dims and kind in (("xlo", "wlo") if tag == "fwd" else ("dylo", "wlo"))
    seed = _seed(tag, k, shape, kind, relu, boxes)
    xs, ws = (n, ci) + vol, (co, ci) + (k,) * dims
    red = k ** dims * ci
    d = types.SimpleNamespace(tag=tag, k=k, shape=shape, kind=kind, wino=wino, dims=dims, relu=relu, boxes=boxes, table=None, x_bound=None)
    conv = F.conv3d if dims == 3 else F.conv2d
    d.conv = lambda a, b: conv(a, b, None, padding=k // 2)
    if kind == "wlo":
        d.x, d.w_eq = R.sparse_ints(xs, _density(kind, red), seed), _frac(ws, kind, seed + 1)
    else:      # (a fused affine's scale of up to 2 doubles the staged magnitudes: half the non-zeros)
        d.x, d.w_eq = _frac(xs, kind, seed), R.sparse_ints(ws, _density(kind, red * (2 if relu is not None else 1)), seed + 1)
    if boxes is not None:
        inside = _box_mask(xs, boxes)
        d.x = d.x * inside.float()
        _put_top(d.x, inside.expand_as(d.x), 1 if kind == "wlo" else 4)
    d.staged = d.x.double()
    if relu is not None:
        d.table = _affine_table(n, ci, seed + 2)
        d.staged = d.staged * d.table[:, :, 0].double().view((n, ci) + (1,) * dims) + d.table[:, :, 1].double().view((n, ci) + (1,) * dims)
        if relu:
            d.staged = d.staged.clamp_min(0.0)
        d.x_bound = 12.0 if kind == "xlo" else 5.0
        assert d.staged.abs().max().item() <= d.x_bound
        d.x_scale = R.pow2_operand_scale(d.x_bound, 14)
    else:
        d.x_scale = R.pow2_operand_scale(d.staged.abs().max().item(), 14)
    if tag == "fwd":
        d.wt = d.w_eq
        d.bias = R.exact_ints((co,), 8, seed + 3)
        d.lin = d.conv(d.staged, d.w_eq.double())
        d.want = (d.lin + d.bias.double().view((1, -1) + (1,) * dims)).float()
    else:
        flip = tuple(range(2, 2 + dims))
        d.wt = d.w_eq.transpose(0, 1).flip(*flip).contiguous()          # the forward weight [channels of dy, channels of dx, k..]
        d.bias = None
        tconv = F.conv_transpose3d if dims == 3 else F.conv_transpose2d
        d.lin = tconv(d.staged, d.wt.double(), None, padding=k // 2)
        d.want = d.lin.float()
    return d


# ------------------------------------------------------------------------------------------------------------------ bwd-weight data (CPU)
@functools.lru_cache(maxsize=None)
def dw_data(k, shape, kind, dims=3, boxes=None):
    """(x, dy, float64 dW) of a bwd-weight case.  boxes: dy is zero outside one box per frame (the dy-box launches)."""
    n, ci, co = shape[:3]
    vol = tuple(shape[3:])
    assert len(vol) == dims and kind in ("xlo", "dylo")
    seed = _seed("dw", k, shape, kind, boxes)
    xs, ys = (n, ci) + vol, (n, co) + vol
    voxels = n
    for v in vol:
        voxels *= v
    d = types.SimpleNamespace(k=k, shape=shape, kind=kind, dims=dims, boxes=boxes)
    d.grad = (lambda a, b: WB.dw_ref(a, b, k)) if dims == 3 else B2.dw_ref
    if boxes is not None:
        inside = _box_mask(ys, boxes)
        voxels = int(inside.sum().item())
    if kind == "xlo":
        d.x, d.dy = _frac(xs, kind, seed, voxels), R.sparse_ints(ys, _density(kind, voxels), seed + 1, chunk=co)
    else:
        d.x, d.dy = R.sparse_ints(xs, _density(kind, voxels), seed, chunk=ci), _frac(ys, kind, seed + 1, voxels)
    if boxes is not None:
        d.dy = d.dy * inside.float()
        _put_top(d.dy, inside.expand_as(d.dy), 1 if kind == "xlo" else 4)
    d.lin = d.grad(d.x, d.dy)
    d.want = d.lin.float()
    return d


# ------------------------------------------------------------------------------------------------------------------ the case tables
FWD_KINDS, BWD_KINDS, DW_KINDS = ("xlo", "wlo"), ("dylo", "wlo"), ("xlo", "dylo")


def _wino(case):
    return case.kernel >= FB.LOCKSTEP


def _one_list(i, names):
    """one list per case, a different one from row to row so that every list name is run"""
    return names[i % len(names)]


FWD_PARAMS = [(c, k) for c in FB.FWD_CASES if not c.half for k in FWD_KINDS if not excluded("FWD_CASES", FB.case_id(c), k)]
K1_PARAMS = [(row, k) for row in FB.K1_CASES for k in FWD_KINDS if not excluded("K1_CASES", FB.case_id(row), k)]
K1_BWD_PARAMS = [(row, k) for row in FB.K1_CASES for k in BWD_KINDS if not excluded("K1_CASES-bwd", FB.case_id(row), k)]
# the fused affine: xlo everywhere, ReLU on every other row.  wlo where the normalised map of a ternary x (integers in [-5, 5], DENSE
# whatever x's density: the shift fills the zeros) leaves the sums room: Ci <= 48, with the ReLU, which zeroes half of the map
GNIN_PARAMS = [(c, "xlo", i % 2) for i, (c, _) in enumerate(FB.GNIN_CASES)] + [(c, "wlo", 1) for c, _ in FB.GNIN_CASES if c.shape[1] <= 48]
ROI_PARAMS = [(c, _one_list(i, names)) for i, (c, names) in enumerate(FB.ROI_CASES)]
BWD_PARAMS = [(c, k) for c in FB.BWD_CASES for k in BWD_KINDS if not excluded("BWD_CASES", FB.case_id(c), k)]
BWD_ROI_PARAMS = [(c, _one_list(i + j, names), k) for i, (c, names) in enumerate(FB.BWD_ROI_CASES) for j, k in enumerate(BWD_KINDS)]
DW3_PARAMS = [(row, k) for row in WB.INT_CASES for k in DW_KINDS if not excluded("INT_CASES-3d", WB.case_id(row), k)]
DW3_ROI_PARAMS = [((k3, shape, claimed), sorted(lists)[i % len(lists)], kind)
                  for i, (k3, shape, claimed, lists) in enumerate(WB.ROI_CASES) for kind in DW_KINDS]
DW2_PARAMS = [(row, k) for row in B2.INT_CASES for k in DW_KINDS if not excluded("INT_CASES-2d", B2.case_id(row), k)]
BD2_PARAMS = [(shape, k) for shape in B2.BWD_DATA_CASES for k in BWD_KINDS]


def fwd_id(c, k):
    return f"{FB.case_id(c)}-{k}"


def bwd_shape2d(shape):
    """the bwd-data launch's own (N, channels of dy, channels of dx, H, W) of a 2-D conv Ci -> Co"""
    n, ci, co, h, w = shape
    return (n, co, ci, h, w)


def roi_data_boxes(case, name):
    """(boxes, roi_frames, tile) of a named list of tests/test_gpu_conv_f16x3_branches.py for this case's tile"""
    tile = {FB.D2: (2, 8, 8)}.get(case.kernel, (4, 8, 8))
    boxes, frames = FB.roi_boxes(name, case.shape, tile)
    return tuple(tuple(b) for b in boxes), frames, tile


def all_cases():
    """(table, id, kind, data thunk) of every case this file runs: what tests/test_f16x3_lo_planes_host.py walks"""
    out = []
    for c, k in FWD_PARAMS:
        out.append(("FWD_CASES", FB.case_id(c), k, functools.partial(conv_data, "fwd", 3, c.shape, k, _wino(c))))
    for (shape, claim), k in K1_PARAMS:
        out.append(("K1_CASES", FB.case_id((shape, claim)), k, functools.partial(conv_data, "fwd", 1, shape, k, False)))
    for (shape, claim), k in K1_BWD_PARAMS:
        out.append(("K1_CASES-bwd", FB.case_id((shape, claim)), k, functools.partial(conv_data, "bwd", 1, shape, k, False)))
    for c, k, relu in GNIN_PARAMS:
        out.append(("GNIN_CASES", FB.case_id(c), k, functools.partial(conv_data, "fwd", 3, c.shape, k, _wino(c), 3, relu)))
    for c, name in ROI_PARAMS:
        out.append(("ROI_CASES", f"{FB.case_id(c)}-{name}", "xlo", functools.partial(conv_data, "fwd", 3, c.shape, "xlo", _wino(c))))
    for c, k in BWD_PARAMS:
        out.append(("BWD_CASES", FB.case_id(c), k, functools.partial(conv_data, "bwd", 3, c.shape, k, _wino(c))))
    for c, name, k in BWD_ROI_PARAMS:
        boxes, frames, _ = roi_data_boxes(c, name)
        out.append(("BWD_ROI_CASES", f"{FB.case_id(c)}-{name}", k, functools.partial(conv_data, "bwd", 3, c.shape, k, _wino(c), 3, None, boxes)))
    for row, k in DW3_PARAMS:
        out.append(("INT_CASES-3d", WB.case_id(row), k, functools.partial(dw_data, row[0], row[1], k)))
    for row, name, k in DW3_ROI_PARAMS:
        boxes = tuple(dict((s, l) for _, s, _, l in WB.ROI_CASES)[row[1]][name])
        out.append(("ROI_CASES-3d-dw", f"{WB.case_id(row)}-{name}", k, functools.partial(dw_data, row[0], row[1], k, 3, boxes)))
    for row, k in DW2_PARAMS:
        out.append(("INT_CASES-2d", B2.case_id(row), k, functools.partial(dw_data, 3, row[0], k, 2)))
    for shape, k in BD2_PARAMS:
        out.append(("BWD_DATA_CASES-2d", "x".join(map(str, shape)), k, functools.partial(conv_data, "bwd", 3, bwd_shape2d(shape), k, False, 2)))
    return out


# ------------------------------------------------------------------------------------------------------------------ fixtures, helpers
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


def _equal(got, want, what):
    got = got.cpu()
    bad = got != want
    assert got.shape == want.shape and torch.equal(got, want), (what, int(bad.sum()), bad.numel(),
                                                                 (got.double() - want.double()).abs().max().item())


def _grad_scale(ops, dyd, dy):
    """dy's operand scale, taken from ops.grad_prep, is the power of two the reference splits at"""
    _, scale = ops.grad_prep(dyd, want_bias=False)
    s = R.pow2_operand_scale(dy.abs().max().item(), 14)
    assert scale.cpu().tolist()[:3] == [s, 1.0 / s, dy.abs().max().item()]
    return scale


# ------------------------------------------------------------------------------------------------------------------ 3-D forward
@pytest.mark.parametrize("case,kind", FWD_PARAMS, ids=[fwd_id(c, k) for c, k in FWD_PARAMS])
def test_forward_lo_planes_are_exact(ops, lib, dev, monkeypatch, case, kind):
    FB.set_switches(monkeypatch, case.env)
    FB.claim_holds(lib, case)
    d = conv_data("fwd", 3, case.shape, kind, _wino(case))
    ops.f16x3_saturation_count(reset=True)
    y = ops.conv3d(d.x.to(dev), ops.PackedConv(d.wt.to(dev), d.bias.to(dev)), precision=1)
    _equal(y, d.want, fwd_id(case, kind))
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("row,kind", K1_PARAMS, ids=[fwd_id(r, k) for r, k in K1_PARAMS])
def test_forward_1x1x1_lo_planes_are_exact(ops, lib, dev, monkeypatch, row, kind):
    FB.set_switches(monkeypatch, {})
    FB.k1_claim_holds(lib, row)
    d = conv_data("fwd", 1, row[0], kind, False)
    ops.f16x3_saturation_count(reset=True)
    y = ops.conv3d(d.x.to(dev), ops.PackedConv(d.wt.to(dev), d.bias.to(dev)), precision=1)
    _equal(y, d.want, fwd_id(row, kind))
    assert ops.f16x3_saturation_count() == 0


GNIN_IDS = [f"{FB.case_id(c)}-{k}-relu{r}" for c, k, r in GNIN_PARAMS]


@pytest.mark.parametrize("case,kind,relu", GNIN_PARAMS, ids=GNIN_IDS)
def test_fused_input_affine_lo_planes_are_exact(ops, lib, dev, monkeypatch, case, kind, relu):
    """conv(pad0(relu?(x * scale + shift))): the lo plane is that of the NORMALISED x, at the scale of the descriptor's bound"""
    FB.set_switches(monkeypatch, case.env)
    plan = FB.claim_holds(lib, case)
    assert case.shape[1] <= plan[6]
    d = conv_data("fwd", 3, case.shape, kind, _wino(case), 3, relu)
    rng = torch.zeros(4100, dtype=torch.float32)
    rng[2] = d.x_bound
    pc = ops.PackedConv(d.wt.to(dev), d.bias.to(dev))
    ops.f16x3_saturation_count(reset=True)
    y, _ = FB._gnin_launch(lib, d.x.to(dev), d.table.to(dev), rng.to(dev), relu, pc, case.shape)
    _equal(y, d.want, f"{fwd_id(case, kind)} in_relu {relu}")
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("case,name", ROI_PARAMS, ids=[f"{FB.case_id(c)}-{nm}-xlo" for c, nm in ROI_PARAMS])
def test_demand_driven_lo_planes_are_exact_in_the_listed_tiles_and_nothing_else_is_written(ops, lib, dev, monkeypatch, case, name):
    FB.set_switches(monkeypatch, case.env)
    plan = FB.claim_holds(lib, case, roi=True)
    assert plan[5] == 1
    n, ci, co, dd, h, w = case.shape
    boxes, frames, tile = roi_data_boxes(case, name)
    assert tile == plan[1:4]
    need = FB.listed_voxels(case.shape, tile, boxes, frames)
    assert bool(need.any())
    d = conv_data("fwd", 3, case.shape, "xlo", _wino(case))
    xd = d.x.to(dev)
    pc = ops.PackedConv(d.wt.to(dev), d.bias.to(dev))
    y = torch.full((n, co, dd, h, w), float("nan"), dtype=torch.float32, device=dev)
    ws_bytes = lib.mphip_conv3d_roi_workspace_bytes(n, ci, co, dd, h, w, 3, 1)
    ws = torch.empty((ws_bytes + 7) // 8 + 1, dtype=torch.float64, device=dev)
    ops.f16x3_saturation_count(reset=True)
    FB._check(lib.mphip_conv3d_fwd_roi(FB.P(xd), FB.P(ops.absmax_range(xd)), FB.P(pc.packed(1)), FB.P(pc.bias), FB.P(y),
                                       FB.P(FB._roi_tensor(boxes, dev)), frames, n, ci, co, dd, h, w, 3, 1, FB.P(ws), ws_bytes, FB._stream()),
              "mphip_conv3d_fwd_roi")
    y = y.cpu()
    mask = need[:, None].expand_as(y)
    assert torch.equal(y[mask], d.want[mask]), "listed tiles"
    if case.splits == 1:
        assert bool(torch.isnan(y[~mask]).all()), "an unsplit launch wrote outside the listed tiles"
    assert ops.f16x3_saturation_count() == 0


# ------------------------------------------------------------------------------------------------------------------ 3-D bwd-data
def _bwd_launch(ops, d, dev, roi=None):
    dyd = d.x.to(dev)
    scale = _grad_scale(ops, dyd, d.x)
    return ops.conv3d_bwd_data(dyd, ops.PackedConv(d.wt.to(dev), None, transposed=True), scale, precision=1, roi=roi)


@pytest.mark.parametrize("case,kind", BWD_PARAMS, ids=[fwd_id(c, k) for c, k in BWD_PARAMS])
def test_bwd_data_lo_planes_are_exact(ops, lib, dev, monkeypatch, case, kind):
    FB.set_switches(monkeypatch, case.env)
    FB.claim_holds(lib, case)
    d = conv_data("bwd", 3, case.shape, kind, _wino(case))
    ops.f16x3_saturation_count(reset=True)
    _equal(_bwd_launch(ops, d, dev), d.want, fwd_id(case, kind))
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("row,kind", K1_BWD_PARAMS, ids=[fwd_id(r, k) for r, k in K1_BWD_PARAMS])
def test_bwd_data_1x1x1_lo_planes_are_exact(ops, lib, dev, monkeypatch, row, kind):
    FB.set_switches(monkeypatch, {})
    FB.k1_claim_holds(lib, row)
    d = conv_data("bwd", 1, row[0], kind, False)
    ops.f16x3_saturation_count(reset=True)
    _equal(_bwd_launch(ops, d, dev), d.want, fwd_id(row, kind))
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("case,name,kind", BWD_ROI_PARAMS, ids=[f"{FB.case_id(c)}-{nm}-{k}" for c, nm, k in BWD_ROI_PARAMS])
def test_bwd_data_roi_lo_planes_are_exact_inside_and_zero_outside(ops, lib, dev, monkeypatch, case, name, kind):
    FB.set_switches(monkeypatch, case.env)
    plan = FB.claim_holds(lib, case, roi=True)
    boxes, frames, tile = roi_data_boxes(case, name)
    assert frames == 0 and tile == plan[1:4]
    d = conv_data("bwd", 3, case.shape, kind, _wino(case), 3, None, boxes)
    inside = FB.listed_voxels(case.shape, tile, boxes, 0, dilate=1)[:, None].expand_as(d.lin)
    assert not bool(d.lin[~inside].any())
    ops.f16x3_saturation_count(reset=True)
    dx = _bwd_launch(ops, d, dev, roi=FB._roi_tensor(boxes, dev)).cpu()
    assert torch.equal(dx[inside], d.want[inside]), "inside the listed tiles"
    assert not bool(dx[~inside].any()), "dx is not 0 outside the listed tiles"
    assert ops.f16x3_saturation_count() == 0


# ------------------------------------------------------------------------------------------------------------------ 3-D bwd-weight
@pytest.mark.parametrize("row,kind", DW3_PARAMS, ids=[f"{WB.case_id(r)}-{k}" for r, k in DW3_PARAMS])
def test_bwd_weight_lo_planes_are_exact(ops, lib, dev, row, kind):
    k, shape, claimed, edges = row
    WB.claim_holds(lib, row)
    d = dw_data(k, shape, kind)
    xd, dyd = d.x.to(dev), d.dy.to(dev)
    scale = _grad_scale(ops, dyd, d.dy)
    ops.f16x3_saturation_count(reset=True)
    _equal(ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1), d.want, f"{WB.case_id(row)}-{kind}")
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("row,name,kind", DW3_ROI_PARAMS, ids=[f"{WB.case_id(r)}-{nm}-{k}" for r, nm, k in DW3_ROI_PARAMS])
def test_bwd_weight_dy_box_lo_planes_are_exact(ops, lib, dev, row, name, kind):
    k, shape, claimed = row
    WB.claim_holds(lib, row)
    boxes = tuple(dict((s, l) for _, s, _, l in WB.ROI_CASES)[shape][name])
    d = dw_data(k, shape, kind, 3, boxes)
    xd, dyd = d.x.to(dev), d.dy.to(dev)
    roi = torch.tensor([list(b) + [0, 0] for b in boxes], dtype=torch.int32).to(dev)
    scale = _grad_scale(ops, dyd, d.dy)
    ops.f16x3_saturation_count(reset=True)
    _equal(ops.conv3d_bwd_weight(xd, dyd, k, scale, precision=1, roi=roi), d.want, f"{WB.case_id(row)}-{name}-{kind}")
    assert ops.f16x3_saturation_count() == 0


# ------------------------------------------------------------------------------------------------------------------ 2-D backward
@pytest.mark.parametrize("row,kind", DW2_PARAMS, ids=[f"{B2.case_id(r)}-{k}" for r, k in DW2_PARAMS])
def test_conv2d_bwd_weight_lo_planes_are_exact(ops, lib, dev, row, kind):
    shape, claimed, edges = row
    B2.claim_holds(lib, row)
    d = dw_data(3, shape, kind, 2)
    xd, dyd = d.x.to(dev), d.dy.to(dev)
    scale = _grad_scale(ops, dyd, d.dy)
    ops.f16x3_saturation_count(reset=True)
    _equal(ops.conv2d_bwd_weight(xd, dyd, scale), d.want, f"{B2.case_id(row)}-{kind}")
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("shape,kind", BD2_PARAMS, ids=[f"{'x'.join(map(str, s))}-{k}" for s, k in BD2_PARAMS])
def test_conv2d_bwd_data_takes_the_grad_prep_scale_with_lo_planes(ops, dev, shape, kind):
    """the transposed pack's bits are tied to the forward pack by tests/test_gpu_conv2d_bwd.py: this checks the grad_prep scale path"""
    n, ci, co, h, w = shape
    assert ops.conv2d_bwd_supported(n, ci, co, h, w, True)
    d = conv_data("bwd", 3, bwd_shape2d(shape), kind, False, 2)
    dyd = d.x.to(dev)
    scale = _grad_scale(ops, dyd, d.x)
    ops.f16x3_saturation_count(reset=True)
    dx = ops.conv2d_bwd_data(dyd, ops.PackedConv2d(d.wt.to(dev), None, transposed=True), scale)
    _equal(dx, d.want, f"{shape}-{kind}")
    assert ops.f16x3_saturation_count() == 0
