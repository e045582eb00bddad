"""Every 2-D matrix-core ("f16x3") conv form, exactly, on data whose `lo` halves are NOT zero, and at power-of-two magnitudes: the plain,
two-source, stride-2, grouped, split-K and pointwise forms of ops._CONV2D_FORMS, the 7x7 stem, the typed one-product entry and the two
up2 forms (csrc/conv2d_f16x3_tile.h and its instantiating units, conv2d_s2_f16x3.hip, conv2d_pw_f16x3.hip, conv2d_splitk_f16x3.hip,
conv2d_stem7_f16x3.hip).

The oracle is the float64 CPU conv of the form (`_linear`: stride, padding, groups, the staged two-source map), then bias, residual, ReLU
and max-pool in float64; the launch must be torch.equal to it, cast ONCE to the output dtype.  There is no tolerance in this file, and
ops.f16x3_saturation_count() must be 0 after each case.

a. lo planes.  Small-integer data makes every lo half of the f16 split zero, so the files that test each form on integers never see the
Wlo*Xhi and Whi*Xlo products, which are half of what these kernels stage, pack and read.  Two data kinds (oracle.hotpath_ref
lo_plane_pair) give ONE operand fractional bits that only hi + lo can hold, and keep every partial sum exact in fp32:
  xlo  x = a + b*2^-11, a integers in [-4, 4] containing a 4, b in [-1023, 1023]; w integers in [-Wm, Wm].  max|x| is in [4, 4.5), the x
       scale is 2^11, x*2^11 is an integer below 2^14 of up to 14 bits: hi + lo is exact, lo != 0 for about half of the elements, w has
       lo = 0, and Wlo*Xhi + Whi*Xhi + Whi*Xlo = w*x exactly.  All products are multiples of one unit (2^-11 of the unscaled result) and
       every partial sum, in any order, is bounded by sum |w| (|xhi| + |xlo|) <= taps * Ci * Wm * 2^14 units < 2^24.
  wlo  w = a + b*2^-12, b in [-2047, 2047]; x integers in [-Xm, Xm].  The w scale is 2^12, w*2^12 an integer below 2^15;
       taps * Ci * Xm * 2^15 < 2^24.
`top` of a case is its Wm / Xm.  Bias and residual are integers in [-8, 8].  Two-source cases with affine tables (integer scale in
{1, 2}, shift in [-3, 3], ReLU on the first source) bring a descriptor that bounds the normalised map (12 for xlo, 5 for wlo with
Xm = 1); the kernel takes the smaller of the two sources' scales for both, which for xlo is 2^10: staged values are multiples of 1/2 below
2^14, still exact as hi + lo.  tests/test_conv2d_exact_data_host.py asserts all of this per case on the CPU (from the case's own data,
not from the formula), and that a one-product or half-swapped emulation is wrong on more than 90 % of the outputs, so each case can fail.
The typed one-product entry (products = 1) multiplies Whi*Xhi alone: its truth is the float64 conv of the operands rounded once to f16 at
their scales (round_f16_at_scale); a half x is built from the values rounded to that dtype.
The up2 / resup2 forms blend with fractional weights and have no exact float64 answer: they must give the bits of ops.conv2d on the
materialised map (model.up2_reference), as in tests/test_gpu_conv2d_up2.py, on both data kinds.

Shapes: 19x35 is 2x3 tiles of 16x16 with ragged last tiles (stride 2: 10x18 outputs, 2x2 tiles of 8x16; pointwise: 665 and 342 pixels on
256-pixel tiles), Ci >= 32 gives at least two K chunks, Co = 96 leaves the second 64-channel tile one 32-row half, N = 2.  The grouped form
runs the shape with one chunk per group (Ci 32, groups 2) and one with two; the split-K cases take Ci / groups = 64 (four chunks) so that
`splits` can be the chunk count and a proper divisor of it (4 and 2); 19x35 takes the finish kernel's scalar body, 20x36 (H * W % 4 == 0) its
16-byte one.

b. magnitudes.  x = integers * 2^p, w = integers * 2^q, p in (-100, -30, 30, 100), q in (-30, 30), zero bias: the result is the integer
conv times 2^(p+q) rounded once to fp32 (Inf where it overflows).  The kernels multiplied their accumulators by ONE float,
1/scale_w * 1/scale_x; at (p, q) = (-100, -30) that is 2^-42 * 2^-111 = 2^-153 = 0.0f and every output equalled its bias.  The two factors
are applied one after the other now (Unscale / unscaled(), csrc/mphip_f16x3.h), bit-identical wherever the single product was
representable.  The 7x7 stem always did so: it is the control.  The up2 forms are compared with ops.conv2d on the materialised map, and
must not be all zero.

Measured on an MI355X: DESIGN.md 3.1c-quinquies."""
import collections
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EXACT = 2 ** 24
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
KINDS = ("xlo", "wlo")
X_EXPONENTS, W_EXPONENTS = (-100, -30, 30, 100), (-30, 30)

# form: plain cat s2 grouped split pw stem7 typed up2 resup2.  shape = (N, Ci, Co, H, W) of the INPUT map (cat: Ci = C1 + C2, C1 = 16).
# top = (Wm for xlo, Xm for wlo).  opt: the form's own switches.
Case = collections.namedtuple("Case", "form shape top opt edges")


def C(form, shape, top, edges, **opt):
    return Case(form, tuple(shape), tuple(top), tuple(sorted(opt.items())), edges)


BASE = (2, 32, 96, 19, 35)
LO_CASES = (
    [C("plain", BASE, (3, 1), "tiles2x3-ragged-chunks2-cohalf", res=res, relu=relu) for res in (False, True) for relu in (False, True)]
    + [C("cat", (2, 48, 96, 19, 35), (1, 1), "c16+32-tiles2x3-ragged-chunks3-cohalf", tables=t, res=True, relu=True)
       for t in ("none", "first", "both")]
    + [C("s2", BASE, (3, 1), "oddHW-tiles2x2-ragged-chunks2-cohalf", res=False, relu=False),
       C("s2", BASE, (3, 1), "oddHW-tiles2x2-ragged-chunks2-cohalf", res=True, relu=True),
       C("grouped", (2, 32, 128, 19, 35), (3, 1), "g2-chunk1-tiles2x3-ragged", groups=2, res=True, relu=True),
       C("grouped", (2, 64, 128, 19, 35), (3, 1), "g2-chunks2-tiles2x3-ragged", groups=2, res=False, relu=False)]
    + [C("split", (2, 64, 96, 19, 35), (1, 1), "chunks4-tiles2x3-ragged-cohalf", groups=1, splits=s, res=True, relu=True) for s in (4, 2)]
    + [C("split", (2, 128, 128, 19, 35), (1, 1), "g2-chunks4-tiles2x3-ragged", groups=2, splits=s, res=True, relu=True) for s in (4, 2)]
    + [C("split", (2, 64, 96, 20, 36), (1, 1), "chunks4-tiles2x3-ragged-cohalf-vecfinish", groups=1, splits=2, res=True, relu=True)]
    + [C("pw", BASE, (4, 4), "pix665-tiles3-ragged-chunks2-cohalf", stride=1, res=True, relu=True),
       C("pw", (2, 32, 96, 35, 37), (4, 4), "oddHW-pix342-tiles2-ragged-chunks2-cohalf", stride=2, res=True, relu=True),
       C("stem7", (2, 3, 48, 19, 35), (4, 3), "tiles2x3-ragged-co48", stride=1, relu=False, pool=False),
       C("stem7", (2, 3, 48, 19, 35), (4, 3), "oddHW-ragged-pool-co48", stride=2, relu=True, pool=True)]
    + [C("typed", BASE, (3, 1), "p1-tiles2x3-ragged-chunks2-cohalf", xdt=xdt, ydt=ydt, res=True, relu=True)
       for xdt, ydt in ((F32, F32), (F16, F32), (BF16, F32), (F32, F16), (F32, BF16))]
)
UP2_CASES = [C("up2", (2, 32, 96, 10, 18), (3, 1), "low10x18-tiles2x3-ragged-chunks2-cohalf", res=True, relu=True),
             C("resup2", (2, 32, 96, 20, 36), (3, 1), "tiles2x3-ragged-chunks2-cohalf", relu=True)]

MAG_SHAPE = (1, 16, 32, 17, 19)       # 2x2 tiles of 16x16 (stride 2: 2x1 of 8x16; pointwise: 323 and 306 pixels)
MAG_CASES = [
    C("plain", MAG_SHAPE, (4, 4), "tiles2x2", res=False, relu=False),
    C("cat", (1, 32, 32, 17, 19), (4, 4), "c16+16-tiles2x2", tables="none", res=False, relu=False),
    C("grouped", (1, 32, 128, 17, 19), (4, 4), "g2-tiles2x2", groups=2, res=False, relu=False),
    C("typed", MAG_SHAPE, (4, 4), "p1-tiles2x2", xdt=F32, ydt=F32, res=False, relu=False),
    C("typed", MAG_SHAPE, (4, 4), "p1-tiles2x2", xdt=BF16, ydt=F32, res=False, relu=False),
    C("s2", MAG_SHAPE, (4, 4), "tiles2x1", res=False, relu=False),
    C("pw", MAG_SHAPE, (4, 4), "pix323-tiles2", stride=1, res=False, relu=False),
    C("pw", (1, 16, 32, 33, 35), (4, 4), "pix306-tiles2", stride=2, res=False, relu=False),
    C("split", (1, 32, 32, 17, 19), (4, 4), "chunks2-tiles2x2-scalarfinish", groups=1, splits=2, res=False, relu=False),
    C("split", (1, 32, 32, 18, 20), (4, 4), "chunks2-tiles2x2-vecfinish", groups=1, splits=2, res=False, relu=False),
    C("stem7", (1, 3, 16, 17, 19), (4, 4), "control-tiles2x2", stride=1, relu=False, pool=False),
]
MAG_UP2_CASES = [C("up2", (1, 16, 32, 9, 10), (4, 4), "low9x10-tiles2x2", res=False, relu=False),
                 C("resup2", (1, 16, 32, 18, 20), (4, 4), "tiles2x2", relu=False)]


def case_id(case):
    n, ci, co, h, w = case.shape
    opt = "".join(f"-{k}{NAME.get(v, v) if not isinstance(v, bool) else int(v)}" for k, v in case.opt)
    return f"{case.form}-{n}x{ci}x{co}@{h}x{w}-{case.edges}{opt}"


# ------------------------------------------------------------------------------------------------------------------ the oracle (CPU)
def _linear(case):
    """The form's bilinear map (x64 staged, w64) -> y64 without bias."""
    o = dict(case.opt)
    if case.form in ("plain", "cat", "typed", "up2", "resup2"):
        return lambda x, w: F.conv2d(x, w, None, padding=1)
    if case.form == "s2":
        return lambda x, w: F.conv2d(x, w, None, stride=2, padding=1)
    if case.form in ("grouped", "split"):
        return lambda x, w: F.conv2d(x, w, None, padding=1, groups=o["groups"])
    if case.form == "pw":
        return lambda x, w: F.conv2d(x, w, None, stride=o["stride"])
    assert case.form == "stem7", case.form
    return lambda x, w: F.conv2d(x, w, None, stride=o["stride"], padding=3)


def _w_shape(case):
    n, ci, co, h, w = case.shape
    o = dict(case.opt)
    k = {"pw": 1, "stem7": 7}.get(case.form, 3)
    return (co, ci // o.get("groups", 1), k, k)


def _epilogue(case, lin, b, res):
    o = dict(case.opt)
    y = lin + b.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    if o.get("relu"):
        y = F.relu(y)
    return F.max_pool2d(y, 3, 2, 1) if o.get("pool") else y


def _tables(n, c, seed):
    return torch.stack([torch.randint(1, 3, (n, c), generator=torch.Generator().manual_seed(seed)).float(),
                        torch.randint(-3, 4, (n, c), generator=torch.Generator().manual_seed(seed + 1)).float()], dim=-1).contiguous()


@functools.lru_cache(maxsize=None)
def lo_data(case, kind):
    """Everything a lo-plane case needs, made once on the CPU and never changed: the operands, the staged map the conv multiplies (float64),
    the operand scale of x the kernel will take, and the float64 answer."""
    n, ci, co, h, w = case.shape
    o = dict(case.opt)
    seed = 1000 + 10 * (LO_CASES + UP2_CASES).index(case)
    top = case.top[KINDS.index(kind)]
    d = types.SimpleNamespace(case=case, kind=kind, top=top, conv=_linear(case), x_bound=None)
    d.x, d.w = R.lo_plane_pair(kind, (n, ci, h, w), _w_shape(case), top, seed)
    d.b = R.exact_ints((co,), 8, seed + 2)
    d.staged = d.x.double()
    if case.form == "cat":
        d.x1, d.x2 = d.x[:, :16].contiguous(), d.x[:, 16:].contiguous()
        if kind == "xlo":
            d.x2.view(-1)[0] = 4.0                                  # each scanned source holds its own maximum in [4, 4.5)
        d.use1, d.use2 = o["tables"] in ("first", "both"), o["tables"] == "both"
        d.t1, d.t2 = _tables(n, 16, seed + 5), _tables(n, ci - 16, seed + 7)
        s1, s2 = d.x1.double(), d.x2.double()
        if d.use1:
            s1 = F.relu(s1 * d.t1[..., 0, None, None].double() + d.t1[..., 1, None, None].double())
        if d.use2:
            s2 = s2 * d.t2[..., 0, None, None].double() + d.t2[..., 1, None, None].double()      # (no ReLU on the second source)
        d.x, d.staged = torch.cat([d.x1, d.x2], 1), torch.cat([s1, s2], 1)
        d.x_bound = (4.5 * 2 + 3) if kind == "xlo" else float(top * 2 + 3)                       # of a source with a table
        assert not d.use1 or s1.abs().max() <= d.x_bound
        assert not d.use2 or s2.abs().max() <= d.x_bound
        scales = [R.pow2_operand_scale(d.x_bound if use else s.abs().max().item(), 14) for s, use in ((s1, d.use1), (s2, d.use2))]
        d.x_scale = min(scales)                                     # one accumulator, one operand scale: the smaller one
    elif case.form == "typed" and o["xdt"] != F32:
        d.staged = d.x.to(o["xdt"]).double()                        # a half x holds the values rounded to its dtype
        d.x_scale = R.pow2_operand_scale(d.staged.abs().max().item(), 14)
    else:
        d.x_scale = R.pow2_operand_scale(d.staged.abs().max().item(), 14)
    if case.form == "typed":                                        # one product: the operands rounded once to f16 at their scales
        xh, _, _ = R.split_f16_at_scale(d.staged, 14, d.x_scale)
        d.lin = d.conv(xh, R.round_f16_at_scale(d.w, top=15))
    else:
        d.lin = d.conv(d.staged, d.w.double())
    d.res = R.exact_ints(tuple(d.lin.shape), 8, seed + 3) if o.get("res") else None
    if o.get("pool"):
        assert d.res is None
    d.want64 = _epilogue(case, d.lin, d.b, d.res)
    return d


@functools.lru_cache(maxsize=None)
def mag_data(case):
    """Integer operands in [-4, 4] (both scales fixed by a 4) and their float64 conv; the magnitude tests multiply by 2^p and 2^q."""
    n, ci, co, h, w = case.shape
    seed = 5000 + 10 * (MAG_CASES + MAG_UP2_CASES).index(case)
    d = types.SimpleNamespace(case=case, conv=_linear(case))
    d.x, d.w = R.exact_ints((n, ci, h, w), 4, seed), R.exact_ints(_w_shape(case), 4, seed + 1)
    if case.form == "cat":
        d.x[0, 16, 0, 0] = 4.0                                      # each scanned source holds its own maximum
    d.truth = d.conv(d.x.double(), d.w.double())
    assert d.truth.abs().max() < EXACT
    return d


def mag_operands(d, p, q):
    xs, ws = (d.x.double() * 2.0 ** p).float(), (d.w.double() * 2.0 ** q).float()
    assert torch.equal(xs.double(), d.x.double() * 2.0 ** p) and torch.equal(ws.double(), d.w.double() * 2.0 ** q)
    return xs, ws, (d.truth * 2.0 ** (p + q)).float()              # float64 holds truth * 2^(p+q) exactly; one rounding to fp32


# ------------------------------------------------------------------------------------------------------------------ the launches
def _launch(ops, case, x, w, b, res, staged_bound=None, tables=None):
    """One launch of the case's form on the GPU from CPU operands -> y on the GPU."""
    o = dict(case.opt)
    g = lambda t: None if t is None else t.to(DEV)
    relu = bool(o.get("relu"))
    if case.form == "stem7":
        return ops.conv2d_stem7(g(x), ops.PackedConv2dStem7(g(w), g(b)), stride=o["stride"], relu=relu, pool=o["pool"])
    pack = ops.PackedConv2d(g(w), g(b), o.get("groups", 1))
    if case.form == "plain":
        return ops.conv2d(g(x), pack, residual=g(res), relu=relu)
    if case.form == "typed":
        r = None if res is None else g(res).to(o["ydt"])
        return ops.conv2d(g(x).to(o["xdt"]), pack, residual=r, relu=relu, out_dtype=o["ydt"], products=1)
    if case.form == "s2":
        return ops.conv2d_s2(g(x), pack, residual=g(res), relu=relu)
    if case.form == "grouped":
        return ops.conv2d_grouped(g(x), pack, residual=g(res), relu=relu)
    if case.form == "split":
        n, ci, co, h, wd = case.shape
        assert ops.conv2d_split_supported(n, ci, co, h, wd, o["groups"], o["splits"]) and ci // o["groups"] // 16 % o["splits"] == 0
        f = ops.conv2d_grouped if o["groups"] > 1 else ops.conv2d
        return f(g(x), pack, residual=g(res), relu=relu, splits=o["splits"])
    if case.form == "pw":
        return ops.conv2d_pw(g(x), pack, residual=g(res), relu=relu, stride=o["stride"])
    assert case.form == "cat", case.form
    use1, use2, t1, t2 = tables or (False, False, None, None)
    bound = lambda: ops.absmax_range(torch.full((4,), float(staged_bound), device=DEV))   # a descriptor that bounds a normalised source
    return ops.conv2d_cat(g(x[:, :16].contiguous()), pack, x2=g(x[:, 16:].contiguous()), affine1=g(t1) if use1 else None, relu1=use1,
                          x1_range=bound() if use1 else None, affine2=g(t2) if use2 else None, x2_range=bound() if use2 else None,
                          residual=g(res), relu=relu)


@pytest.fixture(scope="module")
def ops():
    from megaportrait_hack_amd import _lib, ops

    _lib.load()
    return ops


LO_PARAMS = [(c, k) for c in LO_CASES for k in KINDS]


@pytest.mark.parametrize("case,kind", LO_PARAMS, ids=[f"{case_id(c)}-{k}" for c, k in LO_PARAMS])
def test_lo_planes_are_exact(ops, case, kind):
    d = lo_data(case, kind)
    o = dict(case.opt)
    ydt = o.get("ydt", F32)
    want = d.want64.to(ydt)                                         # the one rounding of a typed y; fp32: exact (the host test)
    ops.f16x3_saturation_count(reset=True)
    got = _launch(ops, case, d.x, d.w, d.b, d.res, d.x_bound, (d.use1, d.use2, d.t1, d.t2) if case.form == "cat" else None)
    assert got.dtype == ydt and got.shape == want.shape
    bad = (got.cpu() != want)
    assert torch.equal(got.cpu(), want), (case_id(case), kind, int(bad.sum()), bad.numel(),
                                          (got.cpu().double() - want.double()).abs().max().item())
    assert ops.f16x3_saturation_count() == 0


UP2_PARAMS = [(c, k) for c in UP2_CASES for k in KINDS]


@pytest.mark.parametrize("case,kind", UP2_PARAMS, ids=[f"{case_id(c)}-{k}" for c, k in UP2_PARAMS])
def test_up2_forms_carry_the_lo_planes_of_the_materialised_map(ops, case, kind):
    from megaportrait_hack_amd import model as M

    d = lo_data(case, kind)
    o = dict(case.opt)
    n, ci, co, h, w = case.shape
    x = d.x.to(DEV)
    pack = ops.PackedConv2d(d.w.to(DEV), d.b.to(DEV))
    r = ops.absmax_range(x.clone())
    ops.f16x3_saturation_count(reset=True)
    if case.form == "up2":
        res = R.exact_ints((n, co, 2 * h, 2 * w), 8, 77).to(DEV)
        got = ops.conv2d_up2(x, pack, residual=res, relu=o["relu"], x_range=r)
        want = ops.conv2d(M.up2_reference(x), pack, residual=res, relu=o["relu"], x_range=r)
    else:
        low = R.lo_plane_operand((n, co, h // 2, w // 2), 11, 78).to(DEV)
        got = ops.conv2d_resup2(x, pack, low, relu=o["relu"], x_range=r)
        want = ops.conv2d(x, pack, residual=M.up2_reference(low), relu=o["relu"], x_range=r)
        # ... and the conv under the blended residual is the exact one
        plain = ops.conv2d(x, pack, x_range=r)
        assert torch.equal(plain.cpu(), _epilogue(C("plain", case.shape, case.top, ""), d.lin, d.b, None).float())
    assert got.shape == want.shape and torch.equal(got, want), (case_id(case), kind, (got - want).abs().max().item())
    assert ops.f16x3_saturation_count() == 0


MAG_PARAMS = [(c, p, q) for c in MAG_CASES for p in X_EXPONENTS for q in W_EXPONENTS]


@pytest.mark.parametrize("case,p,q", MAG_PARAMS, ids=[f"{case_id(c)}-x2^{p}-w2^{q}" for c, p, q in MAG_PARAMS])
def test_power_of_two_magnitudes_are_exact(ops, case, p, q):
    """x = integers * 2^p, w = integers * 2^q, zero bias: the integer conv times 2^(p+q) rounded once to fp32 (Inf at 2^130, subnormals and
    small normals at 2^-130), bit for bit.  At (p, q) = (-100, -30) the single unscale factor 2^-153 was 0 in every kernel but the stem's."""
    d = mag_data(case)
    xs, ws, want = mag_operands(d, p, q)
    if abs(p + q) < 120:
        assert torch.equal(want.double(), d.truth * 2.0 ** (p + q)) and bool(torch.isfinite(want).all())
    ops.f16x3_saturation_count(reset=True)
    got = _launch(ops, case, xs, ws, torch.zeros(case.shape[2]), None)
    bad = (got.cpu() != want)
    assert torch.equal(got.cpu(), want), (case_id(case), p, q, int(bad.sum()), bad.numel(), got.abs().max().item(), want.abs().max().item())
    assert ops.f16x3_saturation_count() == 0


MAG_UP2_PARAMS = [(c, p, q) for c in MAG_UP2_CASES for p in X_EXPONENTS for q in W_EXPONENTS]


@pytest.mark.parametrize("case,p,q", MAG_UP2_PARAMS, ids=[f"{case_id(c)}-x2^{p}-w2^{q}" for c, p, q in MAG_UP2_PARAMS])
def test_up2_forms_follow_the_materialised_map_at_every_magnitude(ops, case, p, q):
    from megaportrait_hack_amd import model as M

    d = mag_data(case)
    n, ci, co, h, w = case.shape
    xs, ws, _ = mag_operands(d, p, q)
    x = xs.to(DEV)
    pack = ops.PackedConv2d(ws.to(DEV), torch.zeros(co, device=DEV))
    r = ops.absmax_range(x.clone())
    ops.f16x3_saturation_count(reset=True)
    if case.form == "up2":
        got = ops.conv2d_up2(x, pack, x_range=r)
        want = ops.conv2d(M.up2_reference(x), pack, x_range=r)
    else:
        e = max(-100, min(100, p + q))                               # (a finite residual: the blend of an Inf is a NaN)
        low = (R.exact_ints((n, co, h // 2, w // 2), 4, 79).double() * 2.0 ** e).float().to(DEV)
        got = ops.conv2d_resup2(x, pack, low, x_range=r)
        want = ops.conv2d(x, pack, residual=M.up2_reference(low), x_range=r)
        _, _, exact = mag_operands(d, p, q)                          # the conv under the blended residual, through ops.conv2d
        assert torch.equal(ops.conv2d(x, pack, x_range=r).cpu(), exact)
    assert torch.equal(got, want), (case_id(case), p, q, (got - want).abs().max().item())
    assert got.abs().max() > 0                                       # (an unscale that underflowed made both sides 0)
    assert ops.f16x3_saturation_count() == 0
