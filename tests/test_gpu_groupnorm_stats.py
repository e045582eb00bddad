"""GroupNorm statistics when a group's |mean| is large against its spread (|mean| / sigma up to 1000).

Every statistics path of the hot slice is compared with float64 statistics of the exact fp32 tensor it normalised, next to ATen's own
fp32 GroupNorm on the same tensor (printed for comparison).  A one-pass `E[x^2] - mean^2` in fp32 cancels catastrophically in this
regime; the bars below are the fp32 rounding of the stored mean and 1e-5 on rstd.

Paths (norm.hip, flowfield.hip, the conv epilogue + gn_tile_finalize_kernel):
  plain tensor: gn_stats_direct (span <= 65536, float4 and scalar loops), gn_partial + gn_finalize (larger spans);
  split-K conv output: gn_stats_split (256- and 1024-thread launches), the bias added before squaring;
  conv epilogue: direct f16x3 kernel (td 4 / td 2), the F(2,3) role-split, lockstep and big-tile schedules, the two-frame mode,
  and the conv with the previous GroupNorm folded into its input;
  tiny tensors: gn_small_fused, FlowField's block kernels (ff_finish) and output head (GroupNorm(1, 3)).
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as R

pytestmark = pytest.mark.gpu

RATIOS = [0, 10, 100, 300, 1000]
EPS = 1e-5


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


def maxabs(a, b):
    return (a.detach().cpu().double() - torch.as_tensor(b).double()).abs().max().item()


def stats64(y, groups):
    """float64 (mean, rstd, sigma) per (sample, group) of the fp32 tensor y: biased variance, eps inside the sqrt (F.group_norm)."""
    yr = y.detach().cpu().double().reshape(y.shape[0] * groups, -1)
    m = yr.mean(-1)
    v = (yr - m[:, None]).square().mean(-1)
    return m, 1.0 / torch.sqrt(v + EPS), v.sqrt()


def aten_stats(y, groups):
    n, c = y.shape[0], y.shape[1]
    _, m, r = torch.ops.aten.native_group_norm(y.detach().contiguous(), None, None, n, c, y[0, 0].numel(), groups, EPS)
    return m.reshape(-1), r.reshape(-1)


def stats_errors(st_mean, st_rstd, m64, r64, s64):
    """(worst |mean - mean64| in units of its bar, worst |rstd / rstd64 - 1|)"""
    em = ((st_mean.detach().cpu().double() - m64).abs() / (2.0 ** -23 * m64.abs() + 1e-6 * s64)).max().item()
    er = (st_rstd.detach().cpu().double() / r64 - 1.0).abs().max().item()
    return em, er


def check_stats(label, st, y, groups):
    """st: [N*G, 2] (mean, rstd) a kernel computed for the fp32 tensor y."""
    m64, r64, s64 = stats64(y, groups)
    ratio = (m64.abs() / s64).max().item()
    em, er = stats_errors(st[:, 0], st[:, 1], m64, r64, s64)
    am, ar = aten_stats(y, groups)
    aem, aer = stats_errors(am, ar, m64, r64, s64)
    print(f"{label}: |mean|/sigma <= {ratio:.0f}: kernel mean {em:.2f} of bar, rstd rel {er:.2e} | ATen fp32 mean {aem:.2f} of bar, "
          f"rstd rel {aer:.2e}")
    assert em <= 1.0, f"{label}: mean off by {em:.2f}x its bar"
    assert er <= 1e-5, f"{label}: rstd relative error {er:.2e}"
    return ratio


def offset_tensor(shape, seed, ratio, sigma=0.5):
    """sigma * (u + ratio * 0.577 * (+-1 per sample)): u uniform in [-1, 1) (std 0.577), so |mean| / std ~= ratio."""
    u = R.seeded_tensor(shape, seed)
    sgn = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(shape[0])]).view(-1, *([1] * (len(shape) - 1)))
    return (sigma * (u + ratio * 0.57735 * sgn)).float().contiguous()


# ------------------------------------------------------------------------------- plain tensors: gn_stats_direct / gn_partial + gn_finalize
PLAIN_CASES = [((2, 96, 4, 8, 8), 32),          # span 768: direct, float4 loop
               ((2, 64, 3, 5, 7), 32),          # span 210: direct, scalar loop
               ((1, 64, 16, 64, 32), 32),       # span 65536 exactly: direct (4 chunks)
               ((1, 128, 5, 29, 113), 32),      # span 65540: two-stage, float4 loop
               ((1, 64, 3, 129, 129), 32),      # span 99846: two-stage, scalar loop
               ((1, 96, 16, 64, 64), 32)]       # span 196608: two-stage (G3d level 0)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("shape,groups", PLAIN_CASES, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_groupnorm_stats_plain_tensor(ops, dev, shape, groups, ratio):
    x = offset_tensor(shape, 901, ratio)
    st = ops.groupnorm_stats(x.to(dev), groups)
    got = check_stats(f"plain {shape} span {shape[1] // groups * x[0, 0].numel()}", st, x, groups)
    assert got >= 0.9 * ratio


# ------------------------------------------------------------------------------- split-K conv output: gn_stats_split
SPLIT_CASES = [(2, 256, 128, 8, 2, 2),   # span 128: 256-thread launch
               (2, 64, 64, 16, 8, 8)]    # span 2048: 1024-thread launch


def _split_conv(ops, dev, case, seed, ratio):
    """conv3d_split output whose groups sit at |mean| / sigma ~= ratio: the offset is a bias shared by every channel."""
    n, ci, co, d, h, w = case
    x = R.seeded_tensor((n, ci, d, h, w), seed, scale=1.7)
    wt = R.seeded_tensor((co, ci, 3, 3, 3), seed + 1, scale=(ci * 27) ** -0.5)
    sigma = F.conv3d(x.double(), wt.double(), None, padding=1).reshape(n * 32, -1).std(-1).mean().item()
    bias = torch.full((co,), ratio * sigma, dtype=torch.float32) + R.seeded_tensor((co,), seed + 2, scale=0.1)
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    co_ = ops.conv3d_split(x.to(dev), pc, precision=0)
    assert co_.splits > 1, "this shape is meant to exercise split-K"
    exact = co_.data.double().sum(0) + co_.bias.double().view(1, -1, 1, 1, 1)   # float64 of the value the kernels form
    return co_, exact.float(), exact


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_groupnorm_stats_split_k(ops, dev, case, ratio):
    co, y32, y64 = _split_conv(ops, dev, case, 911, ratio)
    st = ops.groupnorm_stats(co, 32)
    n = case[0]
    m64 = y64.cpu().reshape(n * 32, -1).mean(-1)
    v64 = (y64.cpu().reshape(n * 32, -1) - m64[:, None]).square().mean(-1)
    r64, s64 = 1.0 / torch.sqrt(v64 + EPS), v64.sqrt()
    em, er = stats_errors(st[:, 0], st[:, 1], m64, r64, s64)
    am, ar = aten_stats(y32.to(dev), 32)
    aem, aer = stats_errors(am, ar, m64, r64, s64)
    print(f"split-K {case} ({co.splits} slabs), |mean|/sigma <= {(m64.abs() / s64).max().item():.0f}: kernel mean {em:.2f} of bar, "
          f"rstd rel {er:.2e} | ATen fp32 mean {aem:.2f} of bar, rstd rel {aer:.2e}")
    assert em <= 1.0 and er <= 1e-5


# ------------------------------------------------------------------------------- tiny tensors: gn_small_fused
@pytest.mark.parametrize("ratio", RATIOS)
def test_groupnorm_small_fused_offset_invariance(ops, dev, ratio):
    case = (2, 256, 128, 8, 2, 2)
    co, y32, y64 = _split_conv(ops, dev, case, 921, ratio)
    assert ops.groupnorm_fused_ok(co, 32)
    c = case[2]
    g, b = R.seeded_tensor((c,), 925, scale=0.25, shift=1.0), R.seeded_tensor((c,), 926, scale=0.25)
    w2, b2 = R.seeded_tensor((1, c, 1, 1, 1), 927, scale=0.25, shift=1.0), R.seeded_tensor((1, c, 1, 1, 1), 928, scale=0.25)
    ref = lambda y: F.relu(F.group_norm(y, 32, g.to(y), b.to(y), EPS) * w2.to(y) + b2.to(y))
    truth = ref(y64.cpu())
    aten = ref(y32.to(dev)).cpu().double()
    got = ops.groupnorm_small(co, g.to(dev), b.to(dev), 32, EPS, w2=w2.to(dev), b2=b2.to(dev), relu=True)
    e_new, e_cpu, scale = maxabs(got, truth), (aten - truth).abs().max().item(), truth.abs().max().item()
    print(f"groupnorm_small r={ratio}: kernel {e_new:.2e}, ATen fp32 {e_cpu:.2e} (|y|max {scale:.2f})")
    assert e_new <= max(3.0 * e_cpu, 1e-6 * scale)


# ------------------------------------------------------------------------------- conv epilogue: per-row partials + gn_tile_finalize
# (name, shape, environment, mphip_conv3d_kernel_variant): the statistics of every unsplit f16x3 launch come from its epilogue; the
# two-frame mode has no epilogue partials and takes the separate pass over the stored output
CONV_CASES = [("direct-td4", (2, 96, 96, 16, 64, 32), {"MPHIP_F16X3_TILE": "0"}, 1),
              ("direct-td2", (4, 96, 96, 2, 64, 128), {"MPHIP_F16X3_TILE": "0"}, 1),
              ("wino-role-split", (2, 96, 96, 16, 64, 32), {}, 5),
              ("wino-lockstep", (2, 96, 96, 16, 64, 32), {"MPHIP_WINO_PP": "0"}, 5),
              ("wino-big-tile", (2, 96, 96, 16, 64, 32), {"MPHIP_WINO_PP": "2"}, 5),
              ("wino-two-frame", (4, 96, 96, 2, 64, 128), {}, 5)]


def _dc_conv(shape, seed):
    """Post-ReLU-like input and weights whose DC comes through the weights: x >= 0, input channel 0 a constant plane, and a delta on
    the centre tap of that channel (inside the volume for every output voxel: a uniform DC, no padding-border gradient)."""
    n, ci, co, d, h, w = shape
    x = R.seeded_tensor((n, ci, d, h, w), seed, scale=1.7).abs()
    x[:, 0] = 1.7
    wt = R.seeded_tensor((co, ci, 3, 3, 3), seed + 1, scale=(ci * 27) ** -0.5)
    return x.contiguous(), wt


# (ratio, large bias): the large bias (+1000) covers the 2*b*sa + nr*b^2 terms of the finalize, once plain and once with the DC as well
CONV_RUNS = [(r, False) for r in RATIOS] + [(0, True), (300, True)]


@pytest.mark.parametrize("ratio,big_bias", CONV_RUNS, ids=lambda v: f"r{v}" if not isinstance(v, bool) else ("bias1000" if v else "bias"))
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c[0])
def test_conv_epilogue_groupnorm_stats(ops, _libmod, dev, case, ratio, big_bias, monkeypatch):
    name, shape, env, variant = case
    n, ci, co, d, h, w = shape
    monkeypatch.setenv("MPHIP_WINOGRAD_MIN_TILES", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert _libmod.load().mphip_conv3d_kernel_variant(n, ci, co, d, h, w, 3, 1) == variant
    x, wt = _dc_conv(shape, 931)
    bias = R.seeded_tensor((co,), 933, scale=0.5) + (1000.0 if big_bias else 0.0)
    xd = x.to(dev)
    if ratio:   # sigma of the output from a launch without the DC, then the DC that puts the groups at the target ratio
        y0 = ops.conv3d(xd, ops.PackedConv(wt.to(dev), bias.to(dev)), precision=1)
        sigma = stats64(y0, 32)[2].median().item()
        wt[:, 0, 1, 1, 1] += ratio * sigma / 1.7
    pc = ops.PackedConv(wt.to(dev), bias.to(dev))
    y, st = ops.conv3d(xd, pc, precision=1, gn_groups=32)
    got = check_stats(f"conv {name} r={ratio}{' +1000 bias' if big_bias else ''}", st, y, 32)
    if not big_bias:
        assert got >= 0.5 * ratio


@pytest.mark.parametrize("ratio", RATIOS)
def test_conv_gn_in_epilogue_groupnorm_stats(ops, _libmod, dev, ratio, monkeypatch):
    """conv(relu(GN(x))) with the output statistics (mphip_conv3d_gnin_gn_fwd): the DC through the weights again; the input's GroupNorm
    keeps channel 0 of the normalised input near its beta, so the delta sits on the centre tap of every input channel."""
    shape = (2, 96, 96, 16, 64, 32)
    n, ci, co, d, h, w = shape
    monkeypatch.setenv("MPHIP_WINOGRAD_MIN_TILES", "1")
    x = R.seeded_tensor((n, ci, d, h, w), 941, scale=1.7)
    wt = R.seeded_tensor((co, ci, 3, 3, 3), 942, scale=(ci * 27) ** -0.5)
    bias = R.seeded_tensor((co,), 943, scale=0.5)
    g, b = R.seeded_tensor((ci,), 944, scale=0.01, shift=0.03), R.seeded_tensor((ci,), 945, scale=0.05, shift=2.0)   # relu(.) ~ 2 +- small
    xd = x.to(dev)
    sx = ops.groupnorm_stats(xd, 32)
    run = lambda wt_: ops.conv3d_gn_in(xd, sx, g.to(dev), b.to(dev), 32, ops.PackedConv(wt_.to(dev), bias.to(dev)), out_gn_groups=32)
    if ratio:
        sigma = stats64(run(wt)[0], 32)[2].median().item()
        wt[:, :, 1, 1, 1] += ratio * sigma / (2.0 * ci)
    y, st = run(wt)
    check_stats(f"conv_gn_in r={ratio}", st, y, 32)


# ------------------------------------------------------------------------------- FlowField: ff_finish and the output head
FF_LEVELS = [(512, 256, 4, 1, 1, (2, 2, 2)), (256, 128, 8, 2, 2, (2, 2, 2)), (128, 64, 16, 4, 4, (1, 2, 2))]


def _group_sigma(y, groups=32):
    return y.reshape(y.shape[0] * groups, -1).std(-1, unbiased=False).median().item()


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("level", FF_LEVELS, ids=["512-256@4x1x1", "256-128@8x2x2", "128-64@16x4x4"])
def test_flowfield_block_offset_invariance(ops, M, dev, level, ratio):
    """Both GroupNorms of a FlowField block at |mean| / sigma ~= ratio (an offset on the conv bias, shared by every channel): the block's
    output does not depend on the offset, and must match the float64 evaluation of the shifted block."""
    ci, co, d, h, w, up = level
    torch.manual_seed(77)
    blk = M.ResBlock3D_Adaptive(ci, co)
    with torch.no_grad():
        for nrm in (blk.norm1, blk.norm2):
            nrm.group_norm.weight.uniform_(0.5, 1.5); nrm.group_norm.bias.uniform_(-0.5, 0.5)
            nrm.weight.uniform_(0.5, 1.5); nrm.bias.uniform_(-0.5, 0.5)
    x = R.seeded_tensor((3, ci, d, h, w), 951, scale=1.7)

    def ref(dt, taps=None):
        c = lambda t: t.detach().to(dt)
        agn = lambda y, nrm: F.group_norm(y, 32, c(nrm.group_norm.weight), c(nrm.group_norm.bias), EPS) * c(nrm.weight) + c(nrm.bias)
        y1 = F.conv3d(x.to(dt), c(blk.conv1.weight), c(blk.conv1.bias), padding=1)
        y = F.relu(agn(y1, blk.norm1))
        y2 = F.conv3d(y, c(blk.conv2.weight), c(blk.conv2.bias), padding=1)
        if taps is not None:
            taps.extend([y1, y2])
        y = F.relu(agn(y2, blk.norm2) + F.conv3d(x.to(dt), c(blk.residual_conv.weight), c(blk.residual_conv.bias)))
        return F.interpolate(y, scale_factor=up, mode="nearest")

    taps = []
    base = ref(torch.float64, taps)
    with torch.no_grad():
        blk.conv1.bias += ratio * _group_sigma(taps[0])
        blk.conv2.bias += ratio * _group_sigma(taps[1])
    taps = []
    truth, cpu32 = ref(torch.float64, taps), ref(torch.float32).double()
    ratios = [(t.reshape(3 * 32, -1).mean(-1).abs() / t.reshape(3 * 32, -1).std(-1, unbiased=False)).median().item() for t in taps]
    blk = blk.to(dev).eval()
    with torch.no_grad():
        a = ops.flowfield_conv_gn(x.to(dev), blk.conv1, blk.norm1, relu=True)
        got = ops.flowfield_conv_gn(a, blk.conv2, blk.norm2, res_x=x.to(dev), res_conv=blk.residual_conv, relu=True, up=up).cpu().double()
    scale = truth.abs().max().item()
    e_new, e_cpu = (got - truth).abs().max().item(), (cpu32 - truth).abs().max().item()
    print(f"flowfield {ci}->{co} r={ratio} (|mean|/sigma {ratios[0]:.0f}, {ratios[1]:.0f}): kernel {e_new:.2e}, ATen fp32 {e_cpu:.2e} "
          f"(|y|max {scale:.2f}; shifted vs unshifted float64 {(truth - base).abs().max().item():.1e})")
    assert e_new <= max(3.0 * e_cpu, 1e-6 * scale)
    assert (got - base).abs().max().item() <= max(3.0 * e_cpu, 1e-6 * scale)


@pytest.mark.parametrize("ratio", RATIOS)
def test_flowfield_output_head_offset_invariance(ops, M, dev, ratio):
    torch.manual_seed(78)
    ff = M.FlowField()
    with torch.no_grad():
        ff.gn.weight.uniform_(0.5, 1.5); ff.gn.bias.uniform_(-0.5, 0.5)
    x = R.seeded_tensor((3, 32, 16, 16, 16), 961, scale=1.7)
    conv = lambda dt: F.conv3d(x.to(dt), ff.conv3x3x3.weight.detach().to(dt), ff.conv3x3x3.bias.detach().to(dt), padding=1)
    ref = lambda dt: torch.tanh(F.relu(F.group_norm(conv(dt), 1, ff.gn.weight.detach().to(dt), ff.gn.bias.detach().to(dt), EPS)))
    base = ref(torch.float64)
    with torch.no_grad():
        ff.conv3x3x3.bias += ratio * _group_sigma(conv(torch.float64), 1)
    y = conv(torch.float64).reshape(3, -1)
    got_ratio = (y.mean(-1).abs() / y.std(-1, unbiased=False)).min().item()
    truth, cpu32 = ref(torch.float64), ref(torch.float32).double()
    ff = ff.to(dev).eval()
    with torch.no_grad():
        got = ops.flowfield_out(x.to(dev), ff.conv3x3x3, ff.gn).cpu().double()
    e_new, e_cpu = (got - truth).abs().max().item(), (cpu32 - truth).abs().max().item()
    print(f"flowfield output head r={ratio} (|mean|/sigma >= {got_ratio:.0f}): kernel {e_new:.2e}, ATen fp32 {e_cpu:.2e}")
    assert e_new <= max(3.0 * e_cpu, 1e-6)
    assert (got - base).abs().max().item() <= max(3.0 * e_cpu, 1e-6)


# ------------------------------------------------------------------------------- backward on offset-dominated inputs
def rel_err(got, want):
    want = want.detach().double()
    return (got.detach().cpu().double() - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


@pytest.mark.parametrize("relu,adaptive", [(False, False), (True, False), (True, True)])
def test_groupnorm_bwd_offset_dominated(ops, dev, relu, adaptive):
    shape = (2, 96, 4, 8, 8)
    c = shape[1]
    x = offset_tensor(shape, 971, 300).double().requires_grad_(True)
    gamma = R.seeded_tensor((c,), 972, scale=0.25, shift=1.0).double().requires_grad_(True)
    beta = R.seeded_tensor((c,), 973, scale=0.25).double().requires_grad_(True)
    w2 = R.seeded_tensor((1, c, 1, 1, 1), 974, scale=0.25, shift=1.0).double()
    b2 = R.seeded_tensor((1, c, 1, 1, 1), 975, scale=0.25).double()
    dy = R.seeded_tensor(shape, 976)
    xg = x.detach().float().to(dev)
    st = ops.groupnorm_stats(xg, 32, EPS)
    gf, bf = gamma.detach().float().to(dev), beta.detach().float().to(dev)
    kw = dict(w2=w2.float().to(dev), b2=b2.float().to(dev)) if adaptive else {}
    yg = ops.groupnorm_apply(xg, st, gf, bf, 32, relu=relu, **kw)
    u = F.group_norm(x, 32, gamma, beta, EPS)
    if adaptive:
        u = u * w2 + b2
    # the ReLU mask of the kernel's own forward: a pre-activation within the fp32 rounding of the stored mean (2^-24 |mean|, ~1e-5 sigma
    # at this ratio) of zero may flip, and a flipped element moves dx by a whole dy * gamma * rstd
    y = u * (yg.cpu() > 0).double() if relu else u
    y.backward(dy.double())
    assert rel_err(yg, y) < 1e-4
    out = ops.groupnorm_bwd(xg, yg, dy.to(dev), st, gf, 32, relu, False, beta=bf if adaptive else None,
                            w2=kw.get("w2"))
    dx, dgamma, dbeta = out[0], out[1], out[2]
    errs = rel_err(dx, x.grad), rel_err(dgamma, gamma.grad), rel_err(dbeta, beta.grad)
    print(f"groupnorm_bwd r=300 relu={relu} adaptive={adaptive}: dx {errs[0]:.2e}, dgamma {errs[1]:.2e}, dbeta {errs[2]:.2e}")
    assert max(errs) < 1e-4
