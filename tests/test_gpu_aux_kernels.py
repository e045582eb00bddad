"""Every host-side dispatch branch of the kernels around the convs — the resamplers and their adjoints, the two small GEMMs, the GroupNorm
apply / backward and the casts (csrc/norm.hip, csrc/backward.hip, csrc/api.hip) — against a plain CPU reference, at the hot slice's own
spatial sizes (few channel planes: the kernels work per plane) and on both sides of every divisibility / size / alignment condition.
A case id names the branch it reaches.

References and bounds (derived, not tuned against the kernels; u = 2^-24):
 * bit-exact kernels (pool, x2 trilinear, nearest, scaled trilinear, casts): torch.equal against the operation written out in its plain
   fp32 order (`_pool_restated`, `_trilinear_restated`); ATen's CPU result is compared with that restatement first and, on this
   software stack, equals it at every shape used here, so the contract of test_resample_bit_exact (ATen) is the same contract.
 * sums in fp32 (add_matmul, nearest adjoint, trilinear adjoints): float64 truth, elementwise |err| <= (terms + 2) * u * sum|products|
   (every product passes at most `terms - 1` additions in any order, its own rounding and one more for a2 / bias).  The trilinear
   adjoints get one more term, see `_adjoint_case`.
 * small_gemm accumulates in double: one fp32 rounding of the result, 2^-23 * |out| + K * 2^-52 * (|a| @ |b|); with a2 the kernel forms
   a + a2 in fp32 first: + u * (|a + a2| @ |b|).
 * GroupNorm backward: float64 autograd, the bars of test_groupnorm_bwd (1e-4 of the maximum for dx / dgamma / dbeta (/ dw2 / db2),
   1e-6 for dres).
Worst measured values are recorded beside each bound (MI355X, this file's own run)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from megaportrait_hack_amd import _lib, ops

    _lib.load()
    return ops


def _offset_view(t: torch.Tensor, dev) -> torch.Tensor:
    """A contiguous device copy of `t` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _check_bound(name, got, truth, bound):
    """elementwise |got - truth| <= bound (float64); prints the worst error / bound ratio"""
    err = (got.detach().cpu().double() - truth).abs()
    assert err.shape == bound.shape, (err.shape, bound.shape)
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, worst err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), (name, ratio)
    return ratio


def _rel_err(got, want):
    want = want.detach().double()
    return (got.detach().cpu().double() - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


# ------------------------------------------------------------------ the resampling rules written out (fp32, ATen's index rules)
def _axis_rule(n_in, n_out, align):
    """ATen's source-index rule of one axis in fp32: (i0, i1, l0, l1) per output index.  One fp32 division for the scale."""
    dst = np.arange(n_out, dtype=np.float32)
    if align:
        scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
        src = scale * dst
    else:
        scale = np.float32(n_in) / np.float32(n_out)
        src = np.maximum(scale * (dst + np.float32(0.5)) - np.float32(0.5), np.float32(0.0))
    assert src.dtype == np.float32
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    return i0, i1, l0, l1


def _lerp32(l0, a, l1, b):
    """fmaf(l0, a, l1 * b) in fp32 — the lerp ATen's CPU kernel and the HIP kernels both evaluate: l1 * b rounded to fp32, l0 * a exact
    (a 48-bit product in float64), one rounding of the sum."""
    p = (l1 * b).astype(np.float32)
    return (l0.astype(np.float64) * a.astype(np.float64) + p.astype(np.float64)).astype(np.float32)


def _trilinear_restated(x: torch.Tensor, scale, align: bool) -> torch.Tensor:
    """F.interpolate(x, scale_factor=scale, mode='trilinear', align_corners=align) as the nested W -> H -> D lerp in fp32."""
    v = x.numpy()
    for axis, s in ((4, scale[2]), (3, scale[1]), (2, scale[0])):
        n_in = v.shape[axis]
        i0, i1, l0, l1 = _axis_rule(n_in, n_in * s, align)
        shp = [1] * 5
        shp[axis] = -1
        v = _lerp32(l0.reshape(shp), np.take(v, i0, axis), l1.reshape(shp), np.take(v, i1, axis))
    return torch.from_numpy(np.ascontiguousarray(v))


def _pool_restated(x: torch.Tensor) -> torch.Tensor:
    """nn.AvgPool3d(2, 2): the eight values added one after the other (d, then h, then w fastest) in fp32, then / 8."""
    s = None
    for a in range(2):
        for b in range(2):
            for c in range(2):
                t = x[:, :, a::2, b::2, c::2]
                s = t.clone() if s is None else s + t
    return s / 8.0


def _reference(aten: torch.Tensor, restated: torch.Tensor, what: str) -> torch.Tensor:
    """The bit-exact reference is the restatement; ATen is checked against it (it agrees at every shape of this file on the stack the
    suite runs on — if an ATen build ever departs from the plain order, the restatement stays the reference and this says so)."""
    if not torch.equal(aten, restated):
        print(f"{what}: ATen's CPU result departs from the plain fp32 order here; the restatement is the reference")
    return restated


def _axis_matrix(n_in, n_out, align, exact: bool) -> torch.Tensor:
    """[n_out, n_in] float64 weights of one axis: the fp32 rule above, or (exact) the same rule evaluated in float64 like ATen does for a
    float64 tensor."""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    if exact:
        dst = np.arange(n_out, dtype=np.float64)
        if align:
            src = (float(n_in - 1) / float(n_out - 1) if n_out > 1 else 0.0) * dst
        else:
            src = np.maximum(float(n_in) / float(n_out) * (dst + 0.5) - 0.5, 0.0)
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        l1 = src - i0
        l0 = 1.0 - l1
    else:
        i0, i1, l0, l1 = _axis_rule(n_in, n_out, align)
    o = torch.arange(n_out)
    m.index_put_((o, torch.from_numpy(i0)), torch.from_numpy(l0.astype(np.float64)), accumulate=True)
    m.index_put_((o, torch.from_numpy(i1)), torch.from_numpy(l1.astype(np.float64)), accumulate=True)
    return m


def _adjoint(g, md, mh, mw):
    return torch.einsum("ncdhw,di,hj,wk->ncijk", g, md, mh, mw)


# ================================================================== bit-exact resamplers
UP2_SHAPES = {
    "brick-hot-2x8x8": (1, 4, 2, 8, 8), "brick-hot-4x16x16": (1, 4, 4, 16, 16), "brick-hot-8x32x32": (1, 3, 8, 32, 32),
    "brick-W2": (2, 3, 2, 3, 2), "brick-W6-odd-brick-count": (1, 4, 3, 5, 6), "brick-D1": (1, 3, 1, 4, 4), "brick-H1": (1, 3, 2, 1, 4),
    "brick-D1-H1": (1, 5, 1, 1, 8),
    "scalar-W5": (1, 3, 3, 4, 5), "scalar-W1": (1, 2, 2, 2, 1), "scalar-D1-H1-W3": (1, 2, 1, 1, 3), "scalar-W7-H1": (2, 3, 4, 1, 7),
}


@pytest.mark.parametrize("case", list(UP2_SHAPES))
def test_upsample_trilinear2_bit_exact(ops, dev, case):
    """mphip_upsample_trilinear2: the brick kernel (W even) and the scalar kernel (W odd), D = 1 / H = 1 (scale 0) included."""
    shape = UP2_SHAPES[case]
    assert (shape[4] % 2 == 0) == case.startswith("brick")
    x = R.seeded_tensor(shape, 1101, scale=3.0)
    ref = _reference(F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=True), _trilinear_restated(x, (2, 2, 2), True), case)
    assert torch.equal(ops.upsample_trilinear2(x.to(dev)).cpu(), ref)


POOL_SHAPES = {"pool-hot-4x16x16": (1, 4, 4, 16, 16), "pool-hot-8x32x32": (1, 4, 8, 32, 32), "pool-hot-16x64x64": (1, 3, 16, 64, 64),
               "pool-2x2x2": (3, 5, 2, 2, 2), "pool-W6": (1, 3, 4, 2, 6), "pool-W2": (2, 2, 6, 4, 2)}


@pytest.mark.parametrize("case", list(POOL_SHAPES))
def test_avgpool2_and_its_adjoint_bit_exact(ops, dev, case):
    shape = POOL_SHAPES[case]
    x = R.seeded_tensor(shape, 1201, scale=3.0)
    ref = _reference(F.avg_pool3d(x, 2, 2), _pool_restated(x), case)
    assert torch.equal(ops.avgpool2(x.to(dev)).cpu(), ref)
    # adjoint: every input voxel receives dout / 8 (one fp32 division, no sum): ATen's own backward, bit for bit
    xg = x.clone().requires_grad_(True)
    dout = R.seeded_tensor(tuple(ref.shape), 1202, scale=2.0)
    F.avg_pool3d(xg, 2, 2).backward(dout)
    restated = (dout / 8.0).repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
    assert torch.equal(ops.avgpool2_bwd(dout.to(dev)).cpu(), _reference(xg.grad, restated, case + " (adjoint)"))


NEAREST_SHAPES = {"4x1x1": (2, 4, 4, 1, 1), "8x2x2": (1, 5, 8, 2, 2), "16x4x4": (1, 3, 16, 4, 4), "3x5x7": (1, 2, 3, 5, 7)}


@pytest.mark.parametrize("scale", [(2, 2, 2), (1, 2, 2), (3, 1, 2)], ids=lambda s: "x%d%d%d" % s)
@pytest.mark.parametrize("case", list(NEAREST_SHAPES))
def test_upsample_nearest_and_its_adjoint(ops, dev, case, scale):
    """FlowField's nearest upsamples (scales (2,2,2) and (1,2,2) at its three levels) and mphip_upsample_nearest_bwd, which had no direct test."""
    shape = NEAREST_SHAPES[case]
    x = R.seeded_tensor(shape, 1301, scale=3.0)
    restated = x.repeat_interleave(scale[0], 2).repeat_interleave(scale[1], 3).repeat_interleave(scale[2], 4)
    ref = _reference(F.interpolate(x, scale_factor=tuple(float(s) for s in scale), mode="nearest"), restated, case)
    assert torch.equal(ops.upsample_nearest(x.to(dev), scale).cpu(), ref)
    # adjoint: a sum of sD*sH*sW gradients per input voxel
    dout = R.seeded_tensor(tuple(ref.shape), 1302, scale=2.0)
    xd = x.double().requires_grad_(True)
    F.interpolate(xd, scale_factor=tuple(float(s) for s in scale), mode="nearest").backward(dout.double())
    terms = scale[0] * scale[1] * scale[2]
    absum = F.avg_pool3d(dout.double().abs(), scale, scale) * terms
    # worst measured err / bound: 0.31
    _check_bound(f"nearest_bwd {case} {scale}", ops.upsample_nearest_bwd(dout.to(dev), scale), xd.grad, (terms + 2) * U * absum)


@pytest.mark.parametrize("scale", [(2, 2, 3), (2, 2, 2), (1, 2, 2), (3, 1, 2)], ids=lambda s: "x%d%d%d" % s)
@pytest.mark.parametrize("shape", [(1, 3, 4, 16, 16), (2, 2, 3, 5, 4), (1, 4, 1, 1, 5)], ids=lambda s: "x".join(map(str, s[2:])))
def test_upsample_trilinear_scaled_and_its_adjoint(ops, dev, shape, scale):
    """mphip_upsample_trilinear (align_corners=False, integer factors) bit for bit, and its atomic-scatter adjoint against float64 autograd.
    With a factor of 3 on an axis ATen's CPU kernel itself departs from the plain order (its source coordinate scale * (dst + 0.5) - 0.5
    is not rounded once per operation there; up to 1.3e-6 on these data, which is why test_resblock_upsample_branch allows 2 ulp): the
    restatement — one fp32 rounding per operation, ATen's index rule — is the bit-exact reference at those scales.  With factors 1 and 2
    ATen equals it."""
    x = R.seeded_tensor(shape, 1401, scale=3.0)
    sf = tuple(float(s) for s in scale)
    ref = _reference(F.interpolate(x, scale_factor=sf, mode="trilinear", align_corners=False), _trilinear_restated(x, scale, False), str(shape))
    assert torch.equal(ops.upsample_trilinear(x.to(dev), scale).cpu(), ref)
    if x.numel() % 4 == 0:       # (the entry requires a 16-byte multiple for its zero fill)
        _adjoint_case(f"trilinear_bwd {shape} {scale}", shape, scale, False, 1402, lambda g: ops.upsample_trilinear_bwd(g, scale), dev)


def _adjoint_case(name, in_shape, scale, align, seed, run, dev, dout=None):
    """A trilinear adjoint against float64 autograd through F.interpolate.  Bound: the sum over the <= `terms` outputs that touch an
    input voxel, (terms + 2) * u * sum |w| |dout| — plus the term the plain derivation misses: the kernels use the FORWARD's fp32
    weights (source coordinate scale * dst evaluated in fp32, as ATen's fp32 forward does), the float64 truth evaluates the same rule in
    float64.  That difference is not a rounding of the sum; it is bounded exactly, from the two index rules alone, by
    sum_o |w32(o, i) - w64(o, i)| * |dout[o]| with the tensor-product difference telescoped over the three axes."""
    n, c, d, h, w = in_shape
    out_shape = (n, c, d * scale[0], h * scale[1], w * scale[2])
    if dout is None:
        dout = R.seeded_tensor(out_shape, seed, scale=2.0)
    xd = torch.zeros(in_shape, dtype=torch.float64, requires_grad=True)
    F.interpolate(xd, scale_factor=tuple(float(s) for s in scale), mode="trilinear", align_corners=align).backward(dout.double())
    m32 = [_axis_matrix(i, i * s, align, False) for i, s in zip((d, h, w), scale)]
    m64 = [_axis_matrix(i, i * s, align, True) for i, s in zip((d, h, w), scale)]
    assert (_adjoint(dout.double(), *m64) - xd.grad).abs().max().item() <= 1e-12 * max(1.0, xd.grad.abs().max().item())   # the rule above IS ATen's
    g = dout.double().abs()
    dm = [(a - b).abs() for a, b in zip(m32, m64)]
    weights_term = _adjoint(g, dm[0], m32[1], m32[2]) + _adjoint(g, m64[0], dm[1], m32[2]) + _adjoint(g, m64[0], m64[1], dm[2])
    # outputs that touch one input index, per axis: < 2 / scale + 1 source intervals -> 5 for the x2 align_corners=True resize, 2 s for a factor s
    per_axis = [5 if align else 2 * s for s in scale]
    terms = per_axis[0] * per_axis[1] * per_axis[2]
    bound = (terms + 2) * U * _adjoint(g, *m32) + weights_term
    got = run(dout.to(dev) if dout.device.type == "cpu" else dout)
    return got, _check_bound(name, got, xd.grad, bound)


ADJ_SHAPES = {   # dx shapes; the middle (H) pass takes V = 4 when 2W % 4 == 0, the first (D) pass always (inner = 4HW), the last (W) never (inner = 1)
    "adjoint-hot-2x8x8-V4-middle": (1, 4, 2, 8, 8), "adjoint-hot-4x16x16-V4-middle": (1, 4, 4, 16, 16), "adjoint-hot-8x32x32-V4-middle": (1, 3, 8, 32, 32),
    "adjoint-V1-middle-W5": (1, 3, 3, 4, 5), "adjoint-V1-middle-W1": (2, 2, 2, 3, 1), "adjoint-V4-middle-W2": (1, 3, 2, 3, 2),
    "adjoint-V4-middle-W6": (1, 4, 3, 5, 6), "adjoint-D1": (1, 3, 1, 4, 4), "adjoint-H1-V1-middle": (1, 3, 2, 1, 3), "adjoint-D1-H1": (1, 2, 1, 1, 8),
}


@pytest.mark.parametrize("path", ["three-pass", "gather", "three-pass-V1-first-unaligned-dout"])
@pytest.mark.parametrize("case", list(ADJ_SHAPES))
def test_upsample_trilinear2_adjoint_paths(ops, dev, case, path):
    """mphip_upsample_trilinear2_bwd: the three separable passes (through ops; V = 4 / V = 1 per pass by `inner % 4`), the one-pass gather
    taken when workspace == NULL (ctypes: the Python host always passes a workspace), and the V = 1 first pass chosen for a dout that is
    not 16-byte aligned — each against float64 autograd; the unaligned call equals the aligned one bit for bit (per-element arithmetic,
    same tap order)."""
    from megaportrait_hack_amd import _lib

    shape = ADJ_SHAPES[case]
    n, c, d, h, w = shape

    def gather(g):
        dx = torch.empty(shape, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().mphip_upsample_trilinear2_bwd(ops._ptr(g), ops._ptr(dx), n * c, d, h, w, None, 0, ops._stream()),
                   "mphip_upsample_trilinear2_bwd")
        return dx

    dout = R.seeded_tensor((n, c, 2 * d, 2 * h, 2 * w), 1502, scale=2.0)
    if path == "gather":
        run = gather
    elif path == "three-pass":
        run = ops.upsample_trilinear2_bwd
    else:
        run = lambda g: ops.upsample_trilinear2_bwd(_offset_view(g, dev))
    # worst measured err / bound: 0.136 (three-pass, aligned or not), 0.137 (gather); the scaled adjoint above: 0.08
    got, _ = _adjoint_case(f"{case} {path}", shape, (2, 2, 2), True, 1502, run, dev, dout=dout)
    if path != "three-pass":
        aligned = ops.upsample_trilinear2_bwd(dout.to(dev))
        if path == "gather":   # a different summation order: close to the three passes, not equal; both met the float64 bound above
            assert _rel_err(got, aligned.cpu()) < 1e-5
        else:
            assert torch.equal(got, aligned)


# ================================================================== the two small GEMMs
# (B, K, N, trans, a2, bias)
ADD_MATMUL = {
    "nk-hot-B3-512x2048-bias": (3, 512, 2048, 1, False, True), "nk-B9-K100-N7-a2": (9, 100, 7, 1, True, False),
    "nk-B17-K513-N24-a2-bias": (17, 513, 24, 1, True, True), "nk-B1-K512-N2049": (1, 512, 2049, 1, False, False),
    "kn-hot-B8-512x512-a2": (8, 512, 512, 0, True, False), "kn-hot-head-B8-512x2048-a2-bias": (8, 512, 2048, 0, True, True),
    "kn-B1-K512-N512": (1, 512, 512, 0, False, False), "kn-B9-K512-N24-bias": (9, 512, 24, 0, False, True),
    "kn-B17-K100-N7-a2": (17, 100, 7, 0, True, False), "kn-B17-K512-N2049-a2-bias": (17, 512, 2049, 0, True, True),
    "kn-B3-K100-N24": (3, 100, 24, 0, False, False), "kn-B8-K64-N7-bias": (8, 64, 7, 0, False, True),
    "generic-B1-K513-N7": (1, 513, 7, 0, False, False), "generic-B9-K513-N2049-a2-bias": (9, 513, 2049, 0, True, True),
    "generic-B17-K1024-N24-a2": (17, 1024, 24, 0, True, False), "generic-B8-K513-N24-bias": (8, 513, 24, 0, False, True),
}


@pytest.mark.parametrize("case", list(ADD_MATMUL))
def test_add_matmul_branches(ops, dev, case):
    """mphip_add_matmul: trans = 1 wave kernel ("nk"), trans = 0 with K <= 512 (the LDS kernel, one launch per 8 rows: B = 1 / 8 / 9 / 17;
    N not a multiple of its 16 columns, K not a multiple of its 32 rows per iteration) and trans = 0 with K > 512 ("generic")."""
    b, k, n, trans, has_a2, has_bias = ADD_MATMUL[case]
    a = R.seeded_tensor((b, k), 1601, scale=1.7)
    a2 = R.seeded_tensor((b, k), 1602, scale=1.7) if has_a2 else None
    m = R.seeded_tensor((n, k) if trans else (k, n), 1603, scale=0.7)
    bias = R.seeded_tensor((n,), 1604, scale=0.5) if has_bias else None
    got = ops.add_matmul(a.to(dev), None if a2 is None else a2.to(dev), m.to(dev), None if bias is None else bias.to(dev), trans=bool(trans))
    s = a.double() + (a2.double() if has_a2 else 0.0)
    md = m.double().t() if trans else m.double()
    truth, absum = s @ md, s.abs() @ md.abs()
    if has_bias:
        truth, absum = truth + bias.double(), absum + bias.double().abs()
    # K products; each passes its own rounding (a + a2 in fp32), at most K - 1 additions in whatever order, and the bias addition.
    # worst measured err / bound: 0.009
    _check_bound(case, got, truth, (k + 2) * U * absum)


# (M, N, K, trans_a, trans_b, a2, bias)
SMALL_GEMM = {
    "small_gemm-wave-hot-512x1536x96": (512, 96, 1536, False, False, False, False),
    "small_gemm-wave-hot-1x1536x512-transB-bias": (1, 512, 1536, False, True, False, True),
    "small_gemm-thread-hot-512x512x2048": (512, 2048, 512, False, False, False, False),
    "small_gemm-wave-dz-ds@gammaT-transB": (8, 512, 512, False, True, False, False),          # AddMatmulFn.backward: dz
    "small_gemm-thread-dgamma-transA-a2": (512, 512, 8, True, False, True, False),              # ... dgamma = (z + e)^T @ ds
    "small_gemm-wave-ds-dx@w": (8, 512, 2048, False, False, False, False),                     # Conv1x1OnVectorFn.backward: ds
    "small_gemm-thread-dw-transA": (2048, 512, 8, True, False, False, False),                   # ... dw = dx^T @ s
    "small_gemm-thread-MN65537": (1, 65537, 128, False, False, False, False), "small_gemm-wave-MN65536": (256, 256, 128, False, False, False, True),
    "small_gemm-thread-K127": (5, 7, 127, False, False, True, True), "small_gemm-wave-K128": (5, 7, 128, False, False, True, True),
    "small_gemm-wave-plain": (5, 7, 130, False, False, False, False), "small_gemm-wave-transA": (5, 7, 130, True, False, True, False),
    "small_gemm-wave-transB": (5, 7, 130, False, True, False, True), "small_gemm-wave-transAB": (5, 7, 130, True, True, True, True),
    "small_gemm-thread-plain": (6, 11, 33, False, False, False, True), "small_gemm-thread-transA": (6, 11, 33, True, False, False, False),
    "small_gemm-thread-transB": (6, 11, 33, False, True, True, False), "small_gemm-thread-transAB": (6, 11, 33, True, True, True, True),
}


def _small_gemm_check(ops, dev, name, a, b, trans_a, trans_b, a2, bias):
    k = a.shape[0] if trans_a else a.shape[1]
    got = ops.small_gemm(a.to(dev), b.to(dev), trans_a=trans_a, trans_b=trans_b, a2=None if a2 is None else a2.to(dev),
                         bias=None if bias is None else bias.to(dev))
    s = a.double() + (a2.double() if a2 is not None else 0.0)
    s = s.t() if trans_a else s
    bd = b.double().t() if trans_b else b.double()
    truth, absum = s @ bd, s.abs() @ bd.abs()
    if bias is not None:
        truth, absum = truth + bias.double(), absum + bias.double().abs()
    assert tuple(got.shape) == tuple(truth.shape)
    bound = 2.0 ** -23 * truth.abs() + k * 2.0 ** -52 * absum        # one fp32 rounding of a double accumulation
    if a2 is not None:
        bound = bound + U * absum                                    # a + a2 is formed in fp32 before the product
    # worst measured err / bound: 0.73 (an a2 case; without a2 the final rounding alone: <= 0.5)
    _check_bound(name, got, truth, bound)


@pytest.mark.parametrize("case", list(SMALL_GEMM))
def test_small_gemm_branches(ops, dev, case):
    """mphip_small_gemm, which had no direct test: the wave kernel (M*N <= 65536 and K >= 128) and the thread kernel on both sides of both
    thresholds, the four trans_a / trans_b stride combinations at non-square sizes, a2, bias, the generators' own head products and the
    gradient forms of AddMatmulFn / Conv1x1OnVectorFn."""
    m, n, k, ta, tb, has_a2, has_bias = SMALL_GEMM[case]
    assert (("wave" in case) == (m * n <= 65536 and k >= 128))
    a = R.seeded_tensor((k, m) if ta else (m, k), 1701, scale=1.7)
    a2 = R.seeded_tensor(tuple(a.shape), 1702, scale=1.7) if has_a2 else None
    b = R.seeded_tensor((n, k) if tb else (k, n), 1703, scale=0.7)
    bias = R.seeded_tensor((n,), 1704, scale=0.5) if has_bias else None
    _small_gemm_check(ops, dev, case, a, b, ta, tb, a2, bias)


@pytest.mark.parametrize("rows", [8, 200], ids=["small_gemm-thread-db-ones-row-K8", "small_gemm-wave-db-ones-row-K200"])
def test_small_gemm_ones_row_bias_gradient(ops, dev, rows):
    """Conv1x1OnVectorFn.backward: db = ones(1, B) @ dx."""
    _small_gemm_check(ops, dev, f"db-K{rows}", torch.ones(1, rows), R.seeded_tensor((rows, 2048), 1711, scale=0.7), False, False, None, None)


def test_small_gemm_checks_its_bias(ops, dev):
    """ops.small_gemm routes `bias` through the same device / dtype / contiguity check as its other operands."""
    a, b = torch.ones(2, 4, device=dev), torch.ones(4, 6, device=dev)
    with pytest.raises(RuntimeError, match="bias: expected a CUDA tensor"):
        ops.small_gemm(a, b, bias=torch.zeros(6))
    with pytest.raises(RuntimeError, match="bias: expected torch.float32"):
        ops.small_gemm(a, b, bias=torch.zeros(6, dtype=torch.float64, device=dev))
    strided = torch.arange(12, dtype=torch.float32, device=dev)[::2]          # not contiguous: copied, not read with stride 1
    assert torch.equal(ops.small_gemm(a, b, bias=strided), torch.full((2, 6), 4.0, device=dev) + strided)


# ================================================================== GroupNorm apply
def _gn_forward64(x, groups, gamma, beta, w2, b2, res, act):
    """float64 restatement: GroupNorm -> second affine -> + residual -> ReLU (act >= 1) -> tanh (act == 2); returns (y, pre-activation)"""
    u = F.group_norm(x, groups, gamma, beta, 1e-5)
    if w2 is not None:
        u = u * w2.view(1, -1, 1, 1, 1) + b2.view(1, -1, 1, 1, 1)
    if res is not None:
        u = u + res
    y = u
    if act >= 1:
        y = F.relu(y)
    if act == 2:
        y = torch.tanh(y)
    return y, u


GN_APPLY = {   # shape, groups
    "apply-vec4-hot-4x16x16": ((1, 8, 4, 16, 16), 4), "apply-vec4-S512": ((2, 64, 2, 16, 16), 32), "apply-scalar-S510": ((2, 64, 2, 15, 17), 32),
    "apply-vec4-S1028": ((1, 64, 1, 4, 257), 32), "apply-scalar-S15": ((2, 64, 1, 3, 5), 32),
}


@pytest.mark.parametrize("affine2", [False, True], ids=["gn", "adaptive"])
@pytest.mark.parametrize("case", list(GN_APPLY))
def test_groupnorm_apply_plain_form(ops, dev, case, affine2):
    """mphip_groupnorm_apply without pooling: the float4 kernel (S % 4 == 0 and 16-byte x / y / residual) and the scalar one (S % 4 != 0,
    or — the rule this entry shares with its pool form and with mphip_groupnorm_bwd — a pointer that is not 16-byte aligned).  Bar: the
    suite's own 1e-5 max-abs for O(1) data (test_groupnorm_parity); the unaligned call equals the aligned one bit for bit."""
    shape, groups = GN_APPLY[case]
    c = shape[1]
    x, res = R.seeded_tensor(shape, 1801, scale=2.0, shift=0.3), R.seeded_tensor(shape, 1802)
    g, b = R.seeded_tensor((c,), 1803, scale=0.25, shift=1.0), R.seeded_tensor((c,), 1804, scale=0.25)
    w2 = R.seeded_tensor((c,), 1805, scale=0.25, shift=1.0) if affine2 else None
    b2 = R.seeded_tensor((c,), 1806, scale=0.25) if affine2 else None
    D = lambda t: None if t is None else t.to(dev)
    st = ops.groupnorm_stats(x.to(dev), groups)
    for act, with_res in ((0, False), (1, True), (2, False)):
        want, _ = _gn_forward64(x.double(), groups, g.double(), b.double(), None if w2 is None else w2.double(),
                                None if b2 is None else b2.double(), res.double() if with_res else None, act)
        kw = dict(w2=D(w2), b2=D(b2), relu=act >= 1, tanh=act == 2)
        got = ops.groupnorm_apply(x.to(dev), st, D(g), D(b), groups, residual=D(res) if with_res else None, **kw)
        err = (got.cpu().double() - want).abs().max().item()
        print(f"{case} act={act}: max-abs {err:.2e}")      # worst measured: 5.5e-7
        assert err < 1e-5
        off = ops.groupnorm_apply(_offset_view(x, dev), st, D(g), D(b), groups, residual=_offset_view(res, dev) if with_res else None, **kw)
        assert torch.equal(off, got), f"{case}: scalar fallback for an unaligned x differs from the aligned call"


GN_POOL = {   # shape, groups: PW = 2 needs W % 4 == 0 and 16-byte pointers
    "pool-PW2-hot-16x64x64": ((1, 4, 16, 64, 64), 2), "pool-PW2-hot-8x32x32": ((1, 8, 8, 32, 32), 4), "pool-PW2-hot-4x16x16": ((2, 8, 4, 16, 16), 4),
    "pool-PW1-W6": ((2, 32, 4, 6, 6), 32), "pool-PW1-W2": ((1, 64, 2, 2, 2), 32), "pool-PW2-W4": ((2, 32, 2, 6, 4), 32),
}


@pytest.mark.parametrize("case", list(GN_POOL))
def test_groupnorm_apply_pool_form(ops, dev, case):
    """mphip_groupnorm_apply with pool2: gn_apply_pool_kernel<2> (W % 4 == 0, 16-byte x / y / residual) and <1> (W % 4 != 0 with even dims,
    or an unaligned pointer — never executed by the suite before).  Reference: float64 GroupNorm (+ residual, ReLU) then AvgPool3d."""
    shape, groups = GN_POOL[case]
    assert (shape[4] % 4 == 0) == ("PW2" in case)
    c = shape[1]
    x, res = R.seeded_tensor(shape, 1901, scale=2.0, shift=0.3), R.seeded_tensor(shape, 1902)
    g, b = R.seeded_tensor((c,), 1903, scale=0.25, shift=1.0), R.seeded_tensor((c,), 1904, scale=0.25)
    st = ops.groupnorm_stats(x.to(dev), groups)
    for with_res, relu in ((True, True), (False, False)):
        want, _ = _gn_forward64(x.double(), groups, g.double(), b.double(), None, None, res.double() if with_res else None, int(relu))
        want = F.avg_pool3d(want, 2, 2)
        got = ops.groupnorm_apply(x.to(dev), st, g.to(dev), b.to(dev), groups, residual=res.to(dev) if with_res else None, relu=relu, pool2=True)
        err = (got.cpu().double() - want).abs().max().item()
        print(f"{case} res={with_res}: max-abs {err:.2e}")     # worst measured: 1.9e-7
        assert err < 1e-5
        off = ops.groupnorm_apply(_offset_view(x, dev), st, g.to(dev), b.to(dev), groups, residual=_offset_view(res, dev) if with_res else None,
                                  relu=relu, pool2=True)
        assert torch.equal(off, got), f"{case}: the <1> kernel on an unaligned x differs from the aligned call"


# ================================================================== GroupNorm backward
GN_BWD = {   # shape, groups.  apply4 kernels: S % 4 == 0 and S >= 512 and 16-byte pointers; flat kernels otherwise
    "bwd-vec4-hot-16x64x64": ((1, 4, 16, 64, 64), 2), "bwd-vec4-hot-8x32x32": ((2, 8, 8, 32, 32), 4), "bwd-vec4-hot-4x16x16": ((2, 8, 4, 16, 16), 4),
    "bwd-flat-hot-2x8x8-S128": ((2, 16, 2, 8, 8), 4),
    "bwd-flat-S508": ((2, 64, 1, 4, 127), 32), "bwd-vec4-S512": ((2, 64, 2, 16, 16), 32), "bwd-vec4-S516": ((2, 64, 1, 4, 129), 32),
    "bwd-vec4-S1028-grid-tail": ((2, 64, 1, 4, 257), 32), "bwd-flat-S510-odd": ((1, 64, 2, 15, 17), 32),
}
MASK_MARGIN = 1e-5   # the suite's bar for the fp32 GroupNorm forward on O(1) data (asserted below before the mask is relied on)


def _gn_bwd_data(shape, groups, seed, res, act, affine2):
    """Inputs whose float64 pre-activation stays MASK_MARGIN away from 0 wherever a ReLU follows: the derivative of ReLU is discontinuous
    there, so an fp32 forward that lands on the other side of 0 is a property of the reference, not an error of the backward kernels.
    The seed walks until the data have that margin (a property of the data alone; the kernels are not consulted)."""
    c = shape[1]
    for s in range(seed, seed + 400, 10):
        x = R.seeded_tensor(shape, s, scale=2.0, shift=0.3)
        r = R.seeded_tensor(shape, s + 1) if res else None
        gamma, beta = R.seeded_tensor((c,), s + 2, shift=1.0), R.seeded_tensor((c,), s + 3)
        w2 = R.seeded_tensor((c,), s + 5, scale=0.25, shift=1.0) if affine2 else None
        b2 = R.seeded_tensor((c,), s + 6, scale=0.25) if affine2 else None
        dy = R.seeded_tensor(shape, s + 4)
        leaves = [t.double().requires_grad_(True) if t is not None else None for t in (x, gamma, beta, w2, b2, r)]
        y, u = _gn_forward64(leaves[0], groups, leaves[1], leaves[2], leaves[3], leaves[4], leaves[5], act)
        if act == 0 or u.detach().abs().min().item() > MASK_MARGIN:
            y.backward(dy.double())
            return dict(x=x, r=r, gamma=gamma, beta=beta, w2=w2, b2=b2, dy=dy, y64=y.detach(), grads=[None if t is None else t.grad for t in leaves])
    raise AssertionError("no seed with a clear ReLU mask")


def _gn_bwd_check(name, outs, grads, res, affine2):
    dx, dgamma, dbeta, dres = outs[:4]
    errs = {"dx": _rel_err(dx, grads[0]), "dgamma": _rel_err(dgamma, grads[1]), "dbeta": _rel_err(dbeta, grads[2])}
    if affine2:
        errs["dw2"], errs["db2"] = _rel_err(outs[4], grads[3]), _rel_err(outs[5], grads[4])
    if res:
        errs["dres"] = _rel_err(dres, grads[5])
    print(name, " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    # worst measured: dx 2.8e-7, dgamma 1.8e-7, dbeta 1.1e-7, dw2 2.9e-7, db2 9.6e-8, dres 0
    for k, v in errs.items():
        assert v < (1e-6 if k == "dres" else 1e-4), (name, k, v)


GN_BWD_VARIANTS = ["act0", "act1-res", "act1", "act2", "act1-res-adaptive", "act2-adaptive", "act0-adaptive"]
# every shape x variant through the two-launch entry; the three-launch pair (reduce, then _bwd_apply's own vector / flat choice) at the S edges
GN_BWD_CASES = [(c, v, "two-launch") for c in GN_BWD for v in GN_BWD_VARIANTS] + \
               [(c, v, "three-launch") for c in GN_BWD if "hot" not in c for v in ("act1-res", "act2-adaptive")]


@pytest.mark.parametrize("case,variant,launches", GN_BWD_CASES, ids=["-".join(t) for t in GN_BWD_CASES])
def test_groupnorm_bwd_branches(ops, dev, case, variant, launches, monkeypatch):
    """mphip_groupnorm_bwd (two launches) and mphip_groupnorm_bwd_reduce + _bwd_apply (three): the float4 kernels and the flat ones, with
    and without residual, act 0 / 1 / 2, with and without the second affine — against float64 autograd through F.group_norm (the vector
    kernels, which every G3d level runs, were only ever compared with the three-launch path that shares their code).  Then the same call
    on x / y / dy views that are not 16-byte aligned: the flat kernels chosen for alignment, bit-equal dx and dres, same bars."""
    shape, groups = GN_BWD[case]
    s = shape[2] * shape[3] * shape[4]
    assert ("vec4" in case) == (s % 4 == 0 and s >= 512)
    monkeypatch.setenv("MPHIP_GN_BWD_FUSED", "1" if launches == "two-launch" else "0")
    act = int(variant[3])
    res, affine2 = "res" in variant, "adaptive" in variant
    d = _gn_bwd_data(shape, groups, 2001, res, act, affine2)
    D = lambda t: None if t is None else t.to(dev)
    xg = D(d["x"])
    st = ops.groupnorm_stats(xg, groups, 1e-5)
    yg = ops.groupnorm_apply(xg, st, D(d["gamma"]), D(d["beta"]), groups, w2=D(d["w2"]), b2=D(d["b2"]), residual=D(d["r"]), relu=act >= 1,
                             tanh=act == 2)
    assert (yg.cpu().double() - d["y64"]).abs().max().item() < MASK_MARGIN
    run = lambda x_, y_, dy_: ops.groupnorm_bwd(x_, y_, dy_, st, D(d["gamma"]), groups, act, res, beta=D(d["beta"]) if affine2 else None,
                                                w2=D(d["w2"]))
    outs = run(xg, yg, D(d["dy"]))
    assert len(outs) == (6 if affine2 else 4) and (outs[3] is not None) == res
    _gn_bwd_check(f"{case} {variant} {launches}", outs, d["grads"], res, affine2)
    off = run(_offset_view(d["x"], dev), _offset_view(yg, dev), _offset_view(d["dy"], dev))
    _gn_bwd_check(f"{case} {variant} {launches} unaligned", off, d["grads"], res, affine2)
    assert torch.equal(off[0], outs[0]), "dx of the flat kernels (unaligned pointers) differs from the aligned call"
    if res:
        assert torch.equal(off[3], outs[3])


# ================================================================== casts
@pytest.mark.parametrize("n", [1, 3, 5, 7, 1023, 1026, 8197, 70001])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_cast_kernels_sizes_not_divisible(ops, dev, n, dtype):
    """mphip_cast_from_f32 / mphip_cast_to_f32_range on sizes that are not multiples of 4 / 8 (vector body plus tail; 70001: several
    workgroups plus a tail): torch's round-to-nearest-even .to(dtype), exact widening, and a range descriptor that holds max|x|."""
    x = R.seeded_tensor((n,), 2101, scale=300.0)
    x[0] = float("inf") if n > 3 else 65519.9        # (65519.9: rounds to the largest finite f16)
    x[-1] = -1e-30
    h = x.to(dtype)
    assert torch.equal(ops.cast_from_f32(x.to(dev), dtype).cpu().view(torch.int16), h.view(torch.int16))
    y = ops.cast_to_f32_range(h.to(dev))
    assert torch.equal(y.cpu(), h.float())
    rng = ops.tensor_range(y).cpu()
    parts = int(rng[3:4].view(torch.int32))
    assert 1 <= parts <= 4096
    assert rng[4:4 + parts].max().item() == h.float().abs().max().item()


# ================================================================== K2 on given coordinates
def test_warp_volume_on_given_coordinates_equals_k2(ops, dev):
    """mphip_warp_volume_coords (no Python caller, no test before): K2's gather on the coordinates of mphip_warp_coords is K2, bit for bit."""
    from megaportrait_hack_amd import _lib

    lib = _lib.load()
    b, c, d, h, w = 2, 5, 6, 10, 14
    v = R.seeded_tensor((b, c, d, h, w), 2201, scale=1.7).to(dev)
    field = (R.seeded_tensor((b, 3, 5, 7, 9), 2202, scale=6.0) + 4.0).to(dev)
    want = ops.warp_volume(v, field)
    coords = ops.warp_coords(field, d, h, w)
    out = torch.empty_like(v)
    ws_bytes = lib.mphip_warp_workspace_bytes(b, d, h, w)
    ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.float32, device=dev)
    _lib.check(lib.mphip_warp_volume_coords(ops._ptr(v), ops._ptr(coords), ops._ptr(out), None, b, c, d, h, w, ops._ptr(ws), ws_bytes,
                                            ops._stream()), "mphip_warp_volume_coords")
    assert torch.equal(out, want)
