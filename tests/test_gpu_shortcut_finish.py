"""The 1x1x1 shortcut conv of a ResBlock3D that finishes its block (mphip_conv3d_k1_gn_res_fwd, csrc/conv3d_f16x3.hip): GroupNorm 2, the
residual add, ReLU and the AvgPool3d(2) that follows run in the k = 1 kernel's epilogue, and the residual tensor is never written.

Every fused launch evaluates the expressions of the two launches it replaces (the conv's `acc * unscale + bias`, then norm.hip's gn_value
with that as the residual; the pooled form adds a cell's eight values in gn_apply_pool_kernel's order), so the bar is torch.equal on the
output and equality of the maximum the range descriptor folds to (the next conv's operand scale is derived from it) — at the kernel, at a
block and at the whole hot slice, against the old sequence (MPHIP_SHORTCUT_FINISH=0, read by the library at every query).

Which instantiation a case reaches follows f16x3_k1_ksplit / f16x3_k1_geometry (csrc/conv3d_f16x3.hip); where the default rule sends a
listed shape elsewhere the project's per-call switches (MPHIP_F16X3_K1_MIN, MPHIP_F16X3_K1_KS) route it, as noted per case."""
import math

import pytest
import torch

from oracle import hotpath_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from megaportrait_hack_amd import _lib, ops

    _lib.load()
    return ops


@pytest.fixture(scope="module")
def M():
    from megaportrait_hack_amd import _lib, model

    _lib.load()
    return model


def _range_max(rng: torch.Tensor) -> float:
    """max|tensor| a derive-mode range descriptor folds to: [2] and the [3] per-workgroup partial maxima behind it"""
    r = rng.cpu()
    assert r[0].item() == 0.0 and r[1].item() == 0.0, "not a derive-mode descriptor"
    n = int(r.view(torch.int32)[3].item())
    assert 0 < n <= 4096
    return max(r[2].item(), r[4:4 + n].max().item())


def _scale_exponent(m: float) -> int:
    """scale_from_bits (csrc/mphip_common.h): the power of two with m * 2^e < 2^14"""
    return min(max(14 - math.frexp(m)[1], -120), 120) if 0.0 < m < 3.0e38 else 0


def _supported(ops, n, ci, co, d, h, w, pool):
    return ops._lib.load().mphip_conv3d_k1_gn_res_supported(n, ci, co, d, h, w, 32, int(pool))


def _kernel_case(ops, dev, n, ci, co, d, h, w, pool, seed, dc=0.0):
    """fused entry vs conv3d(k = 1) + groupnorm_apply(residual=...) on the same y2 and statistics"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((n, ci, d, h, w), generator=g) * 1.7).to(dev)
    y2 = (torch.randn((n, co, d, h, w), generator=g) * 0.8 + dc).to(dev)
    wt = (torch.randn((co, ci, 1, 1, 1), generator=g) / ci ** 0.5).to(dev)
    bias = (torch.randn((co,), generator=g) * 0.3).to(dev)
    gamma = (1.0 + 0.2 * torch.randn((co,), generator=g)).to(dev)
    beta = (0.1 * torch.randn((co,), generator=g)).to(dev)
    pc = ops.PackedConv(wt, bias)
    st = ops.groupnorm_stats(y2, 32)
    assert ops._lib.load().mphip_conv3d_supported(n, ci, co, d, h, w, 1, 1) == 1
    assert _supported(ops, n, ci, co, d, h, w, pool) == 1 and ops.conv3d_k1_gn_res_ok(x.shape, pc, 32, pool)
    ops.f16x3_saturation_count(reset=True)
    identity = ops.conv3d(x, pc, precision=1)
    want = ops.groupnorm_apply(y2, st, gamma, beta, 32, residual=identity, relu=True, pool2=pool)
    got = ops.conv3d_k1_gn_res(x, pc, y2, st, gamma, beta, 32, relu=True, pool2=pool)
    assert got.shape == want.shape == ((n, co, d // 2, h // 2, w // 2) if pool else (n, co, d, h, w))
    assert torch.equal(got, want)
    m_got, m_want = _range_max(ops.tensor_range(got)), _range_max(ops.tensor_range(want))
    assert m_got == m_want == want.abs().max().item()
    assert _scale_exponent(m_got) == _scale_exponent(m_want)
    assert ops.f16x3_saturation_count() == 0
    # ... and without the ReLU (the sign of the sum survives: a wrong residual cannot hide behind the clamp)
    want = ops.groupnorm_apply(y2, st, gamma, beta, 32, residual=identity, relu=False, pool2=pool)
    got = ops.conv3d_k1_gn_res(x, pc, y2, st, gamma, beta, 32, relu=False, pool2=pool)
    assert torch.equal(got, want) and _range_max(ops.tensor_range(got)) == _range_max(ops.tensor_range(want))
    return st


# (N, Ci, Co, D, H, W, pooled forms, switches).  Wave tiles = N*D*H*W/64 * Co/96, chunks = Ci/16:
KERNEL_CASES = {
    # 4 wave tiles, 24 chunks -> eight waves share a tile; 256 voxels are below the k = 1 kernel's default floor of 1024
    "KS8": (2, 384, 96, 2, 8, 8, (False,), {"MPHIP_F16X3_K1_MIN": "64"}),
    # 32 wave tiles, 12 chunks -> four waves share a tile; W = 16: one brick per row pair
    "KS4": (2, 192, 96, 4, 16, 16, (False, True), {}),
    # 2048 wave tiles -> one tile per wave, two column tiles (512 workgroups)
    "KS1_NT2": (8, 96, 192, 8, 32, 32, (False, True), {}),
    # 512 wave tiles with 12 chunks would share tiles four ways: the switch gives each wave its own, <= 1024 -> one column tile
    "KS1_NT1": (4, 192, 96, 8, 32, 32, (False,), {"MPHIP_F16X3_K1_KS": "1"}),
    # N = 3, one column tile: 6 tiles on two workgroups, the last one half filled
    "N3_NT1_partial": (3, 96, 192, 2, 2, 16, (False,), {"MPHIP_F16X3_K1_MIN": "64"}),
    # N = 3, two column tiles: 513 waves (1026 wave tiles) on 129 workgroups, one live wave in the last; 19 x 9 bricks per plane pair
    "N3_NT2_partial": (3, 96, 192, 2, 38, 144, (False, True), {}),
}


@pytest.mark.parametrize("case", sorted(KERNEL_CASES))
def test_fused_entry_equals_conv_then_apply(ops, dev, monkeypatch, case):
    n, ci, co, d, h, w, pools, env = KERNEL_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for pool in pools:
        _kernel_case(ops, dev, n, ci, co, d, h, w, pool, seed=900 + len(case))


@pytest.mark.parametrize("pool", [False, True])
def test_fused_entry_at_a_large_mean_to_sigma_ratio(ops, dev, pool):
    """conv2's output with a DC of 400 sigma: (y2 - mean) cancels almost every bit of y2, so an epilogue that paired an element with
    another group's (mean, rstd), or read them in another order, is off by whole units"""
    st = _kernel_case(ops, dev, 2, 192, 96, 4, 16, 16, pool, seed=977, dc=320.0)
    mean, rstd = st.cpu().view(2, 32, 2).unbind(-1)
    assert float((mean.abs() * rstd).min()) > 300.0


def test_query_refuses_what_the_kernel_does_not_cover(ops, monkeypatch):
    lib = ops._lib.load()
    assert _supported(ops, 8, 96, 192, 8, 32, 32, True) == 1 and _supported(ops, 8, 96, 192, 8, 32, 32, False) == 1
    assert _supported(ops, 8, 96, 192, 8, 31, 32, True) == 0       # an odd H under pooling
    assert _supported(ops, 16, 96, 192, 16, 32, 8, True) == 0      # W = 8: no 16-wide brick ...
    assert _supported(ops, 16, 96, 192, 16, 32, 8, False) == 1     # ... the plain form does not care
    assert _supported(ops, 4, 96, 192, 8, 32, 32, True) == 0       # 1024 wave tiles: one column tile per wave, nothing to pair
    assert _supported(ops, 1, 16, 96, 2, 512, 1032, False) == 0    # 16512 waves on 4128 workgroups > the descriptor's 4096 partial maxima
    assert _supported(ops, 1, 16, 96, 2, 512, 1024, False) == 1    # 4096 workgroups
    assert _supported(ops, 8, 96, 192, 8, 32, 32, False) == 1 and lib.mphip_conv3d_supported(8, 96, 100, 8, 32, 32, 1, 1) == 0
    assert _supported(ops, 8, 96, 100, 8, 32, 32, False) == 0      # not a shape of the k = 1 f16x3 kernel
    one = torch.zeros(1).data_ptr()
    assert lib.mphip_conv3d_k1_gn_res_fwd(one, one, one, None, one, one, one, one, one, None, 16, 96, 192, 16, 32, 8, 32, 1, 1, None) == -1
    assert b"not fused" in lib.mphip_last_error()                  # (argument checks return before any launch)
    assert lib.mphip_conv3d_k1_gn_res_fwd(None, one, one, None, one, one, one, one, one, None, 8, 96, 192, 8, 32, 32, 32, 1, 0, None) == -1
    monkeypatch.setenv("MPHIP_SHORTCUT_FINISH", "0")
    assert _supported(ops, 8, 96, 192, 8, 32, 32, True) == 0


def _block(M, dev, ci, co, seed):
    torch.manual_seed(seed)
    blk = M.ResBlock3D(ci, co)
    with torch.no_grad():
        for gn in (blk.gn1, blk.gn2):
            gn.weight.add_(0.2 * torch.randn_like(gn.weight))
            gn.bias.add_(0.1 * torch.randn_like(gn.bias))
    return blk.to(dev).eval()


def _count_fused(ops, monkeypatch):
    calls = []
    real = ops.conv3d_k1_gn_res
    monkeypatch.setattr(ops, "conv3d_k1_gn_res", lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


# (Ci, Co, N, D, H, W, pool after, fused?)
BLOCK_CASES = {
    "fused_pooled": (192, 384, 2, 4, 16, 16, True, True),
    "fused_plain": (192, 96, 4, 4, 16, 16, False, True),
    "W8_pooled_falls_back": (192, 384, 2, 8, 16, 8, True, False),
    "grid_above_the_descriptor_falls_back": (16, 96, 1, 2, 512, 1032, False, False),
}


@pytest.mark.parametrize("case", sorted(BLOCK_CASES))
def test_block_equals_the_old_sequence(ops, M, dev, monkeypatch, case):
    """ResBlock3D._forward (the per-op schedule): fused where the query says yes, today's sequence where it says no, the same bits as
    the old sequence (MPHIP_SHORTCUT_FINISH=0) either way"""
    ci, co, n, d, h, w, pool, fused = BLOCK_CASES[case]
    blk = _block(M, dev, ci, co, 31)
    x = (torch.randn((n, ci, d, h, w), generator=torch.Generator().manual_seed(32)) * 1.3).to(dev)
    calls = _count_fused(ops, monkeypatch)
    with torch.no_grad():
        got = blk(x, _pool_after=pool)
        assert len(calls) == (1 if fused else 0)
        monkeypatch.setenv("MPHIP_SHORTCUT_FINISH", "0")
        want = blk(x, _pool_after=pool)
        assert len(calls) == (1 if fused else 0)
    assert torch.equal(got, want)
    assert _range_max(ops.tensor_range(got)) == _range_max(ops.tensor_range(want))


# The two small slices: their shortcut convs see fewer than 1024 voxels, or conv2 leaves split-K slabs — every block takes today's sequence
# (the fallback inside the plan and the per-op schedule).  Two frames of the full-size slice: the rule fuses down[2] (pooled, four waves per
# tile), up[1] and up[2] and leaves down[1] alone (one column tile per wave under a pool); with the k = 1 kernel's floor lowered also
# down[3] and up[0] (eight waves per tile).
SLICE_CASES = {
    "2x8x16x16": ((2, 8, 16, 16), {}, 0),
    "1x16x16x16": ((1, 16, 16, 16), {}, 0),
    "2x16x64x64": ((2, 16, 64, 64), {}, 3),
    "2x16x64x64_floor64": ((2, 16, 64, 64), {"MPHIP_F16X3_K1_MIN": "64"}, 5),
}


@pytest.mark.parametrize("case", sorted(SLICE_CASES))
def test_slice_plan_and_python_schedule_equal_the_old_sequence(ops, M, dev, monkeypatch, case):
    from megaportrait_hack_amd import plan as P

    (b, d, h, w), env, fuses = SLICE_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    hot = M.GbaseHotSlice()
    M.load_hot_state_dict(hot, R.seeded_gbase_hot_state_dict(21))
    hot = hot.to(dev).eval()
    inp = {k: v.to(dev) for k, v in R.seeded_hot_inputs(b, 5, D=d, H=h, W=w).items()}
    calls = _count_fused(ops, monkeypatch)
    ops.f16x3_saturation_count(reset=True)
    with torch.no_grad():
        py_on = hot._run_python(check_shape=False, **inp)
        assert len(calls) == fuses
        plan_on = P.HotSlicePlan(hot, dims=(96, d, h, w))(**inp).clone()
        monkeypatch.setenv("MPHIP_SHORTCUT_FINISH", "0")
        n_on = len(calls)
        py_off = hot._run_python(check_shape=False, **inp)
        assert len(calls) == n_on
        plan_off = P.HotSlicePlan(hot, dims=(96, d, h, w))(**inp).clone()   # (a new plan: its workspace is sized for its own schedule)
    assert ops.f16x3_saturation_count() == 0 and bool(torch.isfinite(plan_on).all())
    assert torch.equal(plan_on, plan_off)
    assert torch.equal(plan_on, py_on)
    assert torch.equal(py_on, py_off)
