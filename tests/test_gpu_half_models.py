"""Half models on the GPU: hot modules converted with .half() / .bfloat16() (include/mphip.h "model dtypes").

The oracle is the module's "fp32 twin": a deep copy whose parameters are `.float()` of the half ones, run under ops.half_products(True)
on the inputs cast to fp32, its output rounded with `.to(dtype)`.  A half model must be BITWISE equal to it — K2 widens the half
volume exactly, K3 rounds once at the store, and everything in between is the twin's own fp32 arithmetic."""
import copy

import pytest
import torch

from megaportrait_hack_amd import _lib, ops
from megaportrait_hack_amd import model as M

pytestmark = pytest.mark.gpu

HALF = (torch.float16, torch.bfloat16)
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.build()
    _lib.load()


def _twin(module):
    """deep copy whose parameters are .float() of the module's (caches — packs, plans, twins — are not copied)"""
    memo = {}
    for m in module.modules():
        for k, v in m.__dict__.items():
            if k.startswith("_") and k not in ("_parameters", "_buffers", "_modules") and isinstance(v, (dict, tuple)) and k not in vars(torch.nn.Module()):
                memo[id(v)] = {} if isinstance(v, dict) else None
        for p in m._parameters.values():
            if p is not None:
                memo[id(p)] = torch.nn.Parameter(p.detach().float(), requires_grad=False)
    return copy.deepcopy(module, memo)


def _twin_out(module, dtype, fn, *args):
    twin = _twin(module)
    with torch.no_grad(), ops.half_products(True):
        y = getattr(twin, fn)(*(a.float() if torch.is_tensor(a) and a.is_floating_point() else a for a in args))
    return y.to(dtype)


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb)
    assert torch.equal(a[~na], b[~nb])


def _hot_inputs(b, seed, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r3 = 3.0 ** 0.5

    def u(*shape, scale=r3):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(DEV)

    return dict(vs=u(b, 96, 16, 64, 64).to(dtype), es=u(b, 512), Rs=u(b, 3, scale=30.0), ts=u(b, 3, scale=0.17), zs=u(b, 512),
                Rd=u(b, 3, scale=30.0), td=u(b, 3, scale=0.17), zd=u(b, 512))


@pytest.fixture(scope="module")
def hot32():
    torch.manual_seed(3)
    return M.GbaseHotSlice().to(DEV).eval()


# ------------------------------------------------------------------ 1. full-size hot slice, plan and per-op paths
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("b", [2, 8])
def test_full_size_hot_slice_equals_rounded_twin(hot32, dtype, b):
    hot = copy.deepcopy(hot32).to(dtype)
    inp = _hot_inputs(b, 11 + b, dtype)
    want = _twin_out(hot, dtype, "forward", *inp.values())
    for use_plan in (True, False):
        hot.use_c_plan = use_plan
        with torch.no_grad():
            got = hot(**inp)
        assert got.dtype == dtype and got.shape == (b, 96, 64, 64)
        assert torch.isfinite(got.float()).all()
        _same_bits(got, want)


# ------------------------------------------------------------------ 2. K2 reads a typed source
def _fields(b, kind):
    """Warp fields [B,3,64,64,64] (x, y, z components).  A sample lands at (grid + field) clipped to the volume, so a component of
    value f moves the sample by about f voxels."""
    g = torch.Generator(device="cpu").manual_seed(17 + b)
    f = ((torch.rand(b, 3, 64, 64, 64, generator=g) - 0.5) * 2.0).to(DEV)   # the reference's fields: samples in the low corner
    if kind == "columns":      # smooth and travelling along x: boxes of moderate size -> the column walk
        f[:, 0] += torch.linspace(0, 50, 64, device=DEV).view(1, 1, 1, 64)
    elif kind == "direct":     # incoherent in all three axes: boxes like the whole volume -> the direct gather
        f = torch.rand(b, 3, 64, 64, 64, generator=g).to(DEV) * torch.tensor([62.0, 62.0, 14.0], device=DEV).view(1, 3, 1, 1, 1) + 1.0
    elif kind == "far_z":      # x, y in the low corner, z clipped to the far border (used with D = 6)
        f[:, 2] = 100.0
    return f


def _k2_marks(coords):
    """What warp_gather_kernel decides per 32 x 64 tile of a (frame, slice), recomputed from the sample coordinates [B,D,H,W,3]:
    0 = in the corner image, 1 = column walk (box <= 16384 voxels), 2 = direct gather."""
    b, d, h, w, _ = coords.shape
    fl = coords.floor().to(torch.int64).reshape(b, d, h // 32, 32, w // 64, 64, 3)
    lo, hi = fl.amin(dim=(3, 5)), fl.amax(dim=(3, 5))
    top = torch.tensor([w - 1, h - 1, d - 1], device=coords.device)
    ext = torch.minimum(hi + 1, top) - lo + 1
    corner = ((lo + ext) <= 6).all(dim=-1)
    size = ext.prod(dim=-1)
    return torch.where(corner, 0, torch.where(size <= 16384, 1, 2))


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("kind", ["corner", "columns", "direct"])
def test_k2_typed_source_equals_k2_on_widened_volume(dtype, b, kind):
    v = (torch.randn(b, 96, 16, 64, 64, device=DEV) * 2.0).to(dtype)
    field = _fields(b, kind)
    got, gc, gi = ops.warp_volume(v, field, return_coords=True)
    want, wc, wi = ops.warp_volume(v.float(), field, return_coords=True)
    assert got.dtype == torch.float32
    assert torch.equal(got, want) and torch.equal(gc, wc) and torch.equal(gi, wi)
    # the field exercises the kernel it is named after
    marks = _k2_marks(gc)
    want_mark = {"corner": 0, "columns": 1, "direct": 2}[kind]
    assert (marks == want_mark).float().mean().item() > 0.9, torch.bincount(marks.flatten(), minlength=3)
    # the range descriptor it notes is the one of the fp32 run: the conv that reads it scales the same way
    rg, rw = ops.tensor_range(got), ops.tensor_range(want)
    n = int(rw[3:4].view(torch.int32))
    assert torch.equal(rg[:4 + n], rw[:4 + n])


@pytest.mark.parametrize("dtype", HALF)
def test_k2_typed_source_on_a_six_voxel_axis_clipped_to_its_border(dtype):
    """D = 6, every z sample clipped to 5.0: each tile's clamped box lies in the corner image while its first sample does not pass
    the fp32 kernel's quick corner test (z < 5).  The typed gather must take the corner from the image for such tiles too."""
    b = 2
    v = (torch.randn(b, 96, 6, 64, 64, device=DEV) * 2.0).to(dtype)
    field = _fields(b, "far_z")
    got, gc, _ = ops.warp_volume(v, field, return_coords=True)
    want, _, _ = ops.warp_volume(v.float(), field, return_coords=True)
    first = gc[:, :, ::32, ::64, :]   # the first sample of every tile
    assert (first[..., 2] == 5.0).all() and (_k2_marks(gc) == 0).any()
    assert torch.equal(got, want)


# ------------------------------------------------------------------ 3. K3 writes a typed projection
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("shared", [False, True])
def test_k3_typed_output_equals_rounded_fp32(dtype, shared):
    b = 3
    v = torch.randn(1 if shared else b, 96, 16, 64, 64, device=DEV) * 40.0
    v[0, 0, :, :4, :4] = float("inf")
    v[0, 1, :, :4, :4] = float("nan")
    v[0, 2, :, :4, :4] = 7.0e4   # beyond the f16 range: rounds to Inf in fp16, stays finite in bf16
    field = _fields(b, "corner")
    got = ops.warp_volume_dsum(v, field, out_dtype=dtype)
    want = ops.warp_volume_dsum(v, field).to(dtype)
    assert got.dtype == dtype
    assert not torch.isfinite(want.float()).all()
    _same_bits(got, want)


def test_cast_kernels_match_torch():
    x = torch.randn(5, 96, 7, 9, device=DEV) * 3.0
    x[0, 0, 0, :4] = torch.tensor([float("inf"), -float("inf"), float("nan"), 1e-30])
    for dtype in HALF:
        h = x.to(dtype)
        _same_bits(ops.cast_from_f32(x, dtype), h)
        y = ops.cast_to_f32_range(h)
        _same_bits(y, h.float())
        # the descriptor's maximum is the one mphip_absmax_range measures on the widened tensor
        ref = ops.absmax_range(h.float().clone())
        n, m = int(ops.tensor_range(y)[3:4].view(torch.int32)), int(ref[3:4].view(torch.int32))
        assert ops.tensor_range(y)[4:4 + n].view(torch.int32).max() == ref[4:4 + m].view(torch.int32).max()


# ------------------------------------------------------------------ 4. single modules
def test_g3d_half_equals_twin():
    torch.manual_seed(5)
    g = M.G3d(96).to(DEV).half().eval()
    x = torch.randn(2, 96, 16, 32, 32, device=DEV).half()
    with torch.no_grad():
        got = g(x)
    assert got.dtype == torch.float16
    _same_bits(got, _twin_out(g, torch.float16, "forward", x))


def test_eapp3d_tail_bf16_equals_twin():
    torch.manual_seed(6)
    e = M.Eapp3DTail().to(DEV).bfloat16().eval()
    x = torch.randn(2, 1536, 32, 32, device=DEV).bfloat16()
    with torch.no_grad():
        got = e(x)
    assert got.dtype == torch.bfloat16 and got.shape == (2, 96, 16, 32, 32)
    _same_bits(got, _twin_out(e, torch.bfloat16, "forward", x))


def test_g2d_head_half_equals_twin():
    torch.manual_seed(7)
    h = M.G2dHead().to(DEV).half().eval()
    x = torch.randn(3, 96, 64, 64, device=DEV).half()
    with torch.no_grad():
        got = h(x)
    assert got.dtype == torch.float16 and got.shape == (3, 512, 64, 64)
    _same_bits(got, _twin_out(h, torch.float16, "forward", x))


@pytest.mark.parametrize("dtype", HALF)
def test_warp_generator_half_equals_twin(dtype):
    torch.manual_seed(8)
    wg = M.WarpGeneratorC2D(512).to(DEV).to(dtype).eval()
    b = 2
    R, t = torch.randn(b, 3, device=DEV) * 20, torch.randn(b, 3, device=DEV) * 0.1
    z, e = torch.randn(b, 512, device=DEV).to(dtype), torch.randn(b, 512, device=DEV).to(dtype)
    with torch.no_grad():
        got = wg(R, t, z, e)
    assert got.dtype == dtype
    _same_bits(got, _twin_out(wg, dtype, "forward", R, t, z, e))


@pytest.mark.parametrize("dtype", HALF)
def test_plan_g3d_typed_equals_rounded_fp32_entry(hot32, dtype):
    """mphip_g3d_forward_typed: a typed x is widened with its descriptor in one pass, y rounded once at the end."""
    from megaportrait_hack_amd import plan as P

    pl = P.HotSlicePlan(hot32, dims=(96, 8, 32, 32), g3d_only=True)
    x = (torch.randn(2, 96, 8, 32, 32, device=DEV) * 3.0).to(dtype)
    with torch.no_grad(), ops.half_products(True):
        got = pl.g3d_typed(x, dtype)
        want = pl.g3d(x.float()).to(dtype)
        got32 = pl.g3d_typed(x.float(), torch.float32)
    pl.close()
    assert got.dtype == dtype
    _same_bits(got, want)
    assert torch.equal(got32.to(dtype), want)


def test_half_model_follows_weight_updates(hot32):
    hot = copy.deepcopy(hot32).half()
    inp = _hot_inputs(1, 31, torch.float16)
    with torch.no_grad():
        hot(**inp)
        hot.G3d.final_conv.weight.mul_(0.5)   # in place: the shadow and its packs must follow
        got = hot(**inp)
    _same_bits(got, _twin_out(hot, torch.float16, "forward", *inp.values()))


# ------------------------------------------------------------------ 5. the whole generator
def test_gbase_half_forward_and_reenact_close_to_fp32():
    """Measured on MI355X over two runs: fp16 forward max-abs vs fp32 6.1e-3 - 6.5e-3, reenact 7.5e-3 - 8.8e-3 (images in (0,1));
    the bar is ~10x that."""
    from megaportrait_hack_amd import gbase

    torch.manual_seed(9)
    g32 = gbase.Gbase().to(DEV).eval()
    g16 = copy.deepcopy(g32).half()
    xs = torch.rand(1, 3, 512, 512, device=DEV)
    xd = torch.rand(2, 3, 512, 512, device=DEV)
    with torch.no_grad():
        y32, _ = g32(xs.expand(2, -1, -1, -1), xd)
        y16, pyr = g16(xs.half().expand(2, -1, -1, -1), xd.half())
        r32 = g32.reenact(xs, xd)
        r16 = g16.reenact(xs.half(), xd.half())
    assert y16.dtype == torch.float16 and torch.isfinite(y16).all() and torch.isfinite(r16).all()
    err_f = (y16.float() - y32).abs().max().item()
    err_r = (r16.float() - r32).abs().max().item()
    print(f"Gbase fp16 vs fp32: forward max-abs {err_f:.3e}, reenact max-abs {err_r:.3e}")
    assert err_f < 0.075 and err_r < 0.075


# ------------------------------------------------------------------ 6. graph replay
def test_graphed_half_hot_slice_replays_equal_to_eager(hot32):
    hot = copy.deepcopy(hot32).half()
    inp = _hot_inputs(2, 41, torch.float16)
    with torch.no_grad():
        eager = hot(**inp).clone()
    gh = M.GraphedHotSlice(hot, inp)
    out = gh(**inp)
    torch.cuda.synchronize()
    assert out.dtype == torch.float16
    _same_bits(out, eager)
    inp2 = _hot_inputs(2, 42, torch.float16)
    with torch.no_grad():
        eager2 = hot(**inp2).clone()
    _same_bits(gh(**inp2).clone(), eager2)


# ------------------------------------------------------------------ 7. errors
def test_training_a_half_module_raises():
    g = M.G3d(96).to(DEV).half()
    x = torch.randn(1, 96, 8, 16, 16, device=DEV).half()
    with pytest.raises(RuntimeError, match="keep fp32 parameters and use torch.autocast"):
        g(x)


def test_mixed_dtype_module_raises():
    hot = M.GbaseHotSlice().to(DEV).half()
    hot.G3d.final_conv.float()
    inp = _hot_inputs(1, 51, torch.float16)
    with torch.no_grad(), pytest.raises(RuntimeError, match="mix dtypes"):
        hot(**inp)


# ------------------------------------------------------------------ 8. the untyped warp entry points forward to the typed implementations
def _small_field(b, d, h, w, kind):
    g = torch.Generator(device="cpu").manual_seed(29)
    f = ((torch.rand(b, 3, d, h, w, generator=g) - 0.5) * 2.0).to(DEV)   # samples in the low corner (_fields)
    if kind == "travelling":   # samples spread over the whole volume
        f[:, 0] += torch.linspace(0, w - 1, w, device=DEV).view(1, 1, 1, w)
        f[:, 1] += torch.linspace(0, h - 1, h, device=DEV).view(1, 1, h, 1)
        f[:, 2] += torch.linspace(0, d - 1, d, device=DEV).view(1, d, 1, 1)
    return f


@pytest.mark.parametrize("kind", ["corner", "travelling"])
@pytest.mark.parametrize("w", [8, 6])   # (6: W % 4 != 0, the scalar fallback of mphip_warp_volume)
def test_untyped_warp_entries_equal_typed_entries_with_f32(kind, w):
    """Every forwarded pair: the `_typed` entry point given MPHIP_DTYPE_F32 writes exactly what the untyped entry point writes."""
    lib, P, S = _lib.load(), ops._ptr, ops._stream
    b, c, d, h = 2, 6, 4, 8
    f32 = ops.dtype_code(torch.float32)
    v = torch.randn(b, c, d, h, w, device=DEV) * 2.0
    field = _small_field(b, d, h, w, kind)
    tables = [ops.linspace_table(n, v.device) for n in (d, h, w)]
    lin = [P(t) for t in tables]
    img_bytes = lib.mphip_warp_corner_image_bytes(b, c)
    ws_bytes = lib.mphip_warp_workspace_bytes(b, d, h, w) + img_bytes
    new = lambda shape, fill, dtype=torch.float32: torch.full(shape, fill, dtype=dtype, device=DEV)   # (distinct fills: an unwritten result differs)

    def run(fn, typed, fill):   # mphip_warp_volume(_typed)
        out, coords, idx, rng = new(v.shape, fill), new((b, d, h, w, 3), fill), new((b, d, h, w, 3), int(fill), torch.int32), ops.new_range(v.device)
        ws = new((ws_bytes // 4,), 0.0)
        head = (P(v), f32) if typed else (P(v),)
        assert fn(*head, P(field), *lin, P(out), P(coords), P(idx), P(rng), b, c, d, h, w, d, h, w, P(ws), ws_bytes, S()) == 0, lib.mphip_last_error()
        n = int(rng[3:4].view(torch.int32))
        return out, coords, idx, rng[:4 + n].clone()

    plain, typed = run(lib.mphip_warp_volume, False, 1.0), run(lib.mphip_warp_volume_typed, True, 2.0)
    for x, y in zip(plain, typed):
        assert torch.equal(x, y)
    coords = plain[1]
    if w % 4 != 0:
        return   # (the entry points below need W % 4 == 0 or do not depend on W's path)
    # the corner image and K2 on given coordinates with it
    imgs = [new((img_bytes // 4,), 1.0), new((img_bytes // 4,), 2.0)]
    assert lib.mphip_warp_corner_image(P(v), P(imgs[0]), img_bytes, b, c, d, h, w, S()) == 0, lib.mphip_last_error()
    assert lib.mphip_warp_corner_image_typed(P(v), f32, P(imgs[1]), img_bytes, b, c, d, h, w, S()) == 0, lib.mphip_last_error()
    assert torch.equal(imgs[0], imgs[1])
    outs, ws = [new(v.shape, 1.0), new(v.shape, 2.0)], new((ws_bytes // 4,), 0.0)
    assert lib.mphip_warp_volume_coords_img(P(v), P(coords), P(outs[0]), None, b, c, d, h, w, P(ws), ws_bytes, P(imgs[0]), S()) == 0, lib.mphip_last_error()
    assert lib.mphip_warp_volume_coords_img_typed(P(v), f32, P(coords), P(outs[1]), None, b, c, d, h, w, P(ws), ws_bytes, P(imgs[0]), S()) == 0, lib.mphip_last_error()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], plain[0])
    # K3: on given coordinates, and with its own coordinate pass (own and shared source volume)
    for shared in (0, 1):
        src = v[:1].contiguous() if shared else v
        sums = [new((b, c, h, w), float(k)) for k in range(1, 5)]
        assert lib.mphip_warp_volume_dsum_coords(P(src), P(coords), P(sums[0]), b, c, d, h, w, shared, S()) == 0, lib.mphip_last_error()
        assert lib.mphip_warp_volume_dsum_coords_typed(P(src), P(coords), P(sums[1]), f32, b, c, d, h, w, shared, S()) == 0, lib.mphip_last_error()
        fn = lib.mphip_warp_volume_dsum_shared if shared else lib.mphip_warp_volume_dsum
        assert fn(P(src), P(field), *lin, P(sums[2]), b, c, d, h, w, d, h, w, P(ws), ws_bytes, S()) == 0, lib.mphip_last_error()
        assert lib.mphip_warp_volume_dsum_typed(P(src), shared, P(field), *lin, P(sums[3]), f32, b, c, d, h, w, d, h, w, P(ws), ws_bytes, S()) == 0, lib.mphip_last_error()
        assert torch.equal(sums[0], sums[1]) and torch.equal(sums[2], sums[3]) and torch.equal(sums[0], sums[2])
