"""G3d's first block finishes with gn_apply_pool_warp_kernel (csrc/warp.hip) in the hot-slice plan: GroupNorm + residual + ReLU + AvgPool3d(2)
with the residual — warp #1's output — rebuilt from K2's corner image wherever K2 served a (frame, 32 x 64 tile, slice) from it, and loaded
where it did not.  The launch promises the bits of gn_apply_pool_kernel<2>, so the bar everywhere is torch.equal: the plan against the
per-op Python schedule (which still runs the plain launch), and the plan with MPHIP_RESIDUAL_FROM_WARP=0 (the plain launch inside the plan).

Shapes are the smallest at which each branch of the kernel exists (D = 8: G3d pools three times):
  * 16 x 16: one partial tile per slice; K2 groups the 96 channels in blocks of 16 and the launch splits each block in two parts of 8;
  * 40 x 72: a full 32 x 64 tile, a partial one in w, a partial one in h and the corner tile that is partial in both;
  * B = 3: an odd number of frames (and of workgroups per XCD);
  * 16 x 64 x 64, B = 8: the benchmark's shape, the only one where the image is ONE block of 96 channels (two parts of 48);
  * a frame whose source field is pushed along z so that K2's marks differ from slice to slice: slice pairs that are rebuilt, pairs that are
    loaded, and pairs whose two slices disagree (loaded), all in one launch — asserted from the marks, recomputed here from the coordinates;
  * conv2's output at |mean| / sigma = 400 in every group: (y2 - mean) cancels nearly every bit, so a channel paired with another channel's
    statistics, or a sum in another order, is off by whole units."""
import pytest
import torch

from oracle import hotpath_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    from megaportrait_hack_amd import _lib, model

    _lib.load()
    return model


@pytest.fixture(scope="module")
def hot(M, dev):
    h = M.GbaseHotSlice()
    M.load_hot_state_dict(h, R.seeded_gbase_hot_state_dict(21))
    return h.to(dev).eval()


def _inputs(dev, b, d, h, w, seed=5):
    return {k: v.to(dev) for k, v in R.seeded_hot_inputs(b, seed, D=d, H=h, W=w).items()}


def _k2_marks(coords):
    """What warp_gather_kernel decides per (frame, slice, 32 x 64 tile) from the sample coordinates [B,D,H,W,3] (partial tiles included):
    0 = served from the corner image, 1 = column walk, 2 = direct gather."""
    b, d, h, w, _ = coords.shape
    fl = coords.floor().to(torch.int64)
    top = torch.tensor([w - 1, h - 1, d - 1], device=coords.device)
    out = torch.zeros(b, d, (h + 31) // 32, (w + 63) // 64, dtype=torch.int64)
    for i in range(out.shape[2]):
        for j in range(out.shape[3]):
            t = fl[:, :, i * 32:(i + 1) * 32, j * 64:(j + 1) * 64]
            lo, hi = t.amin(dim=(2, 3)), t.amax(dim=(2, 3))
            ext = torch.minimum(hi + 1, top) - lo + 1
            corner = ((lo + ext) <= 6).all(dim=-1)
            out[:, :, i, j] = torch.where(corner, 0, torch.where(ext.prod(dim=-1) <= 16384, 1, 2)).cpu()
    return out


def _s2c_marks(hot, inp, d, h, w):
    from megaportrait_hack_amd import ops

    with torch.no_grad():
        field = hot.warp_generator_s2c(inp["Rs"], inp["ts"], inp["zs"], inp["es"])
        return _k2_marks(ops.warp_coords(field, d, h, w))


def _pairs(marks):
    """per (frame, slice pair, tile): both slices from the corner (rebuilt) / the two slices disagree / neither from the corner"""
    a, b = marks[:, 0::2], marks[:, 1::2]
    return int(((a == 0) & (b == 0)).sum()), int(((a == 0) != (b == 0)).sum()), int(((a != 0) & (b != 0)).sum())


def _plan_python_off(hot, inp, dims, monkeypatch, poison=False):
    """the plan (new launch), the per-op schedule, the plan with the switch off; the plan's workspace is exactly what its query asks for
    (HotSlicePlan allocates that and no more, and a real pass that outgrew the dry pass fails with a workspace error)"""
    from megaportrait_hack_amd import plan as P

    monkeypatch.delenv("MPHIP_RESIDUAL_FROM_WARP", raising=False)
    b = inp["vs"].shape[0]
    with torch.no_grad():
        want = hot._run_python(check_shape=False, **inp)
        pl = P.HotSlicePlan(hot, dims=dims)
        nbytes = pl.lib.mphip_hot_slice_workspace_bytes(pl._handle, b)
        ws = pl._workspace("slice", b, nbytes)
        assert ws.numel() == nbytes
        if poison:   # nothing may be read that the step did not write: the kept coordinates, marks and image included
            ws.view(torch.float32)[: nbytes // 4].fill_(float("nan"))
        got = pl(**inp).clone()
        again = pl(**inp).clone()
        monkeypatch.setenv("MPHIP_RESIDUAL_FROM_WARP", "0")
        off = pl(**inp).clone()           # same plan, same workspace: the arena does not depend on the switch
        off_fresh = P.HotSlicePlan(hot, dims=dims)(**inp).clone()
        monkeypatch.delenv("MPHIP_RESIDUAL_FROM_WARP")
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want) and torch.equal(again, want)
    assert torch.equal(off, want) and torch.equal(off_fresh, want)
    return got


@pytest.mark.parametrize("shape", [(1, 8, 16, 16), (2, 8, 40, 72), (3, 8, 16, 16)])
def test_plan_equals_python_schedule_and_the_plain_launch(hot, dev, monkeypatch, shape):
    b, d, h, w = shape
    inp = _inputs(dev, b, d, h, w)
    assert _pairs(_s2c_marks(hot, inp, d, h, w))[1:] == (0, 0)   # the model's own fields: every tile from the corner, every pair rebuilt
    _plan_python_off(hot, inp, (96, d, h, w), monkeypatch)


def test_rebuilt_and_loaded_residuals_in_one_launch(hot, dev, monkeypatch):
    """Frame 1 of 3: no rotation, pushed five voxels along z.  Its low slices still sample the corner, its high slices do not, and the border
    falls inside a slice pair; frames 0 and 2 stay in the corner."""
    b, d, h, w = 3, 8, 40, 72
    inp = _inputs(dev, b, d, h, w)
    inp["Rs"][1] = 0.0
    inp["ts"][1] = torch.tensor([0.0, 0.0, -5.0], device=dev)
    marks = _s2c_marks(hot, inp, d, h, w)
    rebuilt, disagree, loaded = _pairs(marks)
    assert rebuilt > 0 and disagree > 0 and loaded > 0, (rebuilt, disagree, loaded)
    assert _pairs(marks[1:2])[1] > 0 and _pairs(marks[1:2])[0] > 0   # ... within the one frame
    assert _pairs(marks[0:1])[1:] == (0, 0) and _pairs(marks[2:3])[1:] == (0, 0)
    _plan_python_off(hot, inp, (96, d, h, w), monkeypatch, poison=True)


def test_benchmark_shape_one_image_block(hot, dev, monkeypatch):
    b, d, h, w = 8, 16, 64, 64
    g = torch.Generator(device="cpu").manual_seed(29)
    r3 = 3.0 ** 0.5

    def u(*shape, scale=r3):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(dev)

    inp = dict(vs=u(b, 96, d, h, w), es=u(b, 512), Rs=u(b, 3, scale=30.0), ts=u(b, 3, scale=0.17), zs=u(b, 512), Rd=u(b, 3, scale=30.0),
               td=u(b, 3, scale=0.17), zd=u(b, 512))
    assert _pairs(_s2c_marks(hot, inp, d, h, w))[1:] == (0, 0)
    _plan_python_off(hot, inp, (96, d, h, w), monkeypatch)


def test_groupnorm_input_at_400_sigma(M, dev, monkeypatch):
    import copy

    import torch.nn.functional as F

    b, d, h, w = 1, 8, 16, 16
    hot = M.GbaseHotSlice()
    M.load_hot_state_dict(hot, R.seeded_gbase_hot_state_dict(21))
    hot = hot.to(dev).eval()
    inp = _inputs(dev, b, d, h, w)
    blk = hot.G3d.downsampling[0]
    with torch.no_grad():
        # conv2's output on the CPU (fp64), then a DC per group that puts its mean at 400 sigma
        vc = M.apply_warping_field(inp["vs"], hot.warp_generator_s2c(inp["Rs"], inp["ts"], inp["zs"], inp["es"])).cpu().double()
        cpu = copy.deepcopy(blk).cpu().double()
        y2 = cpu.conv2(F.relu(cpu.gn1(cpu.conv1(vc))))
        grp = y2.view(b, 32, -1)
        dc = (400.0 * grp.std(dim=-1, unbiased=False) - grp.mean(dim=-1))[0]            # [32]
        blk.conv2.bias.add_(dc.repeat_interleave(3).float().to(dev))
        grp = (y2 + dc.repeat_interleave(3).view(1, 96, 1, 1, 1)).view(b, 32, -1)
        ratio = grp.mean(dim=-1).abs() / grp.std(dim=-1, unbiased=False)
    assert float(ratio.min()) > 390.0 and float(ratio.max()) < 410.0
    _plan_python_off(hot, inp, (96, d, h, w), monkeypatch)
