"""The 2-D 3x3 convs with a bilinear x2 up-sample folded in (csrc/conv2d_up2_f16x3.hip: ops.conv2d_up2, ops.conv2d_resup2) and the fused
stage built on them (model.Up2ResBlock2DFused, native_body(fuse_upsample=True)).

The kernels are pinned bit for bit: with the SAME range descriptor of the low-resolution x, conv2d_up2(x) is conv2d(up2_reference(x))
and conv2d_resup2(x, r) is conv2d(x, residual=up2_reference(r)), outputs and output descriptors alike (model.up2_reference states the
up-sample as separate fp32 torch operations).  Shapes (h, w): (1,1) one pixel, (5,7) inside one tile, (8,8) exactly one tile, (9,11)
ragged across tiles, (17,9) three tile rows and a patch clamped at the map's edge.

The stage commutes the 1x1 shortcut with the up-sample, which changes the rounding order: it is held to the project's rule for that,
e_hip <= 4 * e_torch + 2^-22 * max|y64| against the unswapped modules in fp64 on the CPU (e_torch: the same modules in fp32 on the GPU).
Each pair is printed (lines starting with `conv2d_up2_parity`, run with -s) and, when MPHIP_PARITY_OUT names a file, appended there:
profiles/conv2d_up2_parity.json holds one MI355X run's pairs."""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1), (5, 7), (8, 8), (9, 11), (17, 9)]
SCALES = [1.0, 2.0 ** -20, 2.0 ** 20]
EPILOGUES = [(False, False), (True, False), (False, True), (True, True)]      # (relu, full-size residual)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _descriptor(t):
    """The descriptor a conv left on its output: header and the partial maxima in use, as integers."""
    from megaportrait_hack_amd import ops

    r = ops.tensor_range(t).view(torch.int32)
    return r[:4 + int(r[3].item())].clone()


def _pack(ci, co, seed):
    from megaportrait_hack_amd import ops

    return ops.PackedConv2d(_rand((co, ci, 3, 3), seed, 0.1).to(DEV), _rand((co,), seed + 1).to(DEV))


@pytest.mark.parametrize("hw", SHAPES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("co", [32, 96])
@pytest.mark.parametrize("ci", [16, 48])
def test_upsampled_source_is_bitwise(ci, co, hw):
    from megaportrait_hack_amd import model as M, ops

    h, w = hw
    assert ops.conv2d_up2_supported(2, ci, co, h, w)
    pack = _pack(ci, co, 10)
    x0, res0 = _rand((2, ci, h, w), 1), _rand((2, co, 2 * h, 2 * w), 2)
    ops.f16x3_saturation_count(reset=True)
    for scale in SCALES:
        x, res = (x0 * scale).to(DEV), (res0 * scale).to(DEV)
        r = ops.absmax_range(x.clone())                         # of the LOW-resolution map, for both sides
        up = M.up2_reference(x)
        assert tuple(up.shape) == (2, ci, 2 * h, 2 * w)
        for relu, with_res in EPILOGUES:
            kw = dict(residual=res if with_res else None, relu=relu, x_range=r, want_range=True)
            got = ops.conv2d_up2(x, pack, **kw)
            want = ops.conv2d(up, pack, **kw)
            assert got.shape == want.shape and torch.equal(got, want), (scale, relu, with_res, (got - want).abs().max().item())
            assert torch.equal(_descriptor(got), _descriptor(want))
            again = ops.conv2d_up2(x, pack, **kw)
            assert torch.equal(again, got) and torch.equal(_descriptor(again), _descriptor(got))
            assert torch.isfinite(got).all() and got.abs().max() > 0
    assert ops.f16x3_saturation_count() == 0


@pytest.mark.parametrize("hw", SHAPES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("co", [32, 96])
@pytest.mark.parametrize("ci", [16, 48])
def test_upsampled_residual_is_bitwise(ci, co, hw):
    from megaportrait_hack_amd import model as M, ops

    h, w = hw
    pack = _pack(ci, co, 20)
    x0, low0 = _rand((2, ci, 2 * h, 2 * w), 3), _rand((2, co, h, w), 4)
    ops.f16x3_saturation_count(reset=True)
    for scale in SCALES:
        x, low = (x0 * scale).to(DEV), (low0 * scale).to(DEV)
        r = ops.absmax_range(x.clone())
        up = M.up2_reference(low)
        for relu in (False, True):
            got = ops.conv2d_resup2(x, pack, low, relu=relu, x_range=r, want_range=True)
            want = ops.conv2d(x, pack, residual=up, relu=relu, x_range=r, want_range=True)
            assert got.shape == want.shape and torch.equal(got, want), (scale, relu, (got - want).abs().max().item())
            assert torch.equal(_descriptor(got), _descriptor(want))
            again = ops.conv2d_resup2(x, pack, low, relu=relu, x_range=r, want_range=True)
            assert torch.equal(again, got) and torch.equal(_descriptor(again), _descriptor(got))
            assert not torch.equal(got, ops.conv2d(x, pack, relu=relu, x_range=r))          # the residual arrived
    assert ops.f16x3_saturation_count() == 0


def test_without_a_descriptor_the_library_scans_the_low_resolution_map():
    from megaportrait_hack_amd import ops

    pack = _pack(48, 96, 30)
    x, low = _rand((2, 48, 9, 11), 5).to(DEV), _rand((2, 96, 9, 11), 6).to(DEV)
    assert ops.current_range(x) is None
    got = ops.conv2d_up2(x, pack, relu=True)
    assert ops.current_range(x) is None                                                 # (nothing was tagged: the library scanned)
    assert torch.equal(got, ops.conv2d_up2(x, pack, relu=True, x_range=ops.absmax_range(x.clone())))
    x2 = _rand((2, 48, 18, 22), 7).to(DEV)
    got = ops.conv2d_resup2(x2, pack, low, relu=True)
    assert torch.equal(got, ops.conv2d_resup2(x2, pack, low, relu=True, x_range=ops.absmax_range(x2.clone())))
    # a descriptor its producer left on x is picked up: same bits again
    y = ops.conv2d(_rand((2, 48, 9, 11), 8).to(DEV), pack, want_range=True)                 # [2,96,9,11]
    assert ops.current_range(y) is not None
    pack2 = _pack(96, 32, 31)
    assert torch.equal(ops.conv2d_up2(y, pack2), ops.conv2d_up2(y.clone(), pack2))


def test_python_entries_refuse_what_the_kernels_do_not_take():
    from megaportrait_hack_amd import ops

    pack = _pack(16, 32, 40)
    x = _rand((1, 16, 5, 7), 9).to(DEV)
    for bad in (lambda: ops.conv2d_up2(x[:, :8], pack), lambda: ops.conv2d_up2(x.half(), pack),
                lambda: ops.conv2d_up2(x, pack, residual=torch.zeros(1, 32, 5, 7, device=DEV)),
                lambda: ops.conv2d_resup2(x, pack, torch.zeros(1, 32, 2, 3, device=DEV)),                       # odd H and W
                lambda: ops.conv2d_resup2(x[:, :, :4, :6].contiguous(), pack, torch.zeros(1, 32, 4, 6, device=DEV)),   # a full-size residual
                lambda: ops.conv2d_resup2(x[:, :, :4, :6].contiguous(), pack, None)):
        with pytest.raises(RuntimeError):
            bad()


# ---------------------------------------------------------------------------------------------------------------- stage and body
def _seed(module, seed):
    """Parameters as initialised; BatchNorm statistics and affine moved away from their initial values."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)      # [0.5, 1.5]
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.5)
    return module


def _check(name, y_hip, y_torch, y64):
    e_hip = (y_hip.cpu().double() - y64).abs().max().item()
    e_torch = (y_torch.cpu().double() - y64).abs().max().item()
    top = y64.abs().max().item()
    bound = 4 * e_torch + 2.0 ** -22 * top
    line = {"case": name, "e_hip": e_hip, "e_torch": e_torch, "max_abs_y64": top, "bound": bound}
    print("conv2d_up2_parity " + json.dumps(line))
    out = os.environ.get("MPHIP_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")
    assert e_hip <= bound, (name, e_hip, bound)


def _up():
    return nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)


@pytest.mark.parametrize("ci,co,h,w", [(32, 64, 9, 11), (512, 256, 8, 8)])
def test_fused_stage_against_fp64(ci, co, h, w):
    from megaportrait_hack_amd import encoders2d as E, model as M, ops

    torch.manual_seed(ci + h)
    seq = _seed(nn.Sequential(_up(), E.ResBlock2D(ci, co)), 1).eval()
    x = torch.randn(2, ci, h, w)
    with torch.no_grad():
        y64 = copy.deepcopy(seq).double()(x.double())
        gpu = seq.to(DEV)
        y_torch = gpu(x.to(DEV))
        stage = M.Up2ResBlock2DFused.from_sequential(gpu)
        assert stage[0] is gpu[0] and isinstance(stage[1], M.ResBlock2DFused) and stage[1].conv1 is gpu[1].conv1
        assert list(stage.state_dict().keys()) == list(gpu.state_dict().keys())
        ops.f16x3_saturation_count(reset=True)
        assert stage._native_ok(x.to(DEV))
        y_hip = stage(x.to(DEV))
        assert "_mphip_fold" in stage[1].__dict__ and ops.tensor_range(y_hip) is not None
        assert y_hip.dtype == torch.float32 and y_hip.is_contiguous() and tuple(y_hip.shape) == (2, co, 2 * h, 2 * w)
        _check(f"stage {ci}->{co} {h}x{w}", y_hip, y_torch, y64)
        assert torch.equal(stage(x.to(DEV)), y_hip)                                                 # same bits twice
        assert torch.equal(stage(x.to(DEV).contiguous(memory_format=torch.channels_last)), y_hip)   # NHWC input: copied once
    assert ops.f16x3_saturation_count() == 0


def test_whole_g2d_with_fused_upsamples_against_fp64():
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(7)
    g2d = _seed(E.G2d(), 2).eval()
    x = torch.randn(1, 96, 8, 8)
    with torch.no_grad():
        g64 = copy.deepcopy(g2d).double()       # (the head's forward is HIP only: its two 1x1 convs in fp64 by hand, then the body)
        y64 = g64.body(F.conv2d(F.conv2d(x.double(), g64.reshape.weight, g64.reshape.bias), g64.conv1x1.weight, g64.conv1x1.bias))
        g2d = g2d.to(DEV)
        x = x.to(DEV)
        y_torch = g2d(x).clone()
        keys = list(g2d.state_dict().keys())
        slots = lambda: [g2d.upsample1, g2d.upsample2, g2d.upsample3, g2d.upsample1[0], g2d.upsample1[1], g2d.upsample2[1],
                         g2d.upsample3[1], g2d.final_conv] + list(g2d.res_blocks)
        originals = slots()
        try:
            assert g2d.native_body(fuse_upsample=True) is g2d
            assert all(isinstance(s, M.Up2ResBlock2DFused) for s in (g2d.upsample1, g2d.upsample2, g2d.upsample3))
            assert all(s._native_ok(torch.empty(1, s[1].conv1.in_channels, 8, 8, device=DEV)) for s in (g2d.upsample1, g2d.upsample2))
            assert list(g2d.state_dict().keys()) == keys
            _check("G2d native_body(fuse_upsample=True)", g2d(x), y_torch, y64)
            g2d.native_final_conv()
            _check("G2d native_body(fuse_upsample=True) + native_final_conv", g2d(x), y_torch, y64)
        finally:
            g2d.native_final_conv(False)
            g2d.native_body(False)
        assert all(a is b for a, b in zip(originals, slots())) and list(g2d.state_dict().keys()) == keys
