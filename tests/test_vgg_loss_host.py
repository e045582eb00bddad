"""Host-side checks of the VGG19 feature loss (no GPU): the entries of csrc/feature_loss.hip (mphip_maxpool2_supported,
mphip_maxpool2_fwd, mphip_feature_l1_supported, mphip_feature_l1_workspace_bytes, mphip_feature_l1, mphip_feature_grad_assemble_supported,
mphip_feature_grad_assemble_workspace_bytes, mphip_feature_grad_assemble, mphip_conv2d_stem_bwd_data_supported,
mphip_conv2d_stem_bwd_data) are exported with the ABI still at 30, their shape and workspace rules, their refusals before any HIP call,
the register table, the module's layout and plain-PyTorch path, integration.install_vgg19_loss, and the conditions under which the
integer cases of tests/test_gpu_vgg_loss.py are exact."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn as nn

from megaportrait_hack_amd import _lib, integration
from megaportrait_hack_amd.losses import VGG19_CONVS, VGG19_POOLS, VGG19FeatureLoss

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vgg_loss_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mphip_maxpool2_supported", "mphip_maxpool2_fwd", "mphip_feature_l1_supported", "mphip_feature_l1_workspace_bytes",
           "mphip_feature_l1", "mphip_feature_grad_assemble_supported", "mphip_feature_grad_assemble_workspace_bytes",
           "mphip_feature_grad_assemble", "mphip_conv2d_stem_bwd_data_supported", "mphip_conv2d_stem_bwd_data")
EINVAL, EWORKSPACE = -1, -3
L1_BLOCKS, FGA_BLOCKS = 1024, 4096     # csrc/feature_loss.hip: FL_L1_BLOCKS, FL_MAX_BLOCKS


def test_library_exports_the_entries_and_the_abi_stays_30():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mphip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(raw, name) and (name + "(") in hdr, name
    assert lib.mphip_version() == _lib.EXPECTED_ABI_VERSION == _lib.header_abi_version() == 30


def test_shape_and_workspace_rules():
    lib = _lib.load()
    pool, l1, fga, stem = (lib.mphip_maxpool2_supported, lib.mphip_feature_l1_supported, lib.mphip_feature_grad_assemble_supported,
                           lib.mphip_conv2d_stem_bwd_data_supported)
    # max-pool: NC >= 1, H, W >= 2, NC * H * W < 2^31
    for nc in (0, 1, 3, 128):
        for h in (0, 1, 2, 5, 512):
            for w in (0, 1, 2, 3, 512):
                assert pool(nc, h, w) == int(nc >= 1 and h >= 2 and w >= 2), (nc, h, w)
    assert pool(1 << 11, 1 << 10, 1 << 10) == 0 and pool((1 << 11) - 1, 1 << 10, 1 << 10) == 1
    # the L1 tap: N, M >= 1, 2 * N * M < 2^31; one fp64 slot per workgroup of 1024 differences, at most L1_BLOCKS
    for n in (0, 1, 2, 4):
        for m in (0, 1, 1023, 1024, 1025, 48 * 9 * 17, 1 << 24, 1 << 28):
            ok = n >= 1 and m >= 1 and 2 * n * m < 2 ** 31
            assert l1(n, m) == int(ok), (n, m)
            assert lib.mphip_feature_l1_workspace_bytes(n, m) == (8 * min(L1_BLOCKS, (n * m + 1023) // 1024) if ok else 0), (n, m)
    assert l1(1, (1 << 30) - 1) == 1 and l1(1, 1 << 30) == 0
    # the gradient assembly: N, C, H, W >= 1, upstream 0 / 1 / 2 (2: H, W >= 2), 2 * N * C * H * W < 2^31; one float per workgroup of
    # 256 patches of 2 x 2 elements (the element form), at most FGA_BLOCKS
    for n, c in ((0, 8), (1, 0), (1, 32), (2, 64)):
        for h, w in ((0, 4), (4, 0), (1, 1), (1, 2), (2, 1), (2, 2), (5, 3), (9, 17), (512, 512)):
            for up in (-1, 0, 1, 2, 3):
                ok = n >= 1 and c >= 1 and h >= 1 and w >= 1 and up in (0, 1, 2) and (up != 2 or (h >= 2 and w >= 2))
                assert fga(n, c, h, w, up) == int(ok), (n, c, h, w, up)
            ok = n >= 1 and c >= 1 and h >= 1 and w >= 1
            want = 4 * min(FGA_BLOCKS, (n * c * ((h + 1) // 2) * ((w + 1) // 2) + 255) // 256) if ok else 0
            assert lib.mphip_feature_grad_assemble_workspace_bytes(n, c, h, w) == want, (n, c, h, w)
    assert fga(4, 512, 1 << 10, 1 << 9, 1) == 0 and fga(2, 512, 1 << 10, 1 << 9, 1) == 1     # 2 * N * C * H * W = 2^31 and 2^30
    # the stem's backward-data: Co % 16 == 0, N, H, W >= 1, N * Co * H * W < 2^31
    for bad in [(0, 64, 8, 8), (1, 0, 8, 8), (1, 8, 8, 8), (1, 24, 8, 8), (1, 64, 0, 8), (1, 64, 8, 0), (2, 64, 4096, 4096)]:
        assert stem(*bad) == 0, bad
    for good in [(1, 16, 1, 1), (1, 32, 9, 17), (4, 64, 512, 512), (1, 64, 4096, 4096)]:
        assert stem(*good) == 1, good


def test_arguments_are_refused_without_a_gpu():
    """Every refusal happens before the first HIP call: these pointers are host addresses that are never dereferenced."""
    lib = _lib.load()
    err = lib.mphip_last_error
    buf = ctypes.create_string_buffer(1 << 18)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, r, s = (ctypes.c_void_p(base + i * 65536) for i in range(4))           # four disjoint 64 KiB regions
    at = lambda b, off: ctypes.c_void_p(b.value + off)

    pool = lambda x=p, y=q, rng=None, nc=4, h=8, w=8: lib.mphip_maxpool2_fwd(x, y, rng, nc, h, w, None)
    assert pool(x=None) == EINVAL and b"maxpool2_fwd: null pointer" in err()
    assert pool(y=None, h=1) == EINVAL and b"maxpool2_fwd: null pointer" in err()        # a null pointer is reported before a bad shape
    for bad in (dict(nc=0), dict(h=1), dict(w=1)):
        assert pool(**bad) == EINVAL and b"maxpool2_fwd: unsupported shape" in err(), bad
    for off in (dict(x=at(p, 2)), dict(y=at(q, 1)), dict(rng=at(r, 2))):
        assert pool(**off) == EINVAL and b"4-byte aligned" in err(), off
    assert pool(y=at(p, 1020)) == EINVAL and b"must not alias" in err()                  # x is 4 * 8 * 8 floats = 1024 bytes
    assert pool(h=1, y=at(p, 2)) == EINVAL and b"unsupported shape" in err()             # a bad shape before the alignment

    need = lib.mphip_feature_l1_workspace_bytes(2, 4096)
    assert need == 8 * 8
    l1 = lambda y=p, n=2, m=4096, out=q, ws=r, nb=need: lib.mphip_feature_l1(y, n, m, 0.5, out, ws, nb, None)
    assert l1(y=None) == EINVAL and b"feature_l1: null pointer" in err()
    assert l1(out=None, m=0) == EINVAL and b"feature_l1: null pointer" in err()
    for bad in (dict(n=0), dict(m=0), dict(n=1, m=1 << 30)):
        assert l1(**bad) == EINVAL and b"feature_l1: unsupported shape" in err(), bad
    for off in (dict(y=at(p, 2)), dict(out=at(q, 3))):
        assert l1(**off) == EINVAL and b"4-byte aligned" in err(), off
    assert l1(ws=None) == EWORKSPACE and l1(nb=need - 1) == EWORKSPACE and b"feature_l1: workspace" in err()
    assert l1(ws=at(r, 8)) == EINVAL and b"16-byte aligned" in err()
    assert l1(ws=at(r, 8), nb=need - 1) == EWORKSPACE                                    # the size before the alignment

    need = lib.mphip_feature_grad_assemble_workspace_bytes(1, 32, 8, 8)
    assert need == 4 * 2
    fga = lambda y=p, up=q, kind=1, cf=r, g=s, sc=at(s, 32768), n=1, c=32, h=8, w=8, ws=at(r, 1024), nb=need: \
        lib.mphip_feature_grad_assemble(y, up, kind, cf, g, sc, n, c, h, w, ws, nb, None)
    for missing in ("y", "g", "sc", "up"):
        assert fga(**{missing: None}) == EINVAL and b"feature_grad_assemble: null pointer" in err(), missing
    assert fga(up=None, kind=2) == EINVAL and b"null pointer" in err()
    assert fga(y=None, c=0) == EINVAL and b"null pointer" in err()
    for bad in (dict(n=0), dict(c=0), dict(h=0), dict(kind=3), dict(kind=-1), dict(kind=2, h=1), dict(kind=2, w=1)):
        assert fga(**bad) == EINVAL and b"feature_grad_assemble: unsupported shape" in err(), bad
    assert fga(up=None, kind=0, cf=None) == EINVAL and b"neither an upstream gradient nor a tap" in err()
    for off in (dict(y=at(p, 2)), dict(up=at(q, 2)), dict(cf=at(r, 1)), dict(g=at(s, 2)), dict(sc=at(s, 32770))):
        assert fga(**off) == EINVAL and b"4-byte aligned" in err(), off
    assert fga(g=at(p, 16380)) == EINVAL and b"must not alias" in err()                  # y is 2 * 32 * 8 * 8 floats = 16384 bytes
    assert fga(ws=None) == EWORKSPACE and fga(nb=need - 1) == EWORKSPACE and b"feature_grad_assemble: workspace" in err()
    assert fga(ws=at(r, 1028)) == EINVAL and b"16-byte aligned" in err()

    stem = lambda dy=p, w=q, dx=r, n=1, co=16, h=8, wd=8: lib.mphip_conv2d_stem_bwd_data(dy, w, dx, n, co, h, wd, None)
    for missing in ("dy", "w", "dx"):
        assert stem(**{missing: None}) == EINVAL and b"conv2d_stem_bwd_data: null pointer" in err(), missing
    assert stem(dy=None, co=8) == EINVAL and b"null pointer" in err()
    for bad in (dict(n=0), dict(co=8), dict(co=24), dict(h=0), dict(wd=0)):
        assert stem(**bad) == EINVAL and b"conv2d_stem_bwd_data: unsupported shape" in err(), bad
    for off in (dict(dy=at(p, 2)), dict(w=at(q, 2)), dict(dx=at(r, 1))):
        assert stem(**off) == EINVAL and b"4-byte aligned" in err(), off
    assert stem(dx=at(p, 4092)) == EINVAL and b"must not alias" in err()                 # dy is 16 * 8 * 8 floats = 4096 bytes


def test_kernels_are_in_the_register_table_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import register_table

    kernels = register_table.collect(["feature_loss.hip"])["feature_loss.hip"]["kernels"]
    names = sorted(k["demangled"].split("(")[0] for k in kernels)
    assert names == ["conv2d_stem_bwd_data_kernel", "feature_grad_assemble_kernel<2>", "feature_grad_assemble_kernel<4>",
                     "feature_grad_scale_kernel", "feature_l1_finish_kernel", "feature_l1_partial_kernel<0>", "feature_l1_partial_kernel<1>",
                     "maxpool2_kernel<0>", "maxpool2_kernel<1>"], names
    for k in kernels:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k.get("agpr_count", 0) == 0 and k["vgpr_count"] <= 128, k                 # four waves per SIMD


def test_state_dict_has_vgg19s_26_keys_and_shapes():
    loss = VGG19FeatureLoss()
    sd = loss.vgg19.state_dict()
    ci, want = 3, {}
    for i, co in zip(VGG19_CONVS, (64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512)):
        want[f"{i}.weight"], want[f"{i}.bias"] = (co, ci, 3, 3), (co,)
        ci = co
    assert len(want) == 26 and {k: tuple(v.shape) for k, v in sd.items()} == want
    assert list(loss.state_dict().keys()) == ["vgg19." + k for k in sd]                 # nothing else is persistent
    assert not any(p.requires_grad for p in loss.parameters())
    layers = list(loss.vgg19)
    assert len(layers) == 30 and all(isinstance(layers[i], nn.MaxPool2d) for i in VGG19_POOLS)
    assert all(isinstance(layers[i], nn.Conv2d) and isinstance(layers[i + 1], nn.ReLU) for i in VGG19_CONVS)
    # a Sequential of the same layout loads from it and is shared, not copied, by from_sequential; its requires_grad is left alone
    other = VGG19FeatureLoss(widths=(32, 32, 64, 64, 64))
    seq = nn.Sequential(*[type(m)(**{k: getattr(m, k) for k in ("in_channels", "out_channels", "kernel_size", "padding")})
                          if isinstance(m, nn.Conv2d) else (nn.ReLU(inplace=True) if isinstance(m, nn.ReLU) else nn.MaxPool2d(2, 2))
                          for m in other.vgg19])
    seq.load_state_dict(other.vgg19.state_dict())
    shared = VGG19FeatureLoss.from_sequential(seq)
    assert shared.vgg19 is seq and all(a is b for a, b in zip(shared.parameters(), seq.parameters()))
    assert all(p.requires_grad for p in seq.parameters())


def test_from_sequential_says_what_it_expected():
    good = list(VGG19FeatureLoss(widths=(32, 32, 64, 64, 64)).vgg19)
    for i, wrong, word in ((4, nn.AvgPool2d(2, 2), "MaxPool2d"), (4, nn.MaxPool2d(3, 2, 1), "MaxPool2d"), (1, nn.LeakyReLU(0.1), "ReLU"),
                           (2, nn.Conv2d(32, 32, 3, padding=1, bias=False), "Conv2d"), (2, nn.Conv2d(32, 32, 3, stride=2, padding=1), "Conv2d"),
                           (2, nn.Conv2d(16, 32, 3, padding=1), "Conv2d"), (5, nn.Conv2d(32, 32, 1), "Conv2d")):
        layers = list(good)
        layers[i] = wrong
        with pytest.raises(TypeError, match=word):
            VGG19FeatureLoss.from_sequential(nn.Sequential(*layers))
    with pytest.raises(TypeError, match="30 layers"):
        VGG19FeatureLoss.from_sequential(nn.Sequential(*good[:29]))
    with pytest.raises(TypeError, match="Sequential"):
        VGG19FeatureLoss.from_sequential(object())
    with pytest.raises(ValueError, match="taps"):
        VGG19FeatureLoss(taps=(0, 6))


def _compute_perceptual_loss(model, layers, predicted, target, detach=False):
    """model.py:1990-2017 of the reference, restated (no Linear layer occurs in vgg19.features[0:30])"""
    loss = 0.0
    predicted_features = predicted
    target_features = target
    for i, layer in enumerate(model.children()):
        predicted_features = layer(predicted_features)
        target_features = layer(target_features)
        if i in layers:
            if detach:
                loss += torch.mean(torch.abs(predicted_features - target_features.detach()))
            else:
                loss += torch.mean(torch.abs(predicted_features - target_features))
    return loss


def test_forward_reference_is_the_references_expression_in_float64():
    torch.manual_seed(3)
    loss = VGG19FeatureLoss(widths=(8, 8, 16, 16, 24)).double()
    p, t = torch.randn(2, 3, 20, 28, dtype=torch.float64), torch.randn(2, 3, 20, 28, dtype=torch.float64)
    want = _compute_perceptual_loss(loss.vgg19, [1, 6, 11, 20, 29], p, t)
    assert want.item() > 0 and torch.equal(loss.forward_reference(p, t), want) and torch.equal(loss(p, t), want)     # (CPU: forward is it)
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    norm = VGG19FeatureLoss.from_sequential(loss.vgg19, normalize=True).double()
    want = _compute_perceptual_loss(loss.vgg19, [1, 6, 11, 20, 29], (p - mean.double()) / std.double(), (t - mean.double()) / std.double())
    assert torch.equal(norm(p, t), want)
    # two taps, summed
    some = VGG19FeatureLoss.from_sequential(loss.vgg19, taps=(6, 20), reduction="sum")
    feats, a, b = [], p, t
    for i, layer in enumerate(loss.vgg19):
        a, b = layer(a), layer(b)
        if i in (6, 20):
            feats.append((a - b).abs().sum())
    assert torch.equal(some(p, t), feats[0] + feats[1])
    # the gradient reaches the predicted image on the plain path
    q = p.clone().requires_grad_(True)
    loss(q, t).backward()
    assert q.grad is not None and q.grad.abs().max().item() > 0


def test_install_vgg19_loss_replaces_both_methods_on_a_stub():
    class Stub:
        def __init__(self):
            self.vgg19 = VGG19FeatureLoss(widths=(8, 8, 16, 16, 24)).vgg19
            self.vgg19.requires_grad_(True)           # torchvision's weights come this way
            self.vgg19_layers = [1, 6, 11, 20, 29]

        def compute_vgg19_loss(self, predicted, target):
            raise AssertionError("the original method")

        def compute_feature_matching_loss(self, predicted, target):
            raise AssertionError("the original method")

    stub = Stub()
    assert integration.install_vgg19_loss(stub) == ["compute_vgg19_loss", "compute_feature_matching_loss"]
    assert all(p.requires_grad for p in stub.vgg19.parameters())                        # left alone: freezing is the caller's
    torch.manual_seed(4)
    p, t = torch.randn(1, 3, 16, 16), torch.randn(1, 3, 16, 16, requires_grad=True)
    want = _compute_perceptual_loss(stub.vgg19, stub.vgg19_layers, p, t)
    assert torch.equal(stub.compute_vgg19_loss(p, t), want)
    fm = stub.compute_feature_matching_loss(p, t)
    assert torch.equal(fm, _compute_perceptual_loss(stub.vgg19, stub.vgg19_layers, p, t, detach=True))
    fm.backward()
    assert t.grad is None                                                               # the target is detached there
    assert stub.__dict__["_mphip_vgg19_loss"].vgg19 is stub.vgg19


def test_native_ok_states_the_rules_without_a_gpu():
    loss = VGG19FeatureLoss(widths=(32, 32, 64, 64, 64))
    p = torch.zeros(1, 3, 32, 32)
    assert not loss.native_ok(p, p)                                                     # CPU tensors
    assert loss.native(False) is loss and loss.native() is loss


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_integer_cases_are_exact_by_construction(name):
    """What tests/test_gpu_vgg_loss.py relies on when it asks for torch.equal, checked in float64 before a GPU is touched."""
    loss, predicted, target = cases.case(name)
    for m in loss.vgg19:
        if isinstance(m, nn.Conv2d):
            w = m.weight.view(m.weight.shape[0], -1)
            assert bool(((w == 0) | (w.abs() == 1)).all()) and bool(((w != 0).sum(1) == cases.NONZERO_PER_CHANNEL).all())
            assert bool((m.bias.abs() <= 1).all()) and bool((m.bias == m.bias.round()).all())
    for x in (predicted, target):
        assert bool((x == x.round()).all()) and x.abs().max().item() <= 4
    ref = cases.reference(name)
    print(name, {k: v for k, v in ref.items() if k not in ("loss", "grad")})
    assert ref["a_max"] < 2 ** 21                                                       # max over layers of sum |w||x| + |b|
    assert ref["grads_on_granule"] and ref["grad_max_granules"] < 2 ** 21               # every gradient, in units of the smallest coefficient
    assert all(0.2 <= s <= 0.8 for s in ref["tap_equal_share"]), ref["tap_equal_share"]  # sgn(0) is exercised at every tap
    assert ref["deepest_tap"] > 0
    if loss.reduction == "mean":
        assert all(cases.is_pow2(c) for c in ref["tap_counts"]) and ref["granule"] == 2.0 ** -16
    else:
        assert ref["granule"] == 1.0 and ref["loss"].item() < 2 ** 24
        assert [tuple(t) for t in _map_sizes(predicted.shape[2:])] == [(40, 24), (20, 12), (10, 6), (5, 3), (2, 1)]   # an odd row and column is dropped
    # every tap and the gradient are fp32 values: the cast of the float64 reference loses nothing.  The loss is the taps' sum rounded
    # once (the module adds the five fp32 taps in fp64), which is the float64 reference cast to fp32 whether or not it fits 24 bits
    for v in [ref["grad"]] + [torch.tensor(t, dtype=torch.float64) for t in ref["tap_values"]]:
        assert torch.equal(v.float().double(), v)
    assert sum(ref["tap_values"]) == ref["loss"].item()                                  # (exact in fp64: multiples of 2^-16 below 2^10)


def _map_sizes(hw):
    h, w = hw
    out = [(h, w)]
    for _ in VGG19_POOLS:
        h, w = h // 2, w // 2
        out.append((h, w))
    return out
