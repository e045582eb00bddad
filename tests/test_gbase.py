"""The orchestrator row: `gbase.Gbase` = the reference's Gbase (model.py:1127-1180) with the hot path on
the HIP kernels and the 2D parts as this repo's own PyTorch restatements (encoders2d.py).

CPU tests: state-dict manifest against the name/shape manifests captured from the REFERENCE's modules
(oracle/make_golden_gbase.py -> tests/golden/gbase_manifest.json, manifest.json) and the 2D restatements against
golden outputs of the reference's modules (tests/golden/gbase2d.npz) — they are plain torch, so they run here.
GPU tests: `forward(xs, xd) -> (image, pyramids)` end to end against the same graph evaluated on the CPU (2D parts on
ATen CPU, hot slice through the oracle), the reference's sub-module call pattern (PairwiseTransferLoss,
model.py:2190-2219), config 5's `reenact`, and the full 512x512 contract."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as R
from oracle.make_golden_gbase import SEED, seeded_module_state

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def gold():
    return np.load(os.path.join(GOLD, "gbase2d.npz"))


def _load(module, seed):
    module.load_state_dict(seeded_module_state(module, seed), strict=True)
    return module.eval()


def maxabs(a, b):
    return (a.detach().cpu().double() - torch.as_tensor(b).double()).abs().max().item()


@pytest.fixture(scope="module")
def E():
    from megaportrait_hack_amd import encoders2d

    return encoders2d


@pytest.fixture(scope="module")
def G():
    from megaportrait_hack_amd import gbase

    return gbase


# ------------------------------------------------------------------------------------------------ CPU: manifest
def test_gbase_state_dict_manifest(G):
    """Every key/shape the reference's modules register is registered by Gbase under the same name (checkpoint layout =
    the drop-in contract, train.py:349-356 / inference.py:59-60)."""
    g = G.Gbase()
    own = {k: list(v.shape) for k, v in g.state_dict().items()}
    with open(os.path.join(GOLD, "gbase_manifest.json")) as f:
        ref2d = json.load(f)["state_dict"]
    with open(os.path.join(GOLD, "manifest.json")) as f:
        ref_hot = json.load(f)["state_dict"]
    expected = {}
    for prefix, table in list(ref2d.items()) + list(ref_hot.items()):
        if prefix == "rotation_net.model":
            continue                                   # a plain object in the reference too: not in Gbase.state_dict()
        for k, shp in table.items():
            expected[f"{prefix}.{k}"] = shp
    # the reference's Eapp was captured with torchvision stubbed out: its ResNet-50 trunk keys are the torchvision names
    missing = {k: v for k, v in expected.items() if own.get(k) != v}
    assert not missing, list(missing.items())[:6]
    extra = [k for k in own if k not in expected and not k.startswith("appearanceEncoder.custom_resnet50.")]
    assert not extra, extra[:6]
    r50 = [k for k in own if k.startswith("appearanceEncoder.custom_resnet50.")]
    assert "appearanceEncoder.custom_resnet50.layer3.5.conv3.weight" in r50 and "appearanceEncoder.custom_resnet50.conv_reduce.bias" in r50
    assert not any("layer4" in k for k in r50)         # model.py:148: the last stage is dropped
    n_param = sum(p.numel() for p in g.parameters())
    assert abs(n_param - 150.4e6) < 0.1e6              # ~150.4 M trainable
    # not registered, exactly like the reference (model.py:876): the frozen 6DRepNet
    assert not any(k.startswith("motionEncoder.rotation_net") for k in own)
    with open(os.path.join(GOLD, "gbase_manifest.json")) as f:
        six = json.load(f)["state_dict"]["rotation_net.model"]
    assert {k: list(v.shape) for k, v in g.motionEncoder.rotation_net.model.state_dict().items()} == six


def test_gbase_attribute_contract(G):
    """model.py:1130-1137 attribute names; no-argument constructor; injectable 2D modules."""
    g = G.Gbase()
    for name in ("appearanceEncoder", "motionEncoder", "warp_generator_s2c", "warp_generator_c2d", "G3d", "G2d", "image_pyramid"):
        assert isinstance(getattr(g, name), torch.nn.Module), name
    marker = torch.nn.Identity()
    assert G.Gbase(G2d=marker).G2d is marker


# ------------------------------------------------------------------------------------------------ CPU: 2D restatements
def test_resblock_custom_and_eapp_trunk_golden(E):
    g = gold()
    with torch.no_grad():
        blk = _load(E.ResBlock_Custom(dimension=2, in_channels=64, out_channels=128), SEED + 1)
        assert maxabs(blk(R.seeded_tensor((1, 64, 16, 16), SEED + 2, scale=1.7)), g["rbc_64_128"]) < 2e-5
        eapp = E.Eapp()
        for i, name in enumerate(("conv", "resblock_128", "resblock_256", "resblock_512", "conv_1")):
            _load(getattr(eapp, name), SEED + 10 + i)
        img = (R.seeded_tensor((1, 3, 64, 64), SEED + 20) + 1.0) * 0.5
        assert maxabs(eapp.trunk2d(img), g["eapp_trunk_64"]) < 2e-5


def test_g2d_body_and_resblock2d_golden(E):
    g = gold()
    with torch.no_grad():
        rb2 = _load(E.ResBlock2D(512, 256), SEED + 30)
        assert maxabs(rb2(R.seeded_tensor((1, 512, 8, 8), SEED + 31, scale=1.7)), g["rb2d_512_256"]) < 2e-5
        g2d = _load(E.G2d(96), SEED + 40)
        assert maxabs(g2d.body(torch.as_tensor(g["g2d_head_4"])), g["g2d_full_4"]) < 2e-5


def test_image_pyramid_golden(E):
    g = gold()
    img = (R.seeded_tensor((1, 3, 64, 64), SEED + 20) + 1.0) * 0.5
    res = E.ImagePyramide(scales=[0.5, 0.25], num_channels=3)(img)
    assert sorted(res) == ["prediction_0.25", "prediction_0.5"]
    for k, v in res.items():
        assert maxabs(v, g["pyr_" + k]) < 1e-6


def test_emtn_nets_golden(E):
    g = gold()
    with torch.no_grad():
        r18 = _load(E.CifarResNet18(num_classes=512), SEED + 50)
        x32 = (R.seeded_tensor((2, 3, 32, 32), SEED + 51) + 1.0) * 0.5
        assert maxabs(r18(x32), g["r18_logits"]) < 2e-5
        emtn = E.Emtn()
        emtn.expression_net.load_state_dict({k: v for k, v in r18.state_dict().items() if not k.startswith("fc.")}, strict=False)
        # Sequential(children[:-1]) renames conv1/bn1/layer* to indices 0..8: load by position instead
        src = [m for n, m in r18.named_children() if n != "fc"]
        for dst, s in zip(list(emtn.expression_net.children())[:len(src)], src):
            dst.load_state_dict(s.state_dict())
        emtn.eval()
        assert maxabs(torch.flatten(emtn.expression_net(x32), start_dim=1), g["r18_expression_feat"]) < 2e-5
        six = _load(E.SixDRepNetBackbone(), SEED + 60)
        x64 = (R.seeded_tensor((2, 3, 64, 64), SEED + 61) + 1.0) * 0.5
        rot, _ = six(x64)
        assert maxabs(rot, g["six_rotmat"]) < 2e-5
        euler, _ = E.SixDRepNet_Detector(six).predict(x64)
        assert maxabs(euler, g["six_euler_deg"]) < 2e-3          # degrees
        p6 = R.seeded_tensor((16, 6), SEED + 62, scale=2.0)
        m6 = E.ortho6d_to_matrix(p6)
        assert maxabs(m6, g["ortho6d_matrix"]) < 1e-6
        assert maxabs(E.euler_from_matrix(m6), g["ortho6d_euler_rad"]) < 1e-5


class _RefShaped(torch.nn.Module):
    """A module that is not one of ours, holding one of ours' parameters, buffers and children under the same names (so: the same
    state-dict keys) — what a reference class looks like to integration.install."""

    def __init__(self, inner):
        super().__init__()
        for n, p in inner.named_parameters(recurse=False):
            self.register_parameter(n, p)
        for n, b in inner.named_buffers(recurse=False):
            self.register_buffer(n, b)
        for n, c in inner.named_children():
            self.add_module(n, c)


# the hot slice the way a reference-shaped orchestrator reaches it (model.py:1151-1171): sub-modules by attribute name, the warp
# through the module-level function, looked up in the defining module's globals at call time
_STAND_IN_GBASE_FORWARD = """
def forward(self, xs, xd):
    vs, es = self.appearanceEncoder(xs)
    Rs, ts, zs = self.motionEncoder(xs)
    Rd, td, zd = self.motionEncoder(xd)
    vc2d = self.G3d(apply_warping_field(vs, self.warp_generator_s2c(Rs, ts, zs, es)))
    return self.G2d(torch.sum(apply_warping_field(vc2d, self.warp_generator_c2d(Rd, td, zd, es)), dim=2))
"""


def _stand_in_reference_module():
    """A reference-shaped `model` module for hosts where the reference cannot be imported: a Gbase class whose `forward` is defined
    in this module (so install() must patch the module's globals), and constructors with the reference's names that build modules
    which are not this package's hot-path classes but carry their state-dict keys (the 2D parts: this package's own restatements)."""
    import types

    from megaportrait_hack_amd import encoders2d as E, integration, model as M

    mod = types.ModuleType("model")
    mod.torch, mod.apply_warping_field, mod.compute_rt_warp = torch, R.apply_warping_field, R.compute_rt_warp
    exec(_STAND_IN_GBASE_FORWARD, vars(mod))
    mod.Gbase = type("Gbase", (torch.nn.Module,), {"forward": vars(mod).pop("forward")})

    def eapp():
        enc = E.Eapp()
        for n in integration._EAPP_TAIL_BLOCKS:
            setattr(enc, n, _RefShaped(getattr(enc, n)))
        return enc

    mod.Eapp = eapp
    mod.WarpGeneratorS2C = lambda num_channels: _RefShaped(M.WarpGeneratorS2C(num_channels=num_channels))
    mod.WarpGeneratorC2D = lambda num_channels: _RefShaped(M.WarpGeneratorC2D(num_channels=num_channels))
    mod.G3d = lambda in_channels: _RefShaped(M.G3d(in_channels=in_channels))
    mod.G2d, mod.ImagePyramide = E.G2d, E.ImagePyramide
    return mod


def test_reference_gbase_forward_is_installable():
    """An object of the REFERENCE's own Gbase class (its __init__ cannot run offline, so the attributes are set by hand from the
    reference's classes) goes through integration.install; the reference's `forward` then reaches the HIP classes through the same
    attribute names and the patched module-level functions.  Where the reference cannot be imported, the same with a
    reference-shaped stand-in module (_stand_in_reference_module)."""
    try:
        from oracle.import_reference import load_reference_model

        ref = load_reference_model()
    except Exception:
        ref = _stand_in_reference_module()
    from megaportrait_hack_amd import encoders2d as E, integration, model as M

    g = ref.Gbase.__new__(ref.Gbase)
    torch.nn.Module.__init__(g)
    g.appearanceEncoder, g.motionEncoder = ref.Eapp(), E.Emtn()
    g.warp_generator_s2c, g.warp_generator_c2d = ref.WarpGeneratorS2C(512), ref.WarpGeneratorC2D(512)
    g.G3d, g.G2d = ref.G3d(96), ref.G2d(96)
    g.image_pyramid = ref.ImagePyramide(scales=[0.5, 0.25], num_channels=3)
    keys_before = {k: tuple(v.shape) for k, v in g.state_dict().items()}
    saved = (ref.apply_warping_field, ref.compute_rt_warp)
    try:
        done = integration.install(g, ref)
        assert {"warp_generator_s2c", "warp_generator_c2d", "G3d", "model.apply_warping_field", "model.compute_rt_warp"} <= set(done)
        assert sum(d.startswith("appearanceEncoder.resblock3D") for d in done) == 5
        assert isinstance(g.G3d, M.G3d) and isinstance(g.appearanceEncoder.resblock3D_96_2, M.ResBlock3D_Adaptive)
        assert type(g).forward is ref.Gbase.forward                                 # the reference's own forward, untouched
        assert ref.Gbase.forward.__globals__["apply_warping_field"] is M.apply_warping_field   # what forward will call
        assert {k: tuple(v.shape) for k, v in g.state_dict().items()} == keys_before
    finally:
        ref.apply_warping_field, ref.compute_rt_warp = saved


# ------------------------------------------------------------------------------------------------ GPU
def _cpu_gbase_reference(g_cpu, sd_hot, xs, xd):
    """The same graph with nothing from the HIP library: 2D parts = the plain-torch modules on CPU, Eapp's 3D tail,
    the hot slice and G2d's two 1x1 convs through oracle/hotpath_ref.py (ATen CPU)."""
    enc, mot, g2d = g_cpu.appearanceEncoder, g_cpu.motionEncoder, g_cpu.G2d
    tail_sd = {"appearanceEncoder." + k: v for k, v in enc.state_dict().items() if k.startswith("resblock3D")}
    vs = R.eapp_tail3d(enc.trunk2d(xs), tail_sd)
    es = enc.descriptor(xs)
    Rs, ts, zs = mot(xs)
    Rd, td, zd = mot(xd)
    proj = R.hot_slice(vs=vs, es=es, Rs=Rs, ts=ts, zs=zs, Rd=Rd, td=td, zd=zd, sd=sd_hot)
    head = R.g2d_head(proj, {"G2d." + k: v for k, v in g2d.state_dict().items() if k.startswith(("reshape", "conv1x1"))})
    img = g2d.body(head)
    return img, g_cpu.image_pyramid(img), dict(vs=vs, es=es, Rs=Rs, ts=ts, zs=zs, Rd=Rd, td=td, zd=zd, proj=proj)


def _seeded_gbase(G):
    import copy

    g = G.Gbase()
    g.load_state_dict(seeded_module_state(g, SEED + 70), strict=True)
    six = g.motionEncoder.rotation_net.model
    six.load_state_dict(seeded_module_state(six, SEED + 71), strict=True)
    return g.eval(), copy.deepcopy(g).eval()


@pytest.mark.gpu
def test_gbase_forward_end_to_end_small(G):
    """forward_any_size(xs, xd) on 64x64 images (volume 96x16x8x8) == the CPU evaluation of the same graph."""
    dev = torch.device("cuda:0")
    g, g_cpu = _seeded_gbase(G)
    sd_hot = {k: v for k, v in g_cpu.state_dict().items() if k.startswith(("warp_generator_", "G3d."))}
    xs = (R.seeded_tensor((2, 3, 64, 64), SEED + 80) + 1.0) * 0.5
    xd = (R.seeded_tensor((2, 3, 64, 64), SEED + 81) + 1.0) * 0.5
    with torch.no_grad():
        want_img, want_pyr, mid = _cpu_gbase_reference(g_cpu, sd_hot, xs, xd)
        g.to(dev)
        img, pyr = g.forward_any_size(xs.to(dev), xd.to(dev))
        enc = g.encode(xs.to(dev), xd.to(dev))
    assert img.shape == (2, 3, 64, 64) and sorted(pyr) == ["prediction_0.25", "prediction_0.5"]
    for got, name in zip(enc, ("vs", "es", "Rs", "ts", "zs", "Rd", "td", "zd")):
        tol = 2e-2 if name in ("Rs", "Rd") else 1e-3          # rotations are in degrees (atan2 of a 27-layer net's output)
        assert maxabs(got, mid[name]) < tol, name
    assert maxabs(img, want_img) < 1e-3
    for k in pyr:
        assert maxabs(pyr[k], want_pyr[k]) < 1e-3
    # the NHWC option is a layout choice: same keys, same image (up to MIOpen's kernel selection), forward and reenact
    keys = list(g.state_dict())
    with torch.no_grad():
        g.channels_last_2d()
        img_cl, _ = g.forward_any_size(xs.to(dev), xd.to(dev))
        ree = g.reenact(xs[:1].to(dev), xd.to(dev))
        g.channels_last_2d(False)
    assert list(g.state_dict()) == keys
    assert maxabs(img_cl, want_img) < 1e-3
    assert ree.shape == (2, 3, 64, 64) and ree.is_contiguous() and torch.isfinite(ree).all()


@pytest.mark.gpu
def test_gbase_submodule_call_pattern(G):
    """PairwiseTransferLoss (model.py:2190-2219) bypasses Gbase.forward: it calls the encoders, both warp generators,
    G3d and G2d as attributes and the module-level apply_warping_field + torch.sum(dim=2).  The same pattern on this
    Gbase must give what its fused forward gives, and differentiate."""
    from megaportrait_hack_amd import model as M

    dev = torch.device("cuda:0")
    g, _ = _seeded_gbase(G)
    g.to(dev)
    I1 = ((R.seeded_tensor((1, 3, 64, 64), SEED + 82) + 1.0) * 0.5).to(dev)
    I2 = ((R.seeded_tensor((1, 3, 64, 64), SEED + 83) + 1.0) * 0.5).to(dev)
    with torch.no_grad():
        vs1, es1 = g.appearanceEncoder(I1)
        Rs1, ts1, zs1 = g.motionEncoder(I1)
        Rs2, ts2, zs2 = g.motionEncoder(I2)
        w_s2c = g.warp_generator_s2c(Rs1, ts1, zs1, es1)
        vc2d = g.G3d(M.apply_warping_field(vs1, w_s2c))
        w_c2d = g.warp_generator_c2d(Rs2, ts2, zs2, es1)
        I_sub = g.G2d(torch.sum(M.apply_warping_field(vc2d, w_c2d), dim=2))
        I_fwd, _ = g.forward_any_size(I1, I2)
    assert maxabs(I_sub, I_fwd.cpu()) < 1e-4
    # under autograd (train.py:312-320): the loss of the pattern reaches the hot-path parameters and the encoders
    g.train()
    vs1, es1 = g.appearanceEncoder(I1)
    Rs1, ts1, zs1 = g.motionEncoder(I1)
    Rs2, ts2, zs2 = g.motionEncoder(I2)
    pose = g.G2d(torch.sum(M.apply_warping_field(g.G3d(M.apply_warping_field(vs1, g.warp_generator_s2c(Rs2, ts2, zs1, es1))),
                                                 g.warp_generator_c2d(Rs2, ts2, zs1, es1)), dim=2))
    expr = g.G2d(torch.sum(M.apply_warping_field(g.G3d(M.apply_warping_field(vs1, g.warp_generator_s2c(Rs1, ts1, zs2, es1))),
                                                 g.warp_generator_c2d(Rs1, ts1, zs2, es1)), dim=2))
    F.l1_loss(pose, expr).backward()
    for name in ("G3d.final_conv.weight", "warp_generator_s2c.flowfield.conv3x3x3.weight", "G2d.reshape.weight",
                 "appearanceEncoder.conv.weight", "appearanceEncoder.resblock3D_96_2.conv1.weight", "motionEncoder.fc.weight"):
        p = dict(g.named_parameters())[name]
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0, name


@pytest.mark.gpu
def test_gbase_full_size_contract_and_reenact(G):
    """512x512 (the only size the reference's forward accepts, model.py:1157): return types/shapes of model.py:1180; the
    256x256 input trips the same assert; reenact(1 source x N drivers) == forward on every pair."""
    dev = torch.device("cuda:0")
    g, _ = _seeded_gbase(G)
    g.to(dev)
    xs = ((R.seeded_tensor((1, 3, 512, 512), SEED + 84) + 1.0) * 0.5).to(dev)
    xd = ((R.seeded_tensor((3, 3, 512, 512), SEED + 85) + 1.0) * 0.5).to(dev)
    with torch.no_grad():
        img, pyr = g(xs.expand(3, -1, -1, -1).contiguous(), xd)
        assert img.shape == (3, 3, 512, 512) and img.dtype == torch.float32
        assert pyr["prediction_0.5"].shape == (3, 3, 256, 256) and pyr["prediction_0.25"].shape == (3, 3, 128, 128)
        assert torch.isfinite(img).all() and 0.0 <= img.min().item() and img.max().item() <= 1.0     # sigmoid output
        with pytest.raises(AssertionError):
            g(xs[:, :, :256, :256].contiguous(), xd[:1, :, :256, :256].contiguous())
        fast = g.reenact(xs, xd, chunk=2)
        assert maxabs(fast, img.cpu()) < 1e-4
        # config 5's "fp16": autocast on the PyTorch-ROCm 2D modules (the reference's policy, train.py:188), HIP path unchanged
        half = g.reenact(xs, xd, chunk=2, fp16=True)
        assert half.dtype == torch.float32 and half.shape == fast.shape
        err16 = maxabs(half, fast.cpu())
        print(f"config 5 fp16 (autocast on the 2D modules) vs fp32: max-abs {err16:.3e} on images in (0,1)")
        assert err16 < 3e-2
        parts = [g.reenact(xs, xd, chunk=2, rank=r, world=2) for r in range(2)]
        assert [p.shape[0] for p in parts] == [2, 1]
        assert maxabs(torch.cat(parts), fast.cpu()) < 1e-5      # (MIOpen's 2D convs are not bitwise reproducible run to run)
