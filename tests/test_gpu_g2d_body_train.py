"""Training through G2d's ResBlock2D body on the matrix cores: model.ResBlock2DFused.from_block(block, trainable=True) and
native_body(trainable=True) against the original encoders2d.ResBlock2D — a deep copy in float64 on the CPU is the answer, the same block
in ATen fp32 on the CPU the yardstick.  Bar per tensor: max|got - t64| <= 4 * max|t32 - t64| + 2^-21 * max|t64| (the factor 4 is the
project's margin for two chained f16x3 convs against ATen's own summation-order error).  Checked: the output, dx, the gradient of every
parameter and, in train mode, the updated running statistics.  err, bar and ratio are printed; with MPHIP_PARITY_JSON=<file> the worst
ratios go to the file tests/test_gpu_conv2d_bwd.py writes (profiles/conv2d_bwd_parity.json holds one MI355X run)."""
import copy
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_conv2d_bwd import note, tensor_bar  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FN = "Conv2dFnBackward"


def _seed(module, seed):
    """Parameters as initialised; BatchNorm statistics and affine moved away from their initial values, so the fold is not trivial."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.5)
    return module


def fn_nodes(t, name=FN):
    """how many nodes of that class the autograd graph of t holds"""
    seen, stack, n = set(), [t.grad_fn], 0
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        n += type(f).__name__ == name
        stack.extend(g for g, _ in f.next_functions)
    return n


def _cpu_run(blk, x, g, dtype, train):
    """(output, dx, {parameter: gradient}, {buffer: value after the call}) of a deep copy of blk in `dtype` on the CPU"""
    ref = copy.deepcopy(blk).to("cpu").to(dtype).train(train)
    xr = x.detach().cpu().to(dtype).requires_grad_(True)
    y = ref(xr)
    (y * g.cpu().to(dtype)).sum().backward()
    return (y.detach(), xr.grad, {k: p.grad for k, p in ref.named_parameters()},
            {k: b.detach().clone() for k, b in ref.named_buffers() if b.is_floating_point()})


def _compare(test, case, name, got, t64, t32):
    err, bar = tensor_bar(got, t64.double(), t32)
    print(f"{case} {name}: err {err:.3e}, bar {bar:.3e}, err / bar {err / bar if bar else 0.0:.4f}")
    note(test, f"{case} {name}", err / bar if bar else 0.0)
    assert err <= bar, (case, name, err, bar)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("h,w", [(12, 20), (16, 16)])
@pytest.mark.parametrize("ci,co", [(32, 32), (32, 64)])
def test_trainable_block_against_float64(ci, co, h, w, train):
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(100 * ci + co + h)
    blk = _seed(E.ResBlock2D(ci, co), 5).to(DEV).train(train)
    x = torch.randn(2, ci, h, w, device=DEV)
    g = torch.randn(2, co, h, w, device=DEV)
    a64, a32 = _cpu_run(blk, x, g, torch.float64, train), _cpu_run(blk, x, g, torch.float32, train)
    fused = M.ResBlock2DFused.from_block(blk, trainable=True)
    assert fused.__dict__.get("_mphip_trainable") is True and fused.training == train
    xg = x.clone().requires_grad_(True)
    assert fused._trainable_ok(xg) and not fused._native_ok(xg)
    y = fused(xg)
    assert fn_nodes(y) == 2          # the native path was really taken: both 3x3 convs
    if not train:                    # the bits of the inference path on the same input
        with torch.no_grad():
            assert not fused._trainable_ok(x) and torch.equal(fused(x), y.detach())
        for conv, bn in fused._fold_pairs():      # what that rests on: the differentiable fold gives the bits the packs were made from
            (wa, ba), (w0, b0) = M.fold_batchnorm_autograd(conv, bn), M.fold_batchnorm(conv, bn)
            assert torch.equal(wa.detach(), w0) and torch.equal(ba.detach(), b0) and wa.requires_grad
        assert len(fused._folded_bwd()) == 3 and (fused._folded_bwd()[2] is None) == (ci == co)
    (y * g).sum().backward()
    case, test = f"{ci}->{co}@{h}x{w}-{'train' if train else 'eval'}", "test_trainable_block_against_float64"
    _compare(test, case, "y", y, a64[0], a32[0])
    _compare(test, case, "dx", xg.grad, a64[1], a32[1])
    for k, p in fused.named_parameters():
        assert p.grad is not None, k
        _compare(test, case, f"d {k}", p.grad, a64[2][k], a32[2][k])
    assert set(dict(fused.named_parameters())) == set(a64[2])
    if train:
        bufs = {k: b for k, b in fused.named_buffers() if b.is_floating_point()}
        assert any(k.endswith("running_mean") for k in bufs)
        for k, b in bufs.items():
            _compare(test, case, k, b, a64[3][k], a32[3][k])
        assert "_mphip_pack2d" in blk.conv1.__dict__ and "_mphip_bwd_pack2d" in blk.conv2.__dict__      # cached per weight version ...
    M._set_trainable(fused, False)                                                                      # ... and gone with the switch
    assert not any(k.startswith("_mphip") and k != "_mphip_fold" for m in (fused, blk.conv1, blk.conv2) for k in m.__dict__)


def test_trainable_off_is_todays_behaviour():
    """the default: under autograd the PyTorch expression, no Conv2dFn node, and no attribute left behind"""
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(3)
    blk = _seed(E.ResBlock2D(32, 64), 4).to(DEV).eval()
    x = torch.randn(2, 32, 12, 20, device=DEV, requires_grad=True)
    fused = M.ResBlock2DFused.from_block(blk)
    assert "_mphip_trainable" not in fused.__dict__ and not fused._trainable_ok(x) and not fused._native_ok(x)
    y = fused(x)
    assert fn_nodes(y) == 0 and torch.equal(y, fused._reference(x))
    assert M._set_trainable(fused, True) and fn_nodes(fused(x)) == 2
    assert M._set_trainable(fused, False) and "_mphip_trainable" not in fused.__dict__ and "_mphip_fold_bwd" not in fused.__dict__
    assert fn_nodes(fused(x)) == 0


@pytest.mark.parametrize("mode", ["autocast", "half"])
def test_trainable_changes_nothing_in_autocast_or_on_a_half_block(mode):
    from megaportrait_hack_amd import encoders2d as E, model as M

    torch.manual_seed(4)
    blk = _seed(E.ResBlock2D(32, 64), 6).to(DEV).eval()
    x = torch.randn(2, 32, 12, 20, device=DEV)
    if mode == "half":
        blk, x = blk.half(), x.half()
    x.requires_grad_(True)
    fused = M.ResBlock2DFused.from_block(blk, trainable=True)
    with torch.autocast("cuda", torch.float16, enabled=mode == "autocast"):
        assert not fused._trainable_ok(x)
        y, want = fused(x), fused._reference(x)
    assert fn_nodes(y) == 0 and y.dtype == want.dtype == torch.float16 and torch.equal(y, want)
    y.float().sum().backward()
    assert blk.conv1.weight.grad is not None and x.grad is not None


def _body(g2d, x):
    """G2d between its head and its final_conv: the 11 ResBlock2D that native_body covers (tools/bench_g2d_body.py's Body)"""
    return g2d.upsample3(g2d.upsample2(g2d.upsample1(g2d.res_blocks(x))))


@pytest.fixture(scope="module")
def body_case():
    """E.G2d in eval mode, a [1,512,4,4] map into its body, a sum loss: (model on the GPU, x, per dtype (y, dx, d res_blocks[0].conv1.weight))"""
    from megaportrait_hack_amd import encoders2d as E

    torch.manual_seed(11)
    g2d = _seed(E.G2d(), 8).eval()
    x = torch.randn(1, 512, 4, 4)
    refs = {}
    for dt in (torch.float64, torch.float32):
        ref = copy.deepcopy(g2d).to(dt)
        xr = x.clone().to(dt).requires_grad_(True)      # (a leaf of its own: .to(float32) alone would hand back x itself)
        y = _body(ref, xr)
        y.sum().backward()
        refs[dt] = (y.detach(), xr.grad, ref.res_blocks[0].conv1.weight.grad)
    for a, b in zip(refs[torch.float64], refs[torch.float32]):     # the yardstick is a yardstick: fp32 tracks float64
        assert (a - b.double()).abs().max().item() <= 1e-3 * a.abs().max().item()
    return g2d.to(DEV), x.to(DEV), refs


@pytest.mark.parametrize("fuse_upsample", [False, True], ids=["plain", "fuse_upsample"])
def test_whole_body_trains_natively(body_case, fuse_upsample):
    from megaportrait_hack_amd import model as M

    g2d, x, refs = body_case
    blocks = lambda: list(g2d.res_blocks) + [g2d.upsample1[1], g2d.upsample2[1], g2d.upsample3[1]]
    originals, keys = blocks() + [g2d.upsample1, g2d.upsample2, g2d.upsample3], list(g2d.state_dict().keys())
    g2d.zero_grad(set_to_none=True)
    try:
        assert g2d.native_body(trainable=True, fuse_upsample=fuse_upsample) is g2d
        assert list(g2d.state_dict().keys()) == keys
        xg = x.clone().requires_grad_(True)
        assert all(isinstance(b, M.ResBlock2DFused) and "_mphip_trainable" in b.__dict__ for b in blocks())
        stages = [g2d.upsample1, g2d.upsample2, g2d.upsample3]
        assert all(isinstance(s, M.Up2ResBlock2DFused) == fuse_upsample for s in stages)
        cur, per_block = xg, []          # every one of the 11 blocks contributes its two convs; a fused stage under autograd evaluates
        for b in list(g2d.res_blocks) + stages:      # its two modules in order: the Upsample in PyTorch, then the block
            assert not (fuse_upsample and b in stages and b._native_ok(cur))
            cur = b(cur)
            per_block.append(fn_nodes(cur))
        assert per_block == [2 * (i + 1) for i in range(11)]
        y = _body(g2d, xg)
        assert fn_nodes(y) == 22 and torch.equal(y, cur)
        y.sum().backward()
        case, test = "fuse_upsample" if fuse_upsample else "plain", "test_whole_body_trains_natively"
        for name, got, k in (("y", y, 0), ("dx", xg.grad, 1), ("d res_blocks[0].conv1.weight", g2d.res_blocks[0].conv1.weight.grad, 2)):
            _compare(test, case, name, got, refs[torch.float64][k], refs[torch.float32][k])
    finally:
        g2d.native_body(False)
        g2d.zero_grad(set_to_none=True)
    assert all(a is b for a, b in zip(originals, blocks() + [g2d.upsample1, g2d.upsample2, g2d.upsample3]))
    assert all("_mphip_trainable" not in b.__dict__ for b in blocks())
