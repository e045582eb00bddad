"""G2d's exit as fused HIP kernels (csrc/g2d_final.hip, model.G2dFinalConv): GroupNorm(32,64) -> ReLU -> Conv2d(64,3,3,padding=1) -> Sigmoid.

Oracle: the same nn.Sequential with the same parameters in fp64 on the CPU.  Error bar, per case: e_hip = max|y_hip - y_64| against
e_torch = max|y_torch32 - y_64| (torch's own fp32 evaluation on the GPU): e_hip <= 4 * e_torch + 2^-22 — 4 for a different summation
order of the 576-term dot product, 2^-22 = four fp32 ulps at outputs in (1/2, 1) as the floor where torch happens to be exact.  Gradients:
the same rule per tensor, scaled by that tensor's max-abs in fp64.  Every test prints its measured pair before it asserts (run with -s:
lines starting with `g2d_final_parity`); profiles/g2d_final_parity.json is where one MI355X run's pairs belong."""
import ctypes
import json

import pytest
import torch
import torch.nn as nn

from megaportrait_hack_amd import _lib, autograd as ag, encoders2d as E, gbase, model as M, ops

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22
DEV = torch.device("cuda:0")


def _sequential():
    return nn.Sequential(nn.GroupNorm(32, 64), nn.ReLU(inplace=True), nn.Conv2d(64, 3, 3, padding=1), nn.Sigmoid())


def _seeded(seed, gamma_scale=1.0, beta=None):
    """An fp32 Sequential on the CPU with non-trivial gamma / beta (not the 1 / 0 initial values)."""
    g = torch.Generator().manual_seed(seed)
    seq = _sequential()
    with torch.no_grad():
        seq[0].weight.copy_((0.5 + torch.rand(64, generator=g)) * gamma_scale * (torch.randint(0, 2, (64,), generator=g) * 2 - 1))
        seq[0].bias.copy_(torch.randn(64, generator=g) * 0.5 if beta is None else torch.full((64,), float(beta)))
        seq[2].weight.copy_(torch.randn(3, 64, 3, 3, generator=g) * 0.08)
        seq[2].bias.copy_(torch.randn(3, generator=g) * 0.2)
    return seq


def _input(shape, seed, mean=0.0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std + mean


def _oracle(seq, x):
    import copy

    with torch.no_grad():
        return copy.deepcopy(seq).cpu().double()(x.cpu().double())


def _native(seq):
    return M.G2dFinalConv.from_sequential(seq)


def _report(name, e_hip, e_torch, bar):
    print("g2d_final_parity " + json.dumps({"case": name, "e_hip": e_hip, "e_torch": e_torch, "bar": bar}))


def _check_forward(name, seq_cpu, x_cpu, region=None):
    import copy

    y64 = _oracle(seq_cpu, x_cpu)
    seq = copy.deepcopy(seq_cpu).to(DEV)    # (Module.to moves in place: the caller's CPU module stays on the CPU)
    x = x_cpu.to(DEV)
    with torch.no_grad():
        y_t = seq(x.clone()).cpu().double()    # (the ReLU is in place on GroupNorm's output, not on x; the clone is belt and braces)
        y_h = _native(seq)(x).cpu().double()
    if region is not None:
        y64, y_t, y_h = y64[region], y_t[region], y_h[region]
    e_hip, e_torch = (y_h - y64).abs().max().item(), (y_t - y64).abs().max().item()
    bar = 4 * e_torch + FLOOR
    _report(name, e_hip, e_torch, bar)
    assert e_hip <= bar, f"{name}: e_hip {e_hip:.3e} > 4 * e_torch {e_torch:.3e} + 2^-22 = {bar:.3e}"
    return y_h


@pytest.mark.parametrize("shape", [(2, 64, 8, 8), (1, 64, 13, 19), (2, 64, 24, 40), (1, 64, 64, 96)], ids=lambda s: "x".join(map(str, s)))
def test_forward_parity(shape):
    _check_forward("forward " + "x".join(map(str, shape)), _seeded(3), _input(shape, 5))


def _ring():
    m = torch.zeros(13, 19, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return (slice(None), slice(None), m)


def test_padding_is_applied_after_the_activation():
    """beta = +3 on every channel, small gamma: the activated map is ~3 everywhere, so a kernel that pads x with zeros and THEN normalises
    sees relu(shift) > 0 in the halo where the reference's conv sees 0.  On the outermost ring of [1,64,13,19] the fp64 oracle and the
    fp64 "normalise a zero pad" variant differ by 0.87 (max-abs, this seed) against a bar of about 1e-6."""
    seq, x = _seeded(7, gamma_scale=0.05, beta=3.0), _input((1, 64, 13, 19), 9)
    ring = _ring()
    _check_forward("padding trap, whole image", seq, x)
    _check_forward("padding trap, outer ring", seq, x, region=ring)
    # the gap the trap opens, in fp64: pad x with zeros, normalise with the statistics of the unpadded x, activate, convolve unpadded
    with torch.no_grad():
        d = x.double()
        gn, conv = seq[0], seq[2]
        xg = d.view(1, 32, -1)
        mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
        scale = (gn.weight.double().view(32, 2) / (var.view(32, 1) + gn.eps).sqrt())
        shift = gn.bias.double().view(32, 2) - mean.view(32, 1) * scale
        wrong = torch.relu(nn.functional.pad(d, (1, 1, 1, 1)) * scale.view(1, 64, 1, 1) + shift.view(1, 64, 1, 1))
        wrong = torch.sigmoid(nn.functional.conv2d(wrong, conv.weight.double(), conv.bias.double()))
        gap = (wrong - _oracle(seq, x))[ring].abs().max().item()
    print(f"g2d_final_parity padding-trap gap on the ring (fp64 oracle vs normalised zero pad): {gap:.3e}")
    assert gap > 1e-2


def test_statistics_at_a_large_mean():
    _check_forward("mean 1e4, std 1 at 1x64x24x40", _seeded(11), _input((1, 64, 24, 40), 13, mean=1e4, std=1.0))


def test_deterministic_and_stream_independent():
    seq, x = _seeded(3).to(DEV), _input((2, 64, 24, 40), 5).to(DEV)
    m = _native(seq)
    with torch.no_grad():
        a, b = m(x), m(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = m(x)
        side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


def _grads_native(seq, x, dy, x_grad=True, p_grad=True):
    m = _native(seq)
    for p in m.parameters():
        p.requires_grad_(p_grad)
        p.grad = None
    xin = x.clone().requires_grad_(x_grad)
    m(xin).backward(dy)
    out = [xin.grad] + [p.grad for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias)]
    for p in m.parameters():
        p.requires_grad_(True)
    return out


_GRAD_NAMES = ("dx", "dgamma", "dbeta", "dw", "db")


@pytest.mark.parametrize("shape", [(2, 64, 13, 19), (1, 64, 24, 40)], ids=lambda s: "x".join(map(str, s)))
def test_backward_parity(shape):
    import copy

    seq_cpu, x_cpu = _seeded(17), _input(shape, 19)
    dy_cpu = _input((shape[0], 3) + shape[2:], 23)
    s64 = copy.deepcopy(seq_cpu).double()
    x64 = x_cpu.double().requires_grad_(True)
    s64(x64).backward(dy_cpu.double())
    want = [x64.grad] + [p.grad for p in (s64[0].weight, s64[0].bias, s64[2].weight, s64[2].bias)]

    seq, x, dy = copy.deepcopy(seq_cpu).to(DEV), x_cpu.to(DEV), dy_cpu.to(DEV)
    xt = x.clone().requires_grad_(True)
    seq(xt).backward(dy)
    torch32 = [xt.grad] + [p.grad.clone() for p in (seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias)]
    got = _grads_native(seq, x, dy)
    again = _grads_native(seq, x, dy)
    for name, g, a, t, w in zip(_GRAD_NAMES, got, again, torch32, want):
        assert g is not None and g.shape == w.shape, name
        assert torch.equal(g, a), f"{name}: two runs differ"
        scale = w.abs().max().item()
        e_hip, e_torch = (g.cpu().double() - w).abs().max().item() / scale, (t.cpu().double() - w).abs().max().item() / scale
        bar = 4 * e_torch + FLOOR
        _report(f"backward {'x'.join(map(str, shape))} {name}", e_hip, e_torch, bar)
        assert e_hip <= bar, f"{name}: e_hip {e_hip:.3e} > 4 * e_torch {e_torch:.3e} + 2^-22 = {bar:.3e} (relative to max|{name}|)"

    only_x = _grads_native(seq, x, dy, p_grad=False)
    assert torch.equal(only_x[0], got[0]) and all(g is None for g in only_x[1:])
    only_p = _grads_native(seq, x, dy, x_grad=False)
    assert only_p[0] is None and all(torch.equal(a, b) for a, b in zip(only_p[1:], got[1:]))


def test_from_sequential_shares_parameters():
    seq = _seeded(29).to(DEV)
    m = _native(seq)
    assert m[0].weight is seq[0].weight and m[0].bias is seq[0].bias and m[2].weight is seq[2].weight and m[2].bias is seq[2].bias
    assert list(m.state_dict().keys()) == list(seq.state_dict().keys()) == ["0.weight", "0.bias", "2.weight", "2.bias"]
    fresh = M.G2dFinalConv().to(DEV)
    fresh.load_state_dict(seq.state_dict())
    seq2 = _sequential().to(DEV)
    seq2.load_state_dict(fresh.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(seq.state_dict().values(), seq2.state_dict().values()))
    x = _input((1, 64, 13, 19), 31).to(DEV)
    with torch.no_grad():
        assert torch.equal(fresh(x), m(x))
    # an optimizer built over the ORIGINAL Sequential's parameters steps them through the swapped module
    opt = torch.optim.SGD(seq.parameters(), lr=0.1)
    before = [p.detach().clone() for p in seq.parameters()]
    m(x).square().sum().backward()
    opt.step()
    assert all(not torch.equal(p, b) for p, b in zip(seq.parameters(), before))
    with pytest.raises(TypeError):
        M.G2dFinalConv.from_sequential(nn.Sequential(nn.GroupNorm(32, 64), nn.ReLU(), nn.Conv2d(64, 3, 1), nn.Sigmoid()))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["half", "bfloat16"])
def test_half_models(dtype):
    import copy

    seq = _seeded(37).to(DEV)
    m_half = _native(copy.deepcopy(seq)).to(dtype).eval()
    twin = M.G2dFinalConv().to(DEV).eval()
    twin.load_state_dict({k: v.float() for k, v in m_half.state_dict().items()})    # the half parameters, widened
    x_half = _input((2, 64, 24, 40), 41).to(DEV, dtype)
    with torch.no_grad():
        y = m_half(x_half)
        assert y.dtype == dtype
        assert torch.equal(y, twin(x_half.float()).to(dtype))
        y32 = twin(x_half)                                   # an fp32 module fed a half map: fp32 out, read without a copy
        assert y32.dtype == torch.float32 and torch.equal(y32, twin(x_half.float()))
    mixed = _native(copy.deepcopy(seq)).to(dtype)
    mixed[2].float()
    with pytest.raises(RuntimeError, match="mix dtypes"), torch.no_grad():
        mixed(x_half)
    m_half.train()
    with pytest.raises(RuntimeError, match="training a module whose parameters"):
        m_half(x_half)


def test_switches():
    torch.manual_seed(43)
    g = E.G2d().to(DEV).eval()
    with torch.no_grad():
        g.final_conv[0].weight.uniform_(0.5, 1.5)
        g.final_conv[0].bias.normal_(0.0, 0.5)
    original = g.final_conv
    assert type(original) is nn.Sequential
    x = _input((1, 96, 8, 8), 47).to(DEV)
    keys = list(g.state_dict().keys())
    with torch.no_grad():
        feat = g.upsample3(g.upsample2(g.upsample1(g.res_blocks(M.G2dHead.forward(g, x)))))
        y64 = _oracle(copy_to_cpu(original), feat.cpu())
        y_off = g(x)
        assert g.native_final_conv() is g and isinstance(g.final_conv, M.G2dFinalConv)
        assert list(g.state_dict().keys()) == keys
        y_on = g(x)
        g.native_final_conv(False)
    assert g.final_conv is original
    assert y_on.shape == (1, 3, 64, 64)
    e_hip, e_torch = (y_on.cpu().double() - y64).abs().max().item(), (y_off.cpu().double() - y64).abs().max().item()
    bar = 4 * e_torch + FLOOR
    _report("G2d.native_final_conv 1x96x8x8", e_hip, e_torch, bar)
    assert e_hip <= bar

    gb = gbase.Gbase(appearanceEncoder=nn.Identity(), motionEncoder=nn.Identity(), G2d=g, image_pyramid=nn.Identity())
    assert gb.native_final_conv() is gb and isinstance(g.final_conv, M.G2dFinalConv)
    gb.native_final_conv(False)
    assert g.final_conv is original


def copy_to_cpu(module):
    import copy

    return copy.deepcopy(module).cpu()


def test_c_abi_argument_checks():
    lib = _lib.load()
    P = ctypes.c_void_p
    n, h, w = 1, 8, 8
    x = torch.randn(n, 64, h, w, device=DEV)
    gamma, beta, wt, bias = torch.ones(64, device=DEV), torch.zeros(64, device=DEV), torch.zeros(3, 64, 3, 3, device=DEV), torch.zeros(3, device=DEV)
    sentinel = 123.0
    y = torch.full((n, 3, h, w), sentinel, device=DEV)
    ws_bytes = lib.mphip_g2d_final_workspace_bytes(n, 64, h, w, 32, 0)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=DEV)
    stream = P(torch.cuda.current_stream().cuda_stream)

    def fwd(C=64, G=32, Co=3, xp=x, wsp=ws, wsb=ws_bytes):
        return lib.mphip_g2d_final_fwd(P(xp.data_ptr()) if xp is not None else None, 0, P(gamma.data_ptr()), P(beta.data_ptr()), P(wt.data_ptr()),
                                       P(bias.data_ptr()), P(y.data_ptr()), 0, None, n, C, Co, h, w, G, 1e-5,
                                       P(wsp.data_ptr()) if wsp is not None else None, wsb, stream)

    for kwargs, rc in ((dict(C=48), -1), (dict(G=5), -1), (dict(Co=5), -1), (dict(xp=None), -1), (dict(wsb=ws_bytes - 1), -3), (dict(wsp=None), -3)):
        assert fwd(**kwargs) == rc, kwargs
        assert lib.mphip_last_error(), kwargs
    assert lib.mphip_g2d_final_workspace_bytes(n, 48, h, w, 32, 0) == 0
    bws = lib.mphip_g2d_final_workspace_bytes(n, 64, h, w, 32, 1)
    bw = torch.empty(bws // 4, device=DEV)
    dx, dg, db_, stats = torch.empty_like(x), torch.empty(64, device=DEV), torch.empty(64, device=DEV), torch.zeros(n * 32, 2, device=DEV)
    args = [P(t.data_ptr()) for t in (x, y, y, stats, gamma, beta, wt, dx, dg, db_)] + [None, None]
    assert lib.mphip_g2d_final_bwd(*args, n, 48, 3, h, w, 32, P(bw.data_ptr()), bws, stream) == -1
    assert lib.mphip_g2d_final_bwd(*args, n, 64, 3, h, w, 32, P(bw.data_ptr()), bws - 1, stream) == -3 and b"workspace" in lib.mphip_last_error()
    assert lib.mphip_g2d_final_bwd(*([None] + args[1:]), n, 64, 3, h, w, 32, P(bw.data_ptr()), bws, stream) == -1
    torch.cuda.synchronize()
    assert bool((y == sentinel).all())   # nothing was launched
    with pytest.raises(RuntimeError, match="g2d_final"):
        ops.g2d_final(torch.randn(1, 48, 8, 8, device=DEV), gamma, beta, wt, bias)
    assert ag.G2dFinal is not None
