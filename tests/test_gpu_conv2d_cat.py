"""The two-source, normalise-while-staging 3x3 conv (ops.conv2d_cat over mphip_conv2d_cat_fwd, csrc/conv2d_gn_f16x3.hip; its queries
mphip_conv2d_cat_supported and mphip_conv2d_cat_workspace_bytes are exercised in tests/test_eapp_trunk_host.py as well):
  * the bits of ops.conv2d where the two must agree (no table, one source);
  * the bits of ops.conv2d on the MATERIALISED concatenation [relu(x1 * scale + shift) ; x2] — which fails if a padded pixel is normalised
    instead of left zero, if the chunks of the sources are taken in the wrong order, or if each source takes a scale of its own;
  * the project's accuracy rule for a different summation order against fp64 on the CPU: e_hip <= 4 * e_torch + 2^-22 * max|y64|, e_torch
    the error of stock fp32 PyTorch against the same fp64 result (tests/test_gpu_g2d_body.py);
  * determinism, and the argument checks of the C entry."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GROUPS = {16: 8, 32: 32, 48: 16, 64: 32}      # GroupNorm groups per channel count: 2, 1, 3 and 2 channels per group


def _weights(co, ci, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(co, ci, 3, 3, generator=g) / (3.0 * ci ** 0.5)).to(DEV), (torch.randn(co, generator=g) * 0.1).to(DEV)


def _maps(n, c1, c2, h, w, seed):
    """x1 with a per-channel offset around -1 (its GroupNorm shifts, -mean * rstd, come out mostly positive: relu(shift) != 0), x2 plain."""
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(n, c1, h, w, generator=g) + (-1.0 + 0.5 * torch.randn(c1, generator=g)).view(1, -1, 1, 1)
    x2 = torch.randn(n, c2, h, w, generator=g) * 3.0 + 0.5 if c2 else None
    return x1.to(DEV), None if x2 is None else x2.to(DEV)


def _bound_of(rng):
    """max|.| a derive-mode range descriptor stands for: [2] and the partial maxima [4, 4 + n)."""
    r = rng.cpu()
    assert r[0].item() == 0.0
    n = int(r[3:4].view(torch.int32).item())
    return max(r[2].item(), r[4:4 + n].max().item() if n else 0.0)


def _descriptor(bound):
    """{0, 0, bound, 0}: derive mode, no partial maxima."""
    r = torch.zeros(4100, dtype=torch.float32)
    r[2] = bound
    return r.to(DEV)


@pytest.mark.parametrize("n,c1,co,h,w", [(2, 16, 32, 5, 7), (1, 48, 96, 20, 37), (2, 32, 64, 16, 16)])
def test_one_plain_source_has_the_bits_of_conv2d(n, c1, co, h, w):
    from megaportrait_hack_amd import ops

    pack = ops.PackedConv2d(*_weights(co, c1, 1))
    x1, _ = _maps(n, c1, 0, h, w, 2)
    res = torch.randn(n, co, h, w, device=DEV)
    for residual in (None, res):
        for relu in (False, True):
            want = ops.conv2d(x1, pack, residual=residual, relu=relu)
            assert torch.equal(ops.conv2d_cat(x1, pack, residual=residual, relu=relu), want), (residual is not None, relu)
    want = ops.conv2d(x1, pack, residual=res, relu=True, want_range=True)
    got = ops.conv2d_cat(x1, pack, residual=res, relu=True, want_range=True)
    assert torch.equal(got, want) and ops.tensor_range(got) is not None
    assert _bound_of(ops.tensor_range(got)) == _bound_of(ops.tensor_range(want)) == want.abs().max().item()
    # the descriptor handed in is the one used: same bits as conv2d with it
    d = _descriptor(64.0)
    assert torch.equal(ops.conv2d_cat(x1, pack, x1_range=d), ops.conv2d(x1, pack, x_range=d))


def _activated(x, table, relu):
    a = x * table[:, :, 0, None, None]        # a multiply, then an add: what the kernel does while staging
    a = a + table[:, :, 1, None, None]
    return a.clamp_min(0) if relu else a


@pytest.mark.parametrize("c1,c2,co,h,w,both", [(16, 16, 32, 13, 19, False), (32, 48, 96, 20, 37, False), (64, 0, 64, 9, 33, False),
                                               (16, 32, 64, 1, 1, False), (16, 16, 32, 13, 19, True)])
def test_two_sources_have_the_bits_of_the_materialised_concat(c1, c2, co, h, w, both):
    from megaportrait_hack_amd import ops

    n = 2
    pack = ops.PackedConv2d(*_weights(co, c1 + c2, 3))
    x1, x2 = _maps(n, c1, c2, h, w, 4)
    tab1, rng1 = ops.gn_relu_table2d(x1, groups=GROUPS[c1])
    assert tuple(tab1.shape) == (n, c1, 2)
    assert (tab1[:, :, 1] > 0).sum().item() * 4 >= tab1[:, :, 1].numel()       # relu(shift) != 0 on at least a quarter of the channels
    parts, bound = [_activated(x1, tab1, True)], _bound_of(rng1)
    kw = {}
    if c2 and both:
        tab2, rng2 = ops.gn_relu_table2d(x2, groups=GROUPS[c2])
        parts.append(_activated(x2, tab2, False))
        bound = max(bound, _bound_of(rng2))
        kw = dict(x2=x2, affine2=tab2, relu2=False, x2_range=rng2)
    elif c2:
        parts.append(x2)
        bound = max(bound, x2.abs().max().item())
        kw = dict(x2=x2, x2_range=_descriptor(x2.abs().max().item()))
    ops.f16x3_saturation_count(reset=True)
    res = torch.randn(n, co, h, w, device=DEV)
    for residual, relu in ((None, False), (res, True)):
        want = ops.conv2d(torch.cat(parts, 1).contiguous(), pack, residual=residual, relu=relu, x_range=_descriptor(bound))
        got = ops.conv2d_cat(x1, pack, affine1=tab1, relu1=True, x1_range=rng1, residual=residual, relu=relu, **kw)
        ring = lambda y: torch.cat([y[..., 0, :].flatten(), y[..., -1, :].flatten(), y[..., :, 0].flatten(), y[..., :, -1].flatten()])
        assert torch.equal(ring(got), ring(want)), "the border ring: padding must stay zero in the activated map"
        assert torch.equal(got, want)
    assert ops.f16x3_saturation_count() == 0


def _rule(name, y_hip, y_torch, y64):
    e_hip = (y_hip.cpu().double() - y64).abs().max().item()
    e_torch = (y_torch.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -22 * y64.abs().max().item()
    print(f"conv2d_cat parity {name}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} max|y64|={y64.abs().max().item():.3e} bound={bound:.3e}")
    assert e_hip <= bound, (name, e_hip, bound)


@pytest.mark.parametrize("n,c1,c2,co,h,w", [(2, 32, 48, 96, 20, 37), (1, 16, 16, 32, 13, 19)])
def test_accuracy_rule_against_fp64(n, c1, c2, co, h, w):
    from megaportrait_hack_amd import ops

    wt, b = _weights(co, c1 + c2, 5)
    pack = ops.PackedConv2d(wt, b)
    x1, x2 = _maps(n, c1, c2, h, w, 6)
    g = GROUPS[c1]
    y64 = F.conv2d(torch.cat([F.relu(F.group_norm(x1.cpu().double(), g)), x2.cpu().double()], 1), wt.cpu().double(), b.cpu().double(), padding=1)
    y_torch = F.conv2d(torch.cat([F.relu(F.group_norm(x1, g)), x2], 1), wt, b, padding=1)
    ops.f16x3_saturation_count(reset=True)
    tab, rng = ops.gn_relu_table2d(x1, groups=g)
    _rule(f"{(n, c1, c2, co, h, w)} table bound {_bound_of(rng):.1f}", ops.conv2d_cat(x1, pack, x2=x2, affine1=tab, relu1=True, x1_range=rng), y_torch, y64)
    if c1 == 32:
        # the bound sqrt(2 * 512^2) = 724.1 that the first block of Eapp's trunk meets at full size (64 channels in 32 groups at 512x512)
        _rule(f"{(n, c1, c2, co, h, w)} bound 724.1", ops.conv2d_cat(x1, pack, x2=x2, affine1=tab, relu1=True, x1_range=_descriptor(724.1)), y_torch, y64)
    assert ops.f16x3_saturation_count() == 0


def test_same_call_twice_gives_the_same_bits():
    from megaportrait_hack_amd import ops

    pack = ops.PackedConv2d(*_weights(96, 80, 7))
    x1, x2 = _maps(2, 32, 48, 20, 37, 8)
    tab, rng = ops.gn_relu_table2d(x1)
    tab_again, rng_again = ops.gn_relu_table2d(x1)
    assert torch.equal(tab, tab_again) and _bound_of(rng) == _bound_of(rng_again)
    run = lambda: ops.conv2d_cat(x1, pack, x2=x2, affine1=tab, relu1=True, x1_range=rng, want_range=True)
    a, b = run(), run()
    assert torch.equal(a, b) and _bound_of(ops.tensor_range(a)) == _bound_of(ops.tensor_range(b))


def test_the_c_entry_refuses_bad_arguments_before_any_launch():
    from megaportrait_hack_amd import _lib, ops

    lib = _lib.load()
    n, c1, c2, co, h, w = 1, 16, 16, 32, 6, 5
    pack = ops.PackedConv2d(*_weights(co, c1 + c2, 9))
    wp = pack.packed()
    x1, x2 = _maps(n, c1, c2, h, w, 10)
    tab, rng = ops.gn_relu_table2d(x1, groups=8)
    ws = torch.empty(lib.mphip_conv2d_cat_workspace_bytes(n, c1, c2, co, h, w) // 4, dtype=torch.float32, device=DEV)
    y = torch.full((n, co, h, w), -7.0, device=DEV)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(x1=x1, aff1=tab, r1=rng, c1=c1, x2=x2, c2=c2, wp=wp, y=y, co=co):
        return lib.mphip_conv2d_cat_fwd(P(x1), P(aff1), 1, P(r1), c1, P(x2), None, 0, None, c2, P(wp), P(pack.bias), None, P(y), None, n, co, h, w, 0,
                                        P(ws), ws.numel() * 4, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    for what, kwargs, message in [("a table without a descriptor", dict(r1=None), b"affine1 without x1_range"),
                                  ("C2 % 16 != 0", dict(c2=24), b"unsupported shape"),
                                  ("Co % 32 != 0", dict(co=48), b"unsupported shape"),
                                  ("y aliasing x2", dict(y=x2), b"must not alias"),
                                  ("a null w_packed", dict(wp=None), b"null pointer")]:
        assert call(**kwargs) == -1, what                    # MPHIP_EINVAL
        assert message in lib.mphip_last_error(), (what, lib.mphip_last_error())
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and torch.equal(x2, _maps(n, c1, c2, h, w, 10)[1])      # nothing ran
    assert call() == 0                                                                     # and the good call does
    assert torch.equal(y, ops.conv2d_cat(x1, pack, x2=x2, affine1=tab, relu1=True, x1_range=rng))
    with pytest.raises(RuntimeError, match="affine1 without x1_range"):                   # the wrapper passes the refusal on
        ops.conv2d_cat(x1, pack, x2=x2, affine1=tab, relu1=True)
