"""The fused ResNet-18 stem kernel (csrc/conv2d_stem.hip: mphip_conv2d_stem_supported, mphip_conv2d_stem_fwd; ops.conv2d_stem), with the
conventions of tests/test_gpu_conv2d_s2.py.

Integer data makes every product and partial sum an exact fp32 value (|sum| <= 27 * 8 + 8), so those cases are compared with torch.equal
against the fp64 oracle max_pool2d(relu(conv2d(x, w, b, padding=1)), 3, 2, 1).  On random data the contract of include/mphip.h leaves no
freedom — a fixed fmaf order, one rounded + bias, an exact max — so the output is compared as int32 bit patterns with a plain-C statement
of it (tests/c_abi/stem_ref.c, compiled here with gcc -ffp-contract=off).  Random data is also held to the project's conv bar
4 * e_torch + 2^-21 * A (A = max over conv outputs of sum |w||x| + |bias|) against torch's fp32 conv -> relu -> max_pool2d on the same GPU."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANGE_FLOATS = 4100
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_ROWS, TILE_COLS = 8, 63            # pooled rows and columns of one workgroup (csrc/conv2d_stem.hip: 4 waves x 2 rows, 63 lanes)
CROSS = (1, 48, 2 * TILE_ROWS + 1, 2 * TILE_COLS + 1)     # Ho = 9, Wo = 64: two tile rows, two tile columns; Co no multiple of 32
COMBOS = [(relu, pool) for relu in (False, True) for pool in (False, True)]


def _lib():
    from megaportrait_hack_amd import _lib as L

    return L.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _oracle(x, w, b, relu, pool):
    y = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    y = F.relu(y) if relu else y
    return F.max_pool2d(y, 3, 2, 1) if pool else y


def _misaligned(t):
    """The same values at a base pointer 4 bytes past a 16-byte boundary."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = big[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _range_max(rng):
    r = rng.view(torch.int32)
    n = int(r[3].item())
    assert rng[0].item() == 0.0 and 0 < n <= RANGE_FLOATS - 4
    return torch.cat([r[2:3], r[4:4 + n]]).max().view(1).view(torch.float32).item()


# (1,1) and (2,2): one pooled pixel; (5,7): the last pooled row and column see the padding; (4,6): they do not; CROSS: two tile rows and
# columns of the pooled kernel; 33x70: Ho = 17, Wo = 35; 18x131: two tile rows and columns of the kernel without the pool (16 x 128)
INT_CASES = [(1, 16, 1, 1), (1, 16, 2, 2), (2, 16, 5, 7), (1, 16, 4, 6), CROSS, (1, 64, 33, 70), (1, 16, 18, 131)]


@pytest.mark.parametrize("shape,offset", [(s, False) for s in INT_CASES] + [(s, True) for s in INT_CASES[:2]],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("plus4bytes" if v else "aligned"))
def test_integer_data_is_bit_exact(shape, offset):
    from megaportrait_hack_amd import ops

    n, co, h, w = shape
    x, wt, b = _ints((n, 3, h, w), -4, 4, 1), _ints((co, 3, 3, 3), -2, 2, 2), _ints((co,), -8, 8, 3)
    xg, wg, bg = x.to(DEV), wt.to(DEV), b.to(DEV)
    if offset:
        xg, wg, bg = _misaligned(xg), _misaligned(wg), _misaligned(bg)
    for relu, pool in COMBOS:
        assert ops.conv2d_stem_supported(n, 3, co, h, w, pool)
        want = _oracle(x, wt, b, relu, pool).float()
        got = ops.conv2d_stem(xg, wg, bg, relu=relu, pool=pool)
        assert got.shape == want.shape == (n, co, (h + 1) // 2 if pool else h, (w + 1) // 2 if pool else w) and got.dtype == torch.float32
        assert torch.equal(got.cpu(), want), (shape, relu, pool, (got.cpu() - want).abs().max().item())


def test_zero_padding_counts_the_taps():
    from megaportrait_hack_amd import ops

    n, co, h, w = 1, 16, 19, 35
    ones = lambda *s: torch.ones(*s, device=DEV)
    taps = 3 * F.conv2d(torch.ones(1, 1, h, w), torch.ones(1, 1, 3, 3), padding=1)
    assert taps[0, 0, 0, 0] == 12 and taps[0, 0, 0, 1] == 18 and taps[0, 0, 5, 5] == 27 and taps[0, 0, 18, 34] == 12
    y = ops.conv2d_stem(ones(n, 3, h, w), ones(co, 3, 3, 3), torch.zeros(co, device=DEV), relu=False, pool=False).cpu()
    assert torch.equal(y, taps.expand(n, co, h, w))
    yp = ops.conv2d_stem(ones(n, 3, h, w), ones(co, 3, 3, 3), torch.zeros(co, device=DEV), relu=True, pool=True).cpu()
    assert torch.equal(yp, F.max_pool2d(taps, 3, 2, 1).expand(n, co, 10, 18))


@pytest.fixture(scope="module")
def stem_ref(tmp_path_factory):
    """tests/c_abi/stem_ref.c as a shared object: (x, w, b, relu, pool) on the CPU -> y."""
    so = str(tmp_path_factory.mktemp("stem_ref") / "libstem_ref.so")
    subprocess.run(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "c_abi", "stem_ref.c"), "-o", so, "-lm"],
                   check=True)
    fn = ctypes.CDLL(so).stem_ref
    fn.restype, fn.argtypes = None, [ctypes.c_void_p] * 4 + [ctypes.c_int] * 6

    def run(x, w, b, relu, pool):
        n, _, h, wd = x.shape
        co = w.shape[0]
        x, w, b = x.contiguous(), w.contiguous(), b.contiguous()
        y = torch.empty((n, co, (h + 1) // 2 if pool else h, (wd + 1) // 2 if pool else wd))
        fn(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), n, co, h, wd, int(relu), int(pool))
        return y

    return run


@pytest.mark.parametrize("xscale", [1.0, 1e4, 1e-4])
@pytest.mark.parametrize("shape", [(2, 16, 5, 7), (1, 32, 19, 35), CROSS], ids=lambda s: "x".join(map(str, s)))
def test_random_data_has_the_bits_of_the_contract(stem_ref, shape, xscale):
    from megaportrait_hack_amd import ops

    n, co, h, w = shape
    x, wt, b = _rand((n, 3, h, w), 31, xscale), _rand((co, 3, 3, 3), 32, 0.2), _rand((co,), 33, xscale)
    xg, wg, bg = x.to(DEV), wt.to(DEV), b.to(DEV)
    for relu, pool in COMBOS:
        want = stem_ref(x, wt, b, relu, pool)
        got = ops.conv2d_stem(xg, wg, bg, relu=relu, pool=pool).cpu()
        assert got.shape == want.shape
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (shape, xscale, relu, pool, (got - want).abs().max().item())


def test_pooling_is_pooling_bitwise():
    from megaportrait_hack_amd import ops

    n, co, h, w = 2, 64, 37, 50
    x, wt, b = _rand((n, 3, h, w), 41, 2.0).to(DEV), _rand((co, 3, 3, 3), 42, 0.2).to(DEV), _rand((co,), 43).to(DEV)
    for relu in (False, True):
        flat, pooled = ops.conv2d_stem(x, wt, b, relu=relu, pool=False), ops.conv2d_stem(x, wt, b, relu=relu, pool=True)
        assert torch.equal(pooled, F.max_pool2d(flat, 3, 2, 1))
        assert torch.equal(pooled, ops.conv2d_stem(x, wt, b, relu=relu, pool=True))      # and the same bits twice
    xn = x.clone()
    xn[0, 1, 10, 13], xn[1, 2, 36, 49] = float("nan"), float("inf")
    for relu in (False, True):
        flat, pooled = ops.conv2d_stem(xn, wt, b, relu=relu, pool=False), ops.conv2d_stem(xn, wt, b, relu=relu, pool=True)
        want = F.max_pool2d(flat, 3, 2, 1)
        assert bool(flat.isnan().any()) and bool(flat.isinf().any()) and bool(pooled.isinf().any())
        assert 0 < int(want.isnan().sum()) < want.numel() // 4 and torch.equal(pooled.isnan(), want.isnan())
        assert torch.equal(pooled[~want.isnan()], want[~want.isnan()])


def test_ranges_are_exact_and_interchangeable():
    from megaportrait_hack_amd import ops

    lib = _lib()
    n, co, h, w = 2, 64, 37, 50
    x, wt, b = _rand((n, 3, h, w), 21, 3.0).to(DEV), _rand((co, 3, 3, 3), 22, 0.2).to(DEV), _rand((co,), 23).to(DEV)
    w2, b2 = _rand((32, co, 3, 3), 24, 0.1).to(DEV), _rand((32,), 25).to(DEV)
    for relu, pool in COMBOS:
        plain = ops.conv2d_stem(x, wt, b, relu=relu, pool=pool)
        out_range = torch.full((RANGE_FLOATS,), 1.0e30, device=DEV)                   # poisoned: the launch must initialise what it uses
        y = torch.empty_like(plain)
        assert lib.mphip_conv2d_stem_fwd(_p(x), _p(wt), _p(b), _p(y), _p(out_range), n, 3, co, h, w, int(relu), int(pool), _stream()) == 0
        assert torch.equal(y, plain) and _range_max(out_range) == y.abs().max().item()
    # want_range tags the result; the conv2d that follows picks the tag up and writes the bits it writes after scanning y itself
    pack = ops.PackedConv2d(w2, b2)
    yt = ops.conv2d_stem(x, wt, b, want_range=True)
    assert ops.tensor_range(yt) is not None and _range_max(ops.tensor_range(yt)) == yt.abs().max().item()
    untagged = yt.clone()
    assert ops.tensor_range(untagged) is None
    assert torch.equal(ops.conv2d(yt, pack), ops.conv2d(untagged, pack))


@pytest.mark.parametrize("xscale", [1.0, 1e4, 1e-4])
def test_random_data_accuracy(xscale):
    from megaportrait_hack_amd import ops

    n, co, h, w = 2, 64, 64, 64
    x, wt, b = _rand((n, 3, h, w), 11, xscale), _rand((co, 3, 3, 3), 12, 0.2), _rand((co,), 13, xscale)
    y64 = _oracle(x, wt, b, True, True)
    A = F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), padding=1).max().item()
    xg, wg, bg = x.to(DEV), wt.to(DEV), b.to(DEV)
    cudnn = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        yt = F.max_pool2d(F.relu(F.conv2d(xg, wg, bg, padding=1)), 3, 2, 1)
    finally:
        torch.backends.cudnn.allow_tf32 = cudnn
    yh = ops.conv2d_stem(xg, wg, bg)
    e_torch = (yt.cpu().double() - y64).abs().max().item()
    e_hip = (yh.cpu().double() - y64).abs().max().item()
    bound = 4 * e_torch + 2.0 ** -21 * A
    print(f"conv2d_stem parity {(n, co, h, w)} x*{xscale:g}: e_hip={e_hip:.3e} e_torch={e_torch:.3e} A={A:.3e} bound={bound:.3e}")
    assert e_hip <= bound


def test_argument_rules():
    """Each refusal returns its code before anything is launched: y, pre-filled with a sentinel, is untouched."""
    from megaportrait_hack_amd import ops

    lib = _lib()
    t = torch.zeros(1 << 12, device=DEV)
    y = torch.full((1 << 12,), 7.0, device=DEV)
    args = lambda n, ci, co, h, w, x=t, wt=t, b=t, y=y, pool=1: (_p(x), _p(wt), _p(b), _p(y), None, n, ci, co, h, w, 0, pool, _stream())
    for shape in [(1, 1, 64, 8, 8), (1, 4, 64, 8, 8), (1, 16, 64, 8, 8), (1, 3, 8, 8, 8), (1, 3, 24, 8, 8), (1, 3, 16, 0, 8), (0, 3, 16, 8, 8),
                  (1, 3, 16, 1 << 15, 1 << 16)]:
        assert lib.mphip_conv2d_stem_supported(*shape, 1) == 0 and not ops.conv2d_stem_supported(*shape)
        assert lib.mphip_conv2d_stem_fwd(*args(*shape)) == EINVAL and b"conv2d_stem_fwd: unsupported shape" in lib.mphip_last_error()
    ok = (1, 3, 16, 8, 8)      # x: 192 elements; y: 16 x 4 x 4 = 256 pooled, 1024 flat
    assert lib.mphip_conv2d_stem_supported(*ok, 1) == 1
    for missing in ("x", "wt", "b", "y"):
        assert lib.mphip_conv2d_stem_fwd(*args(*ok, **{missing: None})) == EINVAL and b"conv2d_stem_fwd: null" in lib.mphip_last_error()
    assert lib.mphip_conv2d_stem_fwd(*args(*ok, x=y)) == EINVAL and b"must not alias" in lib.mphip_last_error()           # y is x
    assert lib.mphip_conv2d_stem_fwd(*args(*ok, x=y[255:])) == EINVAL and b"must not alias" in lib.mphip_last_error()     # one element shared
    assert lib.mphip_conv2d_stem_fwd(*args(*ok, x=y[1023:], pool=0)) == EINVAL and b"must not alias" in lib.mphip_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert lib.mphip_conv2d_stem_fwd(*args(*ok, x=y[256:])) == 0, lib.mphip_last_error()      # extents from Ho * Wo: these only touch
    torch.cuda.synchronize()
    assert bool((y[256:] == 7.0).all()) and bool((y[:256] == 0.0).all())                      # w = 0, bias = 0: the pooled y is zeros
    for bad in (lambda: ops.conv2d_stem(torch.zeros(1, 3, 8, 8), t[:432].view(16, 3, 3, 3), t[:16]),                      # a CPU image
                lambda: ops.conv2d_stem(torch.zeros(1, 3, 8, 8, device=DEV).half(), t[:432].view(16, 3, 3, 3), t[:16]),   # a half image
                lambda: ops.conv2d_stem(torch.zeros(1, 4, 8, 8, device=DEV), t[:432].view(16, 3, 3, 3), t[:16]),
                lambda: ops.conv2d_stem(torch.zeros(1, 3, 8, 8, device=DEV), t[:216].view(8, 3, 3, 3), t[:8]),
                lambda: ops.conv2d_stem(torch.zeros(1, 3, 8, 8, device=DEV), t[:432].view(16, 3, 3, 3), t[:8])):
        with pytest.raises(RuntimeError):
            bad()
    nhwc = _rand((2, 3, 9, 11), 61).to(DEV)
    wt, b = _rand((16, 3, 3, 3), 62).to(DEV), _rand((16,), 63).to(DEV)
    assert torch.equal(ops.conv2d_stem(nhwc.contiguous(memory_format=torch.channels_last), wt, b), ops.conv2d_stem(nhwc, wt, b))
    torch.cuda.synchronize()
