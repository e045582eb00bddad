"""The four C entries of the 2-D 3x3 conv (mphip_conv2d_fwd, mphip_conv2d_cat_fwd, mphip_conv2d_fwd_typed, mphip_conv2d_cat_fwd_typed) share
one host routine (conv2d_run, csrc/conv2d_lp.hip): one table of the shared rules, applied to every entry, and on the GPU the same bits
from all four for an fp32, three-product call."""
import ctypes

import pytest
import torch

from megaportrait_hack_amd import _lib

F32 = 0


def _entries(lib):
    """name -> call(**arguments) with one vocabulary: x1, r1 (its descriptor), c1, x2, r2, c2, wp, b, res, y, out, n, co, h, w, ws, wsb,
    stream.  The plain entries take no second source; the typed ones are called with fp32 maps and `products`."""
    def plain(a):
        assert a["x2"] is None and a["c2"] == 0 and a["r2"] is None
        return lib.mphip_conv2d_fwd(a["x1"], a["r1"], a["wp"], a["b"], a["res"], a["y"], a["out"], a["n"], a["c1"], a["co"], a["h"], a["w"], 0,
                                    a["ws"], a["wsb"], a["stream"])

    def cat(a):
        return lib.mphip_conv2d_cat_fwd(a["x1"], None, 0, a["r1"], a["c1"], a["x2"], None, 0, a["r2"], a["c2"], a["wp"], a["b"], a["res"], a["y"],
                                        a["out"], a["n"], a["co"], a["h"], a["w"], 0, a["ws"], a["wsb"], a["stream"])

    def plain_typed(a):
        assert a["x2"] is None and a["c2"] == 0 and a["r2"] is None
        return lib.mphip_conv2d_fwd_typed(a["x1"], F32, a["r1"], a["wp"], a["b"], a["res"], F32, a["y"], F32, a["out"], a["n"], a["c1"], a["co"],
                                          a["h"], a["w"], 0, a["products"], a["ws"], a["wsb"], a["stream"])

    def cat_typed(a):
        return lib.mphip_conv2d_cat_fwd_typed(a["x1"], F32, None, 0, a["r1"], a["c1"], a["x2"], None, 0, a["r2"], a["c2"], a["wp"], a["b"],
                                              a["res"], F32, a["y"], F32, a["out"], a["n"], a["co"], a["h"], a["w"], 0, a["products"], a["ws"],
                                              a["wsb"], a["stream"])

    return {"conv2d_fwd": plain, "conv2d_cat_fwd": cat, "conv2d_fwd_typed": plain_typed, "conv2d_cat_fwd_typed": cat_typed}


def test_every_shared_rule_is_refused_by_every_entry_without_a_gpu():
    """Host pointers that are never dereferenced: every refusal happens before the first HIP call.  The typed entries are called with one
    product, so that they answer under their own name (with three they are the fp32 entries, tests/test_conv2d_lp_host.py)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(5 << 14)
    base = (ctypes.addressof(buf) + 15) & ~15
    x1, x2, y, res, ws = (ctypes.c_void_p(base + i * 16384) for i in range(5))          # five disjoint 16 KiB regions
    off = lambda p, k: ctypes.c_void_p(p.value + k)
    err = lib.mphip_last_error
    EINVAL, EWORKSPACE = -1, -3
    one = 4100 * 4                                                                      # bytes of one range descriptor

    rules = [  # (substring of the message, return code, arguments that break the rule, ... and those only a second source can break)
        (b"null pointer", EINVAL, [dict(x1=None), dict(wp=None), dict(b=None), dict(y=None)], []),
        (b"unsupported shape", EINVAL, [dict(c1=8), dict(c1=24), dict(co=48), dict(co=16), dict(h=0), dict(w=0), dict(n=0)], [dict(c2=24)]),
        (b"aligned", EINVAL, [dict(x1=off(x1, 2)), dict(y=off(y, 2)), dict(res=off(res, 2)), dict(wp=off(x1, 4))], [dict(x2=off(x2, 2))]),
        (b"must not alias", EINVAL, [dict(y=x1), dict(y=off(x1, 64)), dict(res=y), dict(res=off(y, 64))], [dict(y=x2), dict(y=off(x2, 64))]),
        (b"workspace", EWORKSPACE, [dict(r1=None, wsb=one - 1), dict(r1=None, ws=None, wsb=0), dict(r1=None, ws=None)],
         [dict(r2=None, wsb=one - 1), dict(r1=None, r2=None, wsb=2 * one - 1)]),
    ]
    for name, call in _entries(lib).items():
        two = "cat" in name
        good = dict(x1=x1, r1=x1, c1=16, x2=x2 if two else None, r2=x2 if two else None, c2=16 if two else 0, wp=x1, b=x1, res=res, y=y,
                    out=None, n=1, co=32, h=4, w=4, ws=ws, wsb=1 << 20, stream=None, products=1)
        named = lambda: err().startswith(name.encode() + b":")                         # the message names the called entry
        for message, code, cases, second_source in rules:
            for bad in cases + (second_source if two else []):
                assert call({**good, **bad}) == code and message in err() and named(), (name, bad, err())
                if code == EINVAL:                                                      # ... and an argument error wins over the workspace's
                    assert call({**good, **bad, "r1": None, "ws": None, "wsb": 0}) == EINVAL and message in err() and named(), (name, bad, err())
        # (the workspace's own alignment is looked at once it is known to be large enough)
        assert call({**good, "r1": None, "ws": off(ws, 2)}) == EINVAL and b"aligned" in err() and named(), (name, err())


@pytest.mark.gpu
def test_the_four_entries_give_the_same_bits_for_an_fp32_three_product_call():
    """N=1, Ci=16, Co=32, H=W=17: one full and one partial tile in each direction, one K chunk.  The typed entries with products=3, the
    two-source ones with C2=0: equal y and equal out_range descriptors, with the caller's descriptor of x and with a scan."""
    from megaportrait_hack_amd import ops

    dev = "cuda:0"
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    n, ci, co, h, w = 1, 16, 32, 17, 17
    x = torch.randn(n, ci, h, w, generator=g).to(dev)
    res = torch.randn(n, co, h, w, generator=g).to(dev)
    pack = ops.PackedConv2d((torch.randn(co, ci, 3, 3, generator=g) / 12.0).to(dev), (torch.randn(co, generator=g) * 0.1).to(dev))
    wp = pack.packed()
    ws = torch.empty(lib.mphip_conv2d_cat_workspace_bytes(n, ci, 0, co, h, w) // 4, dtype=torch.float32, device=dev)
    descriptor = torch.zeros(4100, dtype=torch.float32)
    descriptor[2] = 8.0                                            # derive mode, bound 8 >= max|x|, no partial maxima
    descriptor = descriptor.to(dev)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for r1 in (descriptor, None):
        got = {}
        for name, call in _entries(lib).items():
            y, out = torch.full((n, co, h, w), float("nan"), device=dev), ops.new_range(dev)
            rc = call(dict(x1=P(x), r1=P(r1), c1=ci, x2=None, r2=None, c2=0, wp=P(wp), b=P(pack.bias), res=P(res), y=P(y), out=P(out), n=n, co=co,
                           h=h, w=w, ws=P(ws), wsb=ws.numel() * 4, stream=stream, products=3))
            assert rc == 0, (name, lib.mphip_last_error())
            got[name] = (y, out)
        y0, out0 = got["conv2d_fwd"]
        assert torch.isfinite(y0).all() and int(out0[3:4].view(torch.int32).item()) == 4     # 2 x 2 tiles x one 64-channel tile
        for name, (y, out) in got.items():
            assert torch.equal(y, y0), (name, r1 is None)
            assert torch.equal(out[:8].view(torch.int32), out0[:8].view(torch.int32)), (name, r1 is None)
        assert float(out0[4:8].max()) == float(y0.abs().max())
