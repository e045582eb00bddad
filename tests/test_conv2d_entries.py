"""The nine forward C entries of the 2-D 3x3 conv (mphip_conv2d_fwd, mphip_conv2d_cat_fwd, their _typed forms, mphip_conv2d_s2_fwd,
mphip_conv2d_up2_fwd, mphip_conv2d_resup2_fwd, mphip_conv2d_grouped_fwd, mphip_conv2d_split_fwd) share one host routine (conv2d_run,
csrc/conv2d_run.hip): one table of the shared rules, applied to every entry; every refusal of every entry, return code and message,
compared with a recording of the library before the routine read a table of forms (tests/golden/conv2d_refusals.json); and on the GPU
the same bits from the six entries that document an fp32, three-product, stride-1, one-group, unsplit call as "that path"."""
import ctypes
import json
import os

import pytest
import torch

from megaportrait_hack_amd import _lib

F32, F16, BF16 = 0, 1, 2
EINVAL, EWORKSPACE = -1, -3
ONE = 4100 * 4                                                                          # bytes of one range descriptor
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv2d_refusals.json")
PARENT = "80c025d"                                                                      # the commit the fixture was recorded from


def _entries(lib):
    """name -> call(**arguments) with one vocabulary: x1, r1 (its descriptor), c1, x2, r2, c2, wp, b, res, y, out, n, co, h, w, ws, wsb,
    stream, and groups / splits for the two entries that take them.  The one-source entries take no second source; the typed ones are
    called with `products` and, where the arguments name them, with the dtype codes xdt / rdt / ydt and the tables aff1 / aff2 (fp32
    maps and no tables otherwise)."""
    def one_source(fn, *counts):                                                        # (counts: what the entry takes after W)
        def call(a):
            assert a["x2"] is None and a["c2"] == 0 and a["r2"] is None
            return fn(a["x1"], a["r1"], a["wp"], a["b"], a["res"], a["y"], a["out"], a["n"], a["c1"], a["co"], a["h"], a["w"],
                      *(a[k] for k in counts), 0, a["ws"], a["wsb"], a["stream"])
        return call

    def cat(a):
        return lib.mphip_conv2d_cat_fwd(a["x1"], a.get("aff1"), 0, a["r1"], a["c1"], a["x2"], a.get("aff2"), 0, a["r2"], a["c2"], a["wp"], a["b"],
                                        a["res"], a["y"], a["out"], a["n"], a["co"], a["h"], a["w"], 0, a["ws"], a["wsb"], a["stream"])

    def plain_typed(a):
        assert a["x2"] is None and a["c2"] == 0 and a["r2"] is None
        return lib.mphip_conv2d_fwd_typed(a["x1"], a.get("xdt", F32), a["r1"], a["wp"], a["b"], a["res"], a.get("rdt", F32), a["y"],
                                          a.get("ydt", F32), a["out"], a["n"], a["c1"], a["co"], a["h"], a["w"], 0, a["products"], a["ws"],
                                          a["wsb"], a["stream"])

    def cat_typed(a):
        return lib.mphip_conv2d_cat_fwd_typed(a["x1"], a.get("xdt", F32), a.get("aff1"), 0, a["r1"], a["c1"], a["x2"], a.get("aff2"), 0, a["r2"],
                                              a["c2"], a["wp"], a["b"], a["res"], a.get("rdt", F32), a["y"], a.get("ydt", F32), a["out"], a["n"],
                                              a["co"], a["h"], a["w"], 0, a["products"], a["ws"], a["wsb"], a["stream"])

    return {"conv2d_fwd": one_source(lib.mphip_conv2d_fwd), "conv2d_cat_fwd": cat, "conv2d_fwd_typed": plain_typed,
            "conv2d_cat_fwd_typed": cat_typed, "conv2d_s2_fwd": one_source(lib.mphip_conv2d_s2_fwd),
            "conv2d_up2_fwd": one_source(lib.mphip_conv2d_up2_fwd), "conv2d_resup2_fwd": one_source(lib.mphip_conv2d_resup2_fwd),
            "conv2d_grouped_fwd": one_source(lib.mphip_conv2d_grouped_fwd, "groups"),
            "conv2d_split_fwd": one_source(lib.mphip_conv2d_split_fwd, "groups", "splits")}


class _Host:
    """Host pointers that are never dereferenced (every refusal happens before the first HIP call): five disjoint 64 KiB regions, the
    valid call of every entry on them, and the table of the shared rules.
    The valid call: N=1, C1=64, Co=128, H=W=4, groups=2, splits=2 (two 16-channel chunks per group, one per split; 64 output channels
    per group); the typed entries with one product, so that they answer under their own name (with three they are the fp32 entries,
    tests/test_conv2d_lp_host.py)."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(6 << 16)
        base = (ctypes.addressof(self.buf) + 15) & ~15
        self.x1, self.x2, self.y, self.res, self.ws = (ctypes.c_void_p(base + i * 65536) for i in range(5))
        self.y_bytes = 128 * 4 * 4 * 4                                                  # of y on the map of x
        self.parts = 2 * self.y_bytes                                                   # the split entry's two partial maps

    @staticmethod
    def off(p, k):
        return ctypes.c_void_p(p.value + k)

    def good(self, name):
        two = "cat" in name
        return dict(x1=self.x1, r1=self.x1, c1=64, x2=self.x2 if two else None, r2=self.x2 if two else None, c2=16 if two else 0, wp=self.x1,
                    b=self.x1, res=self.res, y=self.y, out=None, n=1, co=128, h=4, w=4, ws=self.ws, wsb=1 << 20, stream=None, products=1,
                    groups=2, splits=2)

    def rules(self, name):
        """In the order conv2d_run checks them: (substring of the message, return code, the arguments that break the rule for every
        entry, {entry name, or "two sources": those that break it there only}).  What differs per entry is written here: resup2 also needs
        a residual and even H, W; up2's residual and y live on the doubled map (a residual right behind the y of the other entries lies
        inside up2's); the split entry's workspace also holds its partial maps, with or without a descriptor to compute."""
        x1, x2, y, res, off = self.x1, self.x2, self.y, self.res, self.off
        more = self.parts if name == "conv2d_split_fwd" else 0                          # workspace bytes besides the descriptors
        return [
            (b"null pointer", EINVAL, [dict(x1=None), dict(wp=None), dict(b=None), dict(y=None)], {"conv2d_resup2_fwd": [dict(res=None)]}),
            (b"unsupported shape", EINVAL, [dict(c1=8), dict(c1=24), dict(co=48), dict(co=16), dict(h=0), dict(w=0), dict(n=0)],
             {"two sources": [dict(c2=24)],
              "conv2d_grouped_fwd": [dict(groups=0), dict(groups=-1), dict(groups=3)],
              "conv2d_split_fwd": [dict(groups=0), dict(groups=-1), dict(groups=3), dict(splits=0), dict(splits=-1), dict(splits=3),
                                   dict(splits=17)]}),
            (b"even extents", EINVAL, [], {"conv2d_resup2_fwd": [dict(h=5), dict(w=3), dict(h=3, w=3)]}),
            (b"aligned", EINVAL, [dict(x1=off(x1, 2)), dict(y=off(y, 2)), dict(res=off(res, 2)), dict(wp=off(x1, 4))],
             {"two sources": [dict(x2=off(x2, 2))]}),
            (b"must not alias", EINVAL, [dict(y=x1), dict(y=off(x1, 64)), dict(res=y), dict(res=off(y, 64))],
             {"two sources": [dict(y=x2), dict(y=off(x2, 64))], "conv2d_up2_fwd": [dict(res=off(y, self.y_bytes))]}),
            (b"workspace", EWORKSPACE, [dict(r1=None, wsb=ONE + more - 1), dict(r1=None, ws=None, wsb=0), dict(r1=None, ws=None)],
             {"two sources": [dict(r2=None, wsb=ONE - 1), dict(r1=None, r2=None, wsb=2 * ONE - 1)],
              "conv2d_split_fwd": [dict(wsb=more - 1), dict(ws=None, wsb=0)]}),
        ]

    def breaks(self, name):
        """-> [(rank of the rule, message, code, arguments)] for one entry"""
        keys = (name, "two sources") if "cat" in name else (name,)
        return [(rank, message, code, bad) for rank, (message, code, cases, only) in enumerate(self.rules(name))
                for bad in cases + [b for k in keys for b in only.get(k, [])]]


NO_WORKSPACE = dict(r1=None, ws=None, wsb=0)


def test_every_shared_rule_is_refused_by_every_entry_without_a_gpu():
    """Every break of the rule table through every entry: the rule's return code and message, under the entry's name."""
    lib, host = _lib.load(), _Host()
    err = lib.mphip_last_error
    for name, call in _entries(lib).items():
        good = host.good(name)
        named = lambda: err().startswith(name.encode() + b":")                         # the message names the called entry
        for _, message, code, bad in host.breaks(name):
            assert call({**good, **bad}) == code and message in err() and named(), (name, bad, err())
            if code == EINVAL:                                                          # ... and an argument error wins over the workspace's
                assert call({**good, **bad, **NO_WORKSPACE}) == EINVAL and message in err() and named(), (name, bad, err())
        # (the workspace's own alignment is looked at once it is known to be large enough)
        assert call({**good, "r1": None, "ws": host.off(host.ws, 2)}) == EINVAL and b"aligned" in err() and named(), (name, err())


def _label(bad, host):
    """Arguments -> a stable name: pointers as region+offset, never as addresses."""
    regions = {"x1": host.x1, "x2": host.x2, "y": host.y, "res": host.res, "ws": host.ws}
    def show(v):
        if isinstance(v, ctypes.c_void_p):
            region = max((r for r in regions if regions[r].value <= v.value), key=lambda r: regions[r].value)
            return f"{region}+{v.value - regions[region].value}"
        return repr(v)
    return ",".join(f"{k}={show(v)}" for k, v in bad.items())


def _refusal_matrix(host):
    """-> [(entry name, label, [arguments of a call, the same without a workspace])], a few hundred refused calls.  Per entry: every
    break of the rule table, alone, with the workspace and (an argument error) without one; the first break of every rule paired with the
    first break of the next rule of the entry, with and without the workspace (pairing every break four ways would be some nine hundred
    cases, more than a fixture should hold); then what only some entries
    have: the dtype and product rules of the typed entries, tables without descriptors, x2 without C2 and the reverse.  The group and
    split counts of the grouped and split entries are breaks of the rule table."""
    x1, x2, off = host.x1, host.x2, host.off
    # (unknown codes; products; f16 with bf16; a residual neither fp32 nor y's; not instantiated, or a typed source of the two-source entry;
    # which rule wins; and the name a three-product call reports under)
    typed_only = [dict(xdt=7), dict(rdt=-1), dict(ydt=3), dict(products=2), dict(products=-1), dict(xdt=F16, ydt=BF16), dict(rdt=BF16, ydt=F16),
                  dict(rdt=F16), dict(rdt=BF16, products=3), dict(xdt=F16, ydt=F16), dict(xdt=BF16, ydt=BF16), dict(xdt=F16, products=3),
                  dict(ydt=BF16, products=3), dict(xdt=7, products=2), dict(xdt=F16, ydt=BF16, x1=None), dict(products=3, x1=None),
                  dict(products=3, c1=8), dict(products=3, **NO_WORKSPACE)]
    tables = [dict(aff1=x1, r1=None), dict(aff2=x2, r2=None), dict(aff2=x2, x2=None, c2=0, r2=None), dict(aff1=off(x1, 2)), dict(aff2=off(x2, 1)),
              dict(aff1=x1, r1=None, aff2=x2, r2=None), dict(aff1=x1, r1=None, y=x1)]
    second = [dict(x2=None), dict(c2=0), dict(c2=-16), dict(x2=None, r2=None), dict(x2=None, y=None), dict(c2=0, c1=8)]
    out = []
    for name in _entries(_lib.load()):
        both = lambda bad: (name, _label(bad, host), [bad, {**bad, **NO_WORKSPACE}])
        breaks = host.breaks(name)
        out += [both(bad) if code == EINVAL else (name, _label(bad, host), [bad]) for _, _, code, bad in breaks]
        firsts = {}
        for rank, _, _, bad in breaks:
            firsts.setdefault(rank, bad)
        ranks = sorted(firsts)
        out += [both({**firsts[b], **firsts[a]}) for a, b in zip(ranks, ranks[1:])]
        extra = (typed_only if "typed" in name else []) + (tables + second if "cat" in name else [])
        extra += [dict(xdt=F16), dict(xdt=F16, aff1=x1)] if name == "conv2d_cat_fwd_typed" else []
        out += [(name, _label(bad, host), [bad]) for bad in extra]
    return out


def test_every_refusal_is_the_recorded_one():
    """Return code and whole message of every call of the matrix against tests/golden/conv2d_refusals.json, recorded from the parent
    of the commit that gave conv2d_run its table of forms (the fixture's "recorded_from").  The fixture: "messages", each distinct one
    once, and "refusals"[entry][label] = [return code, index of the message] of the call, followed by the same two of the call without
    a workspace where the matrix makes it.  MPHIP_RECORD_CONV2D_REFUSALS=<path> writes the matrix's answers there instead of comparing
    them: check that commit out, build it, and run this test with the variable set."""
    lib, host = _lib.load(), _Host()
    entries = _entries(lib)
    got = {name: {} for name in entries}
    for name, label, calls in _refusal_matrix(host):
        assert label not in got[name], (name, label)
        got[name][label] = []
        for bad in calls:
            rc = entries[name]({**host.good(name), **bad})
            assert rc != 0, (name, label)
            got[name][label].append((rc, lib.mphip_last_error().decode()))
    path = os.environ.get("MPHIP_RECORD_CONV2D_REFUSALS")
    if path:
        messages = sorted({m for per_entry in got.values() for answers in per_entry.values() for _, m in answers})
        table = {"what": "return code and mphip_last_error() of refused calls of the nine forward entries of the 2-D 3x3 conv "
                         "(tests/test_conv2d_entries.py builds the calls and describes the layout)", "recorded_from": PARENT,
                 "messages": messages,
                 "refusals": {name: {label: [v for rc, m in answers for v in (rc, messages.index(m))] for label, answers in per_entry.items()}
                              for name, per_entry in got.items()}}
        with open(path, "w") as f:
            f.write(json.dumps(table, indent=0, separators=(",", ":")).replace(",\n", ",").replace("[\n", "[").replace("\n]", "]") + "\n")
        return
    with open(GOLDEN) as f:
        table = json.load(f)
    assert table["recorded_from"] == PARENT and list(table["refusals"]) == list(got)
    for name, per_entry in table["refusals"].items():
        assert list(per_entry) == list(got[name]), name
        for label, want in per_entry.items():
            want = [(rc, table["messages"][i]) for rc, i in zip(want[::2], want[1::2])]
            assert got[name][label] == want, (name, label)


@pytest.mark.gpu
def test_the_stride_1_fp32_entries_give_the_same_bits_for_a_three_product_call():
    """N=1, Ci=16, Co=32, H=W=17: one full and one partial tile in each direction, one K chunk.  The typed entries with products=3, the
    two-source ones with C2=0, the grouped one with groups=1 and the split one with groups=1, splits=1: equal y and equal out_range
    descriptors, with the caller's descriptor of x and with a scan."""
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
    same = ("conv2d_fwd", "conv2d_cat_fwd", "conv2d_fwd_typed", "conv2d_cat_fwd_typed", "conv2d_grouped_fwd", "conv2d_split_fwd")
    entries = _entries(lib)
    for r1 in (descriptor, None):
        got = {}
        for name in same:
            y, out = torch.full((n, co, h, w), float("nan"), device=dev), ops.new_range(dev)
            rc = entries[name](dict(x1=P(x), r1=P(r1), c1=ci, x2=None, r2=None, c2=0, wp=P(wp), b=P(pack.bias), res=P(res), y=P(y), out=P(out),
                                    n=n, co=co, h=h, w=w, ws=P(ws), wsb=ws.numel() * 4, stream=stream, products=3, groups=1, splits=1))
            assert rc == 0, (name, lib.mphip_last_error())
            got[name] = (y, out)
        y0, out0 = got["conv2d_fwd"]
        assert torch.isfinite(y0).all() and int(out0[3:4].view(torch.int32).item()) == 4     # 2 x 2 tiles x one 64-channel tile
        for name, (y, out) in got.items():
            assert torch.equal(y, y0), (name, r1 is None)
            assert torch.equal(out[:8].view(torch.int32), out0[:8].view(torch.int32)), (name, r1 is None)
        assert float(out0[4:8].max()) == float(y0.abs().max())
