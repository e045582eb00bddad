"""Informational: Eapp.descriptor, image [B,3,512,512] -> es [B,512] — the torchvision-layout ResNet-50 through layer3
(`custom_resnet50`), the adaptive pool, conv_reduce and fc — with `native_resnet50()` on — its thirteen bottlenecks as
model.BottleneckFused, the 1x1 convs on csrc/conv2d_pw_f16x3.hip, the 3x3 convs on csrc/conv2d_f16x3.hip and csrc/conv2d_s2_f16x3.hip —
against the same call with the switch off (torch fp32, cudnn.benchmark on) on the same box and commit, in the same process, with the
conventions of tools/bench_emtn.py.  Each leg: `warmup` calls, then `runs` calls timed one by one with HIP events; the median is reported.
The legs run off, on, on, off so that neither side always goes first.  B = 1 and B = 8.  One more leg for context: the unswapped net under
torch.autocast(float16).
Then one launch of each distinct 1x1 conv shape of the net at this frame size (B = 1 and B = 8), as the fused block issues it (ReLU and
residual as there, a descriptor of x given, the output's descriptor wanted where the block wants it): ms, GB/s of the compulsory bytes —
4 * (Ci * Ho * Wo pixels of x the conv needs + Co * Ho * Wo of y + the same again for a residual) + the packed weights — and TFLOP/s counting
2 * Ci * Co * Ho * Wo per image.  Prints one JSON line; --out also writes it to a file.
usage: python tools/bench_eapp_resnet50.py [--b 1 8] [--warmup 5] [--runs 20] [--out profiles/eapp_resnet50_timing.json]"""
import argparse, json, os, statistics, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from megaportrait_hack_amd import encoders2d as E, model as M, ops


def median_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end))
    return statistics.median(times), min(times)


def commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        r = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        return r.stdout.strip() or os.environ.get("MPHIP_COMMIT", "unknown")
    except OSError:
        return os.environ.get("MPHIP_COMMIT", "unknown")


def pointwise_shapes(hw):
    """(Ci, Co, H = W of the INPUT map, stride, relu, residual, where) of every distinct 1x1 launch of the thirteen blocks: the stem and
    the max-pool leave a 64-channel map of hw / 4."""
    h1, h2, h3 = hw // 4, hw // 8, hw // 16
    return [(64, 64, h1, 1, True, False, "layer1[0].conv1"), (64, 256, h1, 1, True, True, "layer1[*].conv3"),
            (64, 256, h1, 1, False, False, "layer1[0].downsample"), (256, 64, h1, 1, True, False, "layer1[1:].conv1"),
            (256, 128, h1, 1, True, False, "layer2[0].conv1"), (128, 512, h2, 1, True, True, "layer2[*].conv3"),
            (256, 512, h1, 2, False, False, "layer2[0].downsample"), (512, 128, h2, 1, True, False, "layer2[1:].conv1"),
            (512, 256, h2, 1, True, False, "layer3[0].conv1"), (256, 1024, h3, 1, True, True, "layer3[*].conv3"),
            (512, 1024, h2, 2, False, False, "layer3[0].downsample"), (1024, 256, h3, 1, True, False, "layer3[1:].conv1")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs: the median of at least 20 runs is reported")
    dev = torch.device("cuda:0")
    torch.manual_seed(20241018)
    torch.backends.cudnn.benchmark = True
    eapp = E.Eapp().to(dev).eval()
    out = {"what": "Eapp.descriptor: custom_resnet50 (ResNet-50 through layer3: 13 bottlenecks), adaptive pool, conv_reduce, fc",
           "commit": commit(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "H": a.hw, "W": a.hw, "warmup": a.warmup,
           "runs": a.runs, "timer": "HIP events around each call after `warmup` calls; median (and minimum) of `runs` calls, ms per call",
           "cudnn_benchmark": True, "order": ["off", "on", "on", "off"],
           "pointwise_bytes": "4 * (Ci * Ho * Wo + Co * Ho * Wo * (2 with a residual, else 1)) per image + the packed weights once",
           "pointwise_flop": "2 * Ci * Co * Ho * Wo per image", "pointwise": [], "batches": {}}
    with torch.no_grad():
        for b in a.b:
            for ci, co, h, s, relu, with_res, where in pointwise_shapes(a.hw):
                ho = (h + s - 1) // s
                x = torch.randn(b, ci, h, h, device=dev)
                pack = ops.PackedConv2dPW(torch.randn(co, ci, 1, 1, device=dev) * 0.05, torch.zeros(co, device=dev))
                res = torch.randn(b, co, ho, ho, device=dev) if with_res else None
                rng = ops.absmax_range(x)
                want = relu      # (the block wants the descriptor of y1 and of its output; the downsample's feeds an epilogue)
                med, best = median_ms(lambda: ops.conv2d_pw(x, pack, residual=res, relu=relu, stride=s, x_range=rng, want_range=want),
                                      a.warmup, a.runs)
                nbytes = 4 * b * (ci + co * (2 if with_res else 1)) * ho * ho + pack.packed().numel() * 4
                flop = 2.0 * b * ci * co * ho * ho
                out["pointwise"].append({"N": b, "Ci": ci, "Co": co, "H": h, "W": h, "stride": s, "relu": relu, "residual": with_res,
                                         "where": where, "ms": round(med, 4), "min_ms": round(best, 4), "gbs": round(nbytes / med * 1e-6, 1),
                                         "tflops": round(flop / med * 1e-9, 2)})
                del x, pack, res
        for b in a.b:
            x = torch.rand(b, 3, a.hw, a.hw, device=dev) * 2 - 1
            legs = []
            for on in (False, True, True, False):
                M.native_eapp_resnet50(eapp, on)
                med, best = median_ms(lambda: eapp.descriptor(x), a.warmup, a.runs)
                legs.append({"native_resnet50": on, "median_ms": round(med, 4), "min_ms": round(best, 4)})
            eapp.native_resnet50(True)
            es_on = eapp.descriptor(x)
            eapp.native_resnet50(False)
            es_off = eapp.descriptor(x)
            with torch.autocast(device_type="cuda", dtype=torch.float16):
                amp, amp_best = median_ms(lambda: eapp.descriptor(x), a.warmup, a.runs)
            off = statistics.mean(l["median_ms"] for l in legs if not l["native_resnet50"])
            on = statistics.mean(l["median_ms"] for l in legs if l["native_resnet50"])
            out["batches"][str(b)] = {"legs": legs, "off_ms": round(off, 4), "on_ms": round(on, 4), "off_over_on": round(off / on, 3),
                                      "torch_autocast_fp16_ms": round(amp, 4), "torch_autocast_fp16_min_ms": round(amp_best, 4),
                                      "es_on_vs_off_max_abs": (es_on - es_off).abs().max().item(), "es_max_abs_off": es_off.abs().max().item()}
            del x
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
