"""Informational: Eapp's two 7x7 stems at image [B,3,512,512] with `native_stems()` on — `conv` as model.ConvStem7Fused and
`custom_resnet50`'s conv1-bn1-relu-maxpool as model.Stem7Fused, one launch of csrc/conv2d_stem7_f16x3.hip each — against the same calls
with the switch off (torch fp32, cudnn.benchmark on) on the same box and commit, in the same process, with the conventions of
tools/bench_eapp_resnet50.py.  Each leg: `warmup` calls, then `runs` calls timed one by one with HIP events; the median is reported.  The
legs run off, on, on, off so that neither side always goes first.  B = 1 and B = 8.  What is timed:
  conv_stem      Eapp.conv alone (7x7, stride 1, bias; 64 channels at full resolution)
  resnet_stem    maxpool(relu(bn1(conv1(x)))) of custom_resnet50 alone (7x7, stride 2, BatchNorm, ReLU, max-pool)
  trunk2d        Eapp.trunk2d with native_trunk() on, with and without the stems: the fused resblock_128 then finds a descriptor on its
                 input and does not scan the 64-channel map
  descriptor     Eapp.descriptor with native_resnet50() on, with and without the stems
and, for context, the two stems alone with the switch off under torch.autocast(float16).  The two stems alone also report GB/s of the
compulsory bytes of a launch: 4 * (3 * H * W of x + 64 * Hy * Wy of y) per image + the packed weights.  No threshold: the numbers are
what they are.  Prints one JSON line; --out also writes it to a file.
usage: python tools/bench_eapp_stems.py [--b 1 8] [--warmup 5] [--runs 20] [--out profiles/eapp_stems_timing.json]"""
import argparse, json, os, statistics, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
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
    torch.manual_seed(20241020)
    torch.backends.cudnn.benchmark = True
    eapp = E.Eapp().to(dev).eval()
    net = eapp.custom_resnet50
    pack_bytes = ops.PackedConv2dStem7(eapp.conv.weight, eapp.conv.bias).packed().numel() * 4
    out = {"what": "Eapp's two 7x7 stems: conv (stride 1, bias) and custom_resnet50's conv1-bn1-relu-maxpool (stride 2), alone and inside "
                   "Eapp.trunk2d (native_trunk on) and Eapp.descriptor (native_resnet50 on)",
           "commit": commit(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "H": a.hw, "W": a.hw, "warmup": a.warmup,
           "runs": a.runs, "timer": "HIP events around each call after `warmup` calls; median (and minimum) of `runs` calls, ms per call",
           "cudnn_benchmark": True, "order": ["off", "on", "on", "off"],
           "stem_bytes": "4 * (3 * H * W + 64 * Hy * Wy) per image + the packed weights once",
           "image_scan": "the descriptor of the image rides on it in every leg; the one scan per new image (image_scan_ms) is not in the "
                         "other figures", "batches": {}}
    stem = lambda x: net.maxpool(F.relu(net.bn1(net.conv1(x))))
    with torch.no_grad():
        for b in a.b:
            x = torch.rand(b, 3, a.hw, a.hw, device=dev) * 2 - 1
            ops.absmax_range(x)      # the image's descriptor rides on it, as it does after the first stem of a forward
            calls = {"conv_stem": (lambda: eapp.conv(x), None), "resnet_stem": (lambda: stem(x), None),
                     "trunk2d": (lambda: eapp.trunk2d(x), eapp.native_trunk), "descriptor": (lambda: eapp.descriptor(x), eapp.native_resnet50)}
            scan, scan_best = median_ms(lambda: ops.absmax_range(x), a.warmup, a.runs)
            rec = {"image_scan_ms": round(scan, 4), "image_scan_min_ms": round(scan_best, 4)}
            for name, (fn, other) in calls.items():
                if other:
                    other(True)
                legs = []
                for on in (False, True, True, False):
                    M.native_eapp_stems(eapp, on)
                    med, best = median_ms(fn, a.warmup, a.runs)
                    legs.append({"native_stems": on, "median_ms": round(med, 4), "min_ms": round(best, 4)})
                M.native_eapp_stems(eapp, True)
                y_on = fn()
                M.native_eapp_stems(eapp, False)
                y_off = fn()
                if other:
                    other(False)
                off = statistics.mean(l["median_ms"] for l in legs if not l["native_stems"])
                on = statistics.mean(l["median_ms"] for l in legs if l["native_stems"])
                rec[name] = {"legs": legs, "off_ms": round(off, 4), "on_ms": round(on, 4), "off_over_on": round(off / on, 3),
                             "on_vs_off_max_abs": (y_on - y_off).abs().max().item(), "max_abs_off": y_off.abs().max().item()}
                if name in ("conv_stem", "resnet_stem"):
                    nbytes = 4 * (x.numel() + y_on.numel()) + pack_bytes
                    rec[name]["compulsory_bytes"] = nbytes
                    rec[name]["on_gbs"] = round(nbytes / on * 1e-6, 1)
                    rec[name]["tflops_on"] = round(2.0 * 147 * 64 * b * (a.hw // (1 if name == "conv_stem" else 2)) ** 2 / on * 1e-9, 2)
                    with torch.autocast(device_type="cuda", dtype=torch.float16):
                        amp, amp_best = median_ms(fn, a.warmup, a.runs)
                    rec[name]["torch_autocast_fp16_ms"], rec[name]["torch_autocast_fp16_min_ms"] = round(amp, 4), round(amp_best, 4)
                del y_on, y_off
            out["batches"][str(b)] = rec
            del x
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
