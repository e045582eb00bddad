"""Informational: Eapp.trunk2d, image [B,3,512,512] -> [B,1536,64,64] (7x7 stem, three ResBlock_Custom 64->128 @512^2, 128->256 @256^2,
256->512 @128^2 with 2x2 average pools, GroupNorm-ReLU-1x1 conv) with `native_trunk()` on — the three blocks as model.ResBlockCustomFused,
two launches of csrc/conv2d_gn_f16x3.hip each — against the same call with the switch off (torch fp32, cudnn.benchmark on) on the same
box and commit, in the same process.  Each leg: `warmup` calls, then `runs` calls timed one by one with HIP events; the median is
reported.  The legs run off, on, on, off so that neither side always goes first.  B = 1 and B = 8.  Two more pairs of legs in the same
process and order discipline, with native_trunk(half_precision=True): torch under autocast-fp16 against the fused trunk under
autocast-fp16, and a .half() Eapp, torch against native; and the one 512->512 conv launch at 128x128 in one product with its TFLOP/s.
Prints one JSON line; --out also writes it to a file.
usage: python tools/bench_eapp_trunk.py [--b 1 8] [--warmup 5] [--runs 20] [--out profiles/eapp_trunk_timing.json]"""
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
    per_frame_gflop = sum(2.0 * 9 * (ci * co * 2 + co * co) * (a.hw >> i) ** 2 for i, (ci, co) in enumerate([(64, 128), (128, 256), (256, 512)])) * 1e-9
    out = {"what": "Eapp.trunk2d: 7x7 stem, ResBlock_Custom 64->128, 128->256, 256->512 with 2x2 average pools, GroupNorm-ReLU-1x1 conv",
           "commit": commit(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "H": a.hw, "W": a.hw, "warmup": a.warmup,
           "runs": a.runs, "timer": "HIP events around each call after `warmup` calls; median (and minimum) of `runs` calls, ms per call",
           "order": ["off", "on", "on", "off"], "resblock_gflop_per_frame": round(per_frame_gflop, 1), "batches": {}}
    eapp_h = E.Eapp().to(dev).eval().half()
    with torch.no_grad():
        # one launch of the last block's second conv shape, 512 -> 512 at 128x128 (B = 1), in three products and in one
        xc = torch.randn(1, 512, a.hw // 4, a.hw // 4, device=dev)
        pk = ops.PackedConv2d(torch.randn(512, 512, 3, 3, device=dev) * 0.02, torch.zeros(512, device=dev))
        rng = ops.absmax_range(xc)
        flop = 2.0 * 9 * 512 * 512 * (a.hw // 4) ** 2
        c3, _ = median_ms(lambda: ops.conv2d(xc, pk, x_range=rng), a.warmup, a.runs)
        c1, _ = median_ms(lambda: ops.conv2d(xc, pk, x_range=rng, products=1), a.warmup, a.runs)
        out["conv_512_512"] = {"H": a.hw // 4, "W": a.hw // 4, "three_products_ms": round(c3, 4), "three_products_tflops": round(flop / c3 * 1e-9, 1),
                               "one_product_ms": round(c1, 4), "one_product_tflops": round(flop / c1 * 1e-9, 1)}
        del xc, pk
        for b in a.b:
            x = torch.rand(b, 3, a.hw, a.hw, device=dev) * 2 - 1
            legs = []
            for on in (False, True, True, False):
                M.native_eapp_trunk(eapp, on)
                med, best = median_ms(lambda: eapp.trunk2d(x), a.warmup, a.runs)
                legs.append({"native_trunk": on, "median_ms": round(med, 4), "min_ms": round(best, 4)})
            eapp.native_trunk(True)
            y_on = eapp.trunk2d(x)
            eapp.native_trunk(False)
            y_off = eapp.trunk2d(x)
            off = statistics.mean(l["median_ms"] for l in legs if not l["native_trunk"])
            on = statistics.mean(l["median_ms"] for l in legs if l["native_trunk"])
            half = {}
            for mode in ("autocast_fp16", "half_module"):
                net = eapp if mode == "autocast_fp16" else eapp_h
                xin = x if mode == "autocast_fp16" else x.half()
                hl = []
                with torch.autocast(device_type="cuda", dtype=torch.float16, enabled=mode == "autocast_fp16"):
                    for on_ in (False, True, True, False):
                        M.native_eapp_trunk(net, on_, half_precision=True)
                        med, best = median_ms(lambda: net.trunk2d(xin), a.warmup, a.runs)
                        hl.append({"native_trunk_half_precision": on_, "median_ms": round(med, 4), "min_ms": round(best, 4)})
                    M.native_eapp_trunk(net, True, half_precision=True)
                    yh_on = net.trunk2d(xin).float()
                    M.native_eapp_trunk(net, False)
                    yh_off = net.trunk2d(xin).float()
                h_off = statistics.mean(l["median_ms"] for l in hl if not l["native_trunk_half_precision"])
                h_on = statistics.mean(l["median_ms"] for l in hl if l["native_trunk_half_precision"])
                half[mode] = {"legs": hl, "off_ms": round(h_off, 4), "on_ms": round(h_on, 4), "off_over_on": round(h_off / h_on, 3),
                              "on_vs_off_max_abs": (yh_on - yh_off).abs().max().item(), "max_abs_off": yh_off.abs().max().item()}
                del yh_on, yh_off
            out["batches"][str(b)] = {"half_precision": half, "legs": legs, "off_ms": round(off, 4), "on_ms": round(on, 4), "off_over_on": round(off / on, 3),
                                      "on_vs_off_max_abs": (y_on - y_off).abs().max().item(), "max_abs_off": y_off.abs().max().item()}
            del x, y_on, y_off
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
