"""Informational: Emtn.forward, image [B,3,512,512] -> (rotation, translation, expression) — the frozen 6DRepNet and the two CIFAR-stem
ResNet-18s `head_pose_net` and `expression_net` — with `native_resnets()` on — their sixteen BasicBlocks as model.BasicBlockFused, the 3x3
convs on csrc/conv2d_f16x3.hip and csrc/conv2d_s2_f16x3.hip — against the same call with the switch off (torch fp32, cudnn.benchmark on) on
the same box and commit, in the same process.  Each leg: `warmup` calls, then `runs` calls timed one by one with HIP events; the median is
reported.  The legs run off, on, on, off so that neither side always goes first.  B = 1 and B = 8.  One more leg for context: the unswapped
module under torch.autocast(float16).  And one 64 -> 128 stride-2 launch at 256 x 256 (layer2's first conv at 512^2 input) with its
TFLOP/s, counting 2 * 9 * Ci * Co * Ho * Wo.  Prints one JSON line; --out also writes it to a file.
--stem measures the fused stem instead (model.StemFused, csrc/conv2d_stem.hip), same timer and rules: (a) one net's stem alone — the one
fused launch on the folded weights against the four torch fp32 modules conv1, bn1, relu, maxpool, legs torch, fused, fused, torch, and for
context the four modules under torch.autocast(float16) — in ms and in GB/s counted as 4 * (3 * H * W + Co * Ho * Wo) bytes per frame;
(b) Emtn.forward with everything off, with the BasicBlocks fused, and with the blocks and the stems fused, legs off, resnets, stem, stem,
resnets, off.
--rotation measures the 6DRepNet switch instead (model.RepVGGBlockFused, model.native_rotation_net; csrc/conv2d_grp_f16x3.hip for its
thirteen groups = 2 blocks), same timer and rules: (a) `rotation_net.predict` alone, legs off, on, on, off, and for context the unswapped
net under torch.autocast(float16); (b) Emtn.forward with everything off, with the ResNets and stems fused, and with the ResNets, the
stems and the rotation net fused, legs off, resnets+stem, all, all, resnets+stem, off, and the all-off call under autocast(float16).
--split measures the split-K form of the stride-1 convs instead (csrc/conv2d_splitk_f16x3.hip; the `split_small_maps` switches), same timer
and rules: (a) per conv: every stride-1 3x3 conv shape of the three nets at this frame size, one launch as the fused blocks issue it (ReLU,
a descriptor of x given, the output's descriptor wanted), legs S = 1, then every S of 2, 4, 8, 16 that divides the (Ci / groups) / 16
chunks, then S = 1 again: the spread between the two S = 1 legs is the noise a gain has to beat; (b) Emtn.forward and rotation_net.predict
with everything off (torch fp32), with today's switches (ResNets, stems, rotation net), with those plus split_small_maps, and for context
the all-off call under torch.autocast(float16): legs off, on, split, autocast, autocast, split, on, off.
usage: python tools/bench_emtn.py [--b 1 8] [--warmup 5] [--runs 20] [--out profiles/emtn_timing.json]
       python tools/bench_emtn.py --stem [--b 1 8] [--out profiles/emtn_stem_timing.json]
       python tools/bench_emtn.py --rotation [--b 1 8] [--out profiles/rotation_net_timing.json]
       python tools/bench_emtn.py --split [--b 1 8] [--out profiles/conv2d_splitk_timing.json]"""
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


def stem_timing(a, dev, emtn):
    """--stem: (a) one stem alone, (b) Emtn.forward off / resnets on / resnets and stems on."""
    net = emtn.head_pose_net
    co = net.conv1.out_channels
    ho = wo = (a.hw + 1) // 2
    out = {"what": "the 3->64 stem of Emtn's ResNet-18s (conv1, bn1, relu, maxpool) as one launch of csrc/conv2d_stem.hip",
           "commit": commit(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "H": a.hw, "W": a.hw, "warmup": a.warmup,
           "runs": a.runs, "timer": "HIP events around each call after `warmup` calls; median (and minimum) of `runs` calls, ms per call",
           "bytes_per_frame": 4 * (3 * a.hw * a.hw + co * ho * wo), "stem_order": ["torch", "fused", "fused", "torch"],
           "forward_order": ["off", "resnets", "resnets+stem", "resnets+stem", "resnets", "off"], "batches": {}}
    with torch.no_grad():
        w, bias = M.fold_batchnorm(net.conv1, net.bn1)
        torch_stem = lambda x: net.maxpool(net.relu(net.bn1(net.conv1(x))))
        for b in a.b:
            x = torch.rand(b, 3, a.hw, a.hw, device=dev) * 2 - 1
            gbs = lambda ms: round(out["bytes_per_frame"] * b / ms * 1e-6, 1)
            legs = []
            for fused in (False, True, True, False):
                fn = (lambda: ops.conv2d_stem(x, w, bias, want_range=True)) if fused else (lambda: torch_stem(x))
                med, best = median_ms(fn, a.warmup, a.runs)
                legs.append({"fused": fused, "median_ms": round(med, 4), "min_ms": round(best, 4)})
            with torch.autocast(device_type="cuda", dtype=torch.float16):
                amp, amp_best = median_ms(lambda: torch_stem(x), a.warmup, a.runs)
            t_ms = statistics.mean(l["median_ms"] for l in legs if not l["fused"])
            f_ms = statistics.mean(l["median_ms"] for l in legs if l["fused"])
            err = (ops.conv2d_stem(x, w, bias) - torch_stem(x)).abs().max().item()
            stem = {"legs": legs, "torch_fp32_ms": round(t_ms, 4), "fused_ms": round(f_ms, 4), "torch_over_fused": round(t_ms / f_ms, 2),
                    "torch_fp32_gbs": gbs(t_ms), "fused_gbs": gbs(f_ms), "torch_autocast_fp16_ms": round(amp, 4),
                    "torch_autocast_fp16_min_ms": round(amp_best, 4), "fused_vs_torch_max_abs": err}
            flegs = []
            for mode in (0, 1, 2, 2, 1, 0):
                emtn.native_resnets(mode > 0, fuse_stem=mode == 2)
                med, best = median_ms(lambda: emtn(x), a.warmup, a.runs)
                flegs.append({"mode": ("off", "resnets", "resnets+stem")[mode], "median_ms": round(med, 4), "min_ms": round(best, 4)})
            emtn.native_resnets(True, fuse_stem=True)
            _, t_on, e_on = emtn(x)
            emtn.native_resnets(False)
            _, t_off, e_off = emtn(x)
            mean = lambda m: round(statistics.mean(l["median_ms"] for l in flegs if l["mode"] == m), 4)
            out["batches"][str(b)] = {"stem": stem, "forward": {"legs": flegs, "off_ms": mean("off"), "resnets_ms": mean("resnets"),
                                                                 "resnets_stem_ms": mean("resnets+stem"),
                                                                 "expression_stem_vs_off_max_abs": (e_on - e_off).abs().max().item(),
                                                                 "expression_max_abs_off": e_off.abs().max().item(),
                                                                 "translation_stem_vs_off_max_abs": (t_on - t_off).abs().max().item(),
                                                                 "translation_max_abs_off": t_off.abs().max().item()}}
            del x
    return out


def rotation_timing(a, dev, emtn):
    """--rotation: (a) rotation_net.predict alone, (b) Emtn.forward off / ResNets and stems on / those and the rotation net on."""
    det = emtn.rotation_net
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():   # He initialisation: activations stay O(1) through the 28 ReLU layers, as a trained net's do
        for m in det.model.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu", generator=gen)
                m.bias.normal_(0.0, 0.1, generator=gen)
    det.model.to(dev)
    out = {"what": "the frozen 6DRepNet (RepVGG-B1g2, deploy form) of Emtn: 27 of its 28 blocks as one matrix-core launch each",
           "commit": commit(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "H": a.hw, "W": a.hw, "warmup": a.warmup,
           "runs": a.runs, "timer": "HIP events around each call after `warmup` calls; median (and minimum) of `runs` calls, ms per call",
           "predict_order": ["off", "on", "on", "off"], "forward_order": ["off", "resnets+stem", "all", "all", "resnets+stem", "off"],
           "batches": {}}
    mean = lambda legs, key, val: round(statistics.mean(l["median_ms"] for l in legs if l[key] == val), 4)
    with torch.no_grad():
        for b in a.b:
            x = torch.rand(b, 3, a.hw, a.hw, device=dev) * 2 - 1
            legs = []
            for on in (False, True, True, False):
                M.native_rotation_net(emtn, on)
                med, best = median_ms(lambda: det.predict(x), a.warmup, a.runs)
                legs.append({"native_rotation_net": on, "median_ms": round(med, 4), "min_ms": round(best, 4)})
            with torch.autocast(device_type="cuda", dtype=torch.float16):
                amp, amp_best = median_ms(lambda: det.predict(x), a.warmup, a.runs)
            M.native_rotation_net(emtn, True)
            deg_on, _ = det.predict(x)
            M.native_rotation_net(emtn, False)
            deg_off, _ = det.predict(x)
            off, on = mean(legs, "native_rotation_net", False), mean(legs, "native_rotation_net", True)
            predict = {"legs": legs, "off_ms": off, "on_ms": on, "off_over_on": round(off / on, 3), "torch_autocast_fp16_ms": round(amp, 4),
                       "torch_autocast_fp16_min_ms": round(amp_best, 4), "degrees_on_vs_off_max_abs": (deg_on - deg_off).abs().max().item()}
            flegs = []
            for mode in (0, 1, 2, 2, 1, 0):
                emtn.native_resnets(mode > 0, fuse_stem=mode > 0)
                emtn.native_rotation_net(mode == 2)
                med, best = median_ms(lambda: emtn(x), a.warmup, a.runs)
                flegs.append({"mode": ("off", "resnets+stem", "all")[mode], "median_ms": round(med, 4), "min_ms": round(best, 4)})
            with torch.autocast(device_type="cuda", dtype=torch.float16):
                famp, famp_best = median_ms(lambda: emtn(x), a.warmup, a.runs)
            out["batches"][str(b)] = {"predict": predict,
                                      "forward": {"legs": flegs, "off_ms": mean(flegs, "mode", "off"),
                                                  "resnets_stem_ms": mean(flegs, "mode", "resnets+stem"), "all_ms": mean(flegs, "mode", "all"),
                                                  "torch_autocast_fp16_ms": round(famp, 4), "torch_autocast_fp16_min_ms": round(famp_best, 4)}}
            del x
    return out


def split_timing(a, dev, emtn):
    """--split: (a) the per-conv sweep over S, (b) Emtn.forward and rotation_net.predict off / on / on + split_small_maps / autocast."""
    det = emtn.rotation_net
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():   # (rotation_timing's He initialisation)
        for m in det.model.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu", generator=gen)
                m.bias.normal_(0.0, 0.1, generator=gen)
    det.model.to(dev)
    hw = a.hw
    # (Ci, Co, H = W, groups, where): layer1 .. layer4 of the ResNet-18s (after the stem's max-pool), stages 1 .. 3 of RepVGG-B1g2
    shapes = [(64, 64, hw // 2, 1, "resnet18.layer1"), (128, 128, hw // 4, 1, "resnet18.layer2, repvgg.layer1"),
              (128, 128, hw // 4, 2, "repvgg.layer1 (groups 2)"), (256, 256, hw // 8, 1, "resnet18.layer3, repvgg.layer2"),
              (256, 256, hw // 8, 2, "repvgg.layer2 (groups 2)"), (512, 512, hw // 16, 1, "resnet18.layer4, repvgg.layer3"),
              (512, 512, hw // 16, 2, "repvgg.layer3 (groups 2)")]
    out = {"what": "split-K form of the stride-1 2-D 3x3 f16x3 convs (csrc/conv2d_splitk_f16x3.hip) and the split_small_maps switches",
           "commit": commit(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "H": hw, "W": hw, "warmup": a.warmup,
           "runs": a.runs, "timer": "HIP events around each call after `warmup` calls; median (and minimum) of `runs` calls, ms per call",
           "cudnn_benchmark": True, "sweep_order": "S = 1, the S > 1 legs in ascending order, S = 1 again",
           "net_order": ["off", "on", "split", "autocast", "autocast", "split", "on", "off"],
           "net_modes": {"off": "torch fp32, every switch off", "on": "native_resnets(fuse_stem) + native_rotation_net (predict: the latter)",
                         "split": "the same with split_small_maps=True", "autocast": "every switch off under torch.autocast(float16)"},
           "sweep": [], "batches": {}}
    with torch.no_grad():
        for b in a.b:
            for ci, co, h, g, where in shapes:
                x = torch.randn(b, ci, h, h, device=dev)
                pack = ops.PackedConv2d(torch.randn(co, ci // g, 3, 3, device=dev) * 0.05, torch.zeros(co, device=dev), g)
                rng = ops.absmax_range(x)
                conv = ops.conv2d if g == 1 else ops.conv2d_grouped
                cands = [s for s in (2, 4, 8, 16) if ops.conv2d_split_supported(b, ci, co, h, h, g, s)]
                legs = []
                for s in [1] + cands + [1]:
                    med, best = median_ms(lambda: conv(x, pack, relu=True, x_range=rng, want_range=True, splits=s), a.warmup, a.runs)
                    legs.append({"S": s, "median_ms": round(med, 4), "min_ms": round(best, 4)})
                ones = [l["median_ms"] for l in legs if l["S"] == 1]
                s1, spread = statistics.mean(ones), abs(ones[0] - ones[1])
                best_leg = min((l for l in legs if l["S"] > 1), key=lambda l: l["median_ms"], default=None)
                row = {"N": b, "Ci": ci, "Co": co, "H": h, "W": h, "groups": g, "where": where, "legs": legs, "s1_ms": round(s1, 4),
                       "s1_spread_ms": round(spread, 4), "recommended_S": ops.conv2d_splits(b, ci, co, h, h, g)}
                if best_leg is not None:
                    gain = s1 - best_leg["median_ms"]
                    row.update({"best_S": best_leg["S"], "best_ms": best_leg["median_ms"], "gain_ms": round(gain, 4),
                                "gain_beats_spread": bool(gain > spread and best_leg["median_ms"] < min(ones))})
                out["sweep"].append(row)
                del x, pack
        mean = lambda legs, mode: round(statistics.mean(l["median_ms"] for l in legs if l["mode"] == mode), 4)
        for b in a.b:
            x = torch.rand(b, 3, hw, hw, device=dev) * 2 - 1
            res = {}
            for name in ("emtn_forward", "rotation_net_predict"):
                fn = (lambda: emtn(x)) if name == "emtn_forward" else (lambda: det.predict(x))
                legs = []
                for mode in ("off", "on", "split", "autocast", "autocast", "split", "on", "off"):
                    on, split = mode in ("on", "split"), mode == "split"
                    if name == "emtn_forward":
                        emtn.native_resnets(on, fuse_stem=on, split_small_maps=split)
                    emtn.native_rotation_net(on, split_small_maps=split)
                    if mode == "autocast":
                        with torch.autocast(device_type="cuda", dtype=torch.float16):
                            med, best = median_ms(fn, a.warmup, a.runs)
                    else:
                        med, best = median_ms(fn, a.warmup, a.runs)
                    legs.append({"mode": mode, "median_ms": round(med, 4), "min_ms": round(best, 4)})
                emtn.native_resnets(False)
                emtn.native_rotation_net(False)
                res[name] = {"legs": legs, "off_ms": mean(legs, "off"), "on_ms": mean(legs, "on"), "split_ms": mean(legs, "split"),
                             "torch_autocast_fp16_ms": mean(legs, "autocast")}
            out["batches"][str(b)] = res
            del x
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--stem", action="store_true", help="measure the fused stem (model.StemFused) instead; see the module docstring")
    ap.add_argument("--rotation", action="store_true", help="measure the 6DRepNet switch (model.native_rotation_net) instead; see the module docstring")
    ap.add_argument("--split", action="store_true", help="measure the split-K convs and the split_small_maps switches instead; see the module docstring")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs: the median of at least 20 runs is reported")
    dev = torch.device("cuda:0")
    torch.manual_seed(20241018)
    torch.backends.cudnn.benchmark = True
    emtn = E.Emtn().to(dev).eval()
    if a.stem or a.rotation or a.split:
        out = split_timing(a, dev, emtn) if a.split else rotation_timing(a, dev, emtn) if a.rotation else stem_timing(a, dev, emtn)
        print(json.dumps(out))
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        return
    out = {"what": "Emtn.forward: 6DRepNet rotation_net, head_pose_net and expression_net (CIFAR-stem ResNet-18s), fc",
           "commit": commit(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "H": a.hw, "W": a.hw, "warmup": a.warmup,
           "runs": a.runs, "timer": "HIP events around each call after `warmup` calls; median (and minimum) of `runs` calls, ms per call",
           "order": ["off", "on", "on", "off"], "batches": {}}
    with torch.no_grad():
        # one launch of layer2's first conv: 64 -> 128 at stride 2 from a 256 x 256 map (B = 1), and the stride-1 conv that follows it
        h = a.hw // 2
        xc = torch.randn(1, 64, h, h, device=dev)
        pk = ops.PackedConv2d(torch.randn(128, 64, 3, 3, device=dev) * 0.05, torch.zeros(128, device=dev))
        rng = ops.absmax_range(xc)
        flop = 2.0 * 9 * 64 * 128 * (h // 2) ** 2
        s2, _ = median_ms(lambda: ops.conv2d_s2(xc, pk, x_range=rng), a.warmup, a.runs)
        out["conv_s2_64_128"] = {"H": h, "W": h, "Ho": h // 2, "Wo": h // 2, "ms": round(s2, 4), "tflops": round(flop / s2 * 1e-9, 1)}
        x1 = torch.randn(1, 128, h // 2, h // 2, device=dev)
        pk1 = ops.PackedConv2d(torch.randn(128, 128, 3, 3, device=dev) * 0.05, torch.zeros(128, device=dev))
        rng1 = ops.absmax_range(x1)
        s1, _ = median_ms(lambda: ops.conv2d(x1, pk1, x_range=rng1), a.warmup, a.runs)
        out["conv_s1_128_128"] = {"H": h // 2, "W": h // 2, "ms": round(s1, 4), "tflops": round(2.0 * 9 * 128 * 128 * (h // 2) ** 2 / s1 * 1e-9, 1)}
        del xc, pk, x1, pk1
        for b in a.b:
            x = torch.rand(b, 3, a.hw, a.hw, device=dev) * 2 - 1
            legs = []
            for on in (False, True, True, False):
                M.native_emtn_resnets(emtn, on)
                med, best = median_ms(lambda: emtn(x), a.warmup, a.runs)
                legs.append({"native_resnets": on, "median_ms": round(med, 4), "min_ms": round(best, 4)})
            emtn.native_resnets(True)
            _, t_on, e_on = emtn(x)
            emtn.native_resnets(False)
            _, t_off, e_off = emtn(x)
            with torch.autocast(device_type="cuda", dtype=torch.float16):
                amp, amp_best = median_ms(lambda: emtn(x), a.warmup, a.runs)
            off = statistics.mean(l["median_ms"] for l in legs if not l["native_resnets"])
            on = statistics.mean(l["median_ms"] for l in legs if l["native_resnets"])
            out["batches"][str(b)] = {"legs": legs, "off_ms": round(off, 4), "on_ms": round(on, 4), "off_over_on": round(off / on, 3),
                                      "torch_autocast_fp16_ms": round(amp, 4), "torch_autocast_fp16_min_ms": round(amp_best, 4),
                                      "expression_on_vs_off_max_abs": (e_on - e_off).abs().max().item(), "expression_max_abs_off": e_off.abs().max().item(),
                                      "translation_on_vs_off_max_abs": (t_on - t_off).abs().max().item(), "translation_max_abs_off": t_off.abs().max().item()}
            del x
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
