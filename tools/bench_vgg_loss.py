"""Informational: forward + backward of the VGG19 perceptual loss (losses.VGG19FeatureLoss, default widths 64..512, seeded random weights)
on [B,3,512,512] images, the gradient taken to the predicted image, at B = 1 and B = 4: the native path (one VGG19FeatureLossFn node: the
convs on the matrix cores, csrc/feature_loss.hip between them) against the same nn.Sequential in PyTorch on the same box, in the same run:
fp32 with cudnn.benchmark off and on (the faster of the two is what a user has without the module) and torch.autocast(float16).  The legs
alternate, `rounds` times, and each leg reports the median of its rounds and their spread.  There is no speed bar: the module is opt-in and
the rows are quoted as measured, slower ones included.  The loss values and the relative L2 of the image gradient between the legs are for
information: ReLU, pool-argmax and sgn decisions flip on single elements between any two implementations, the tests compare exactly.
HIP events over `steps` calls after `warmup`.  Prints one JSON line; --out also writes it.
usage: python tools/bench_vgg_loss.py [--warmup 3] [--steps 10] [--rounds 3] [--out profiles/vgg19_loss_timing.json]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
from megaportrait_hack_amd.losses import VGG19FeatureLoss, VGG19FeatureLossFn
from bench_g2d_body import commit, step_ms


def gflop(loss, h, w):
    """forward of ONE image through the convs up to the deepest tap"""
    total, pools = 0.0, 0
    for i, m in enumerate(loss.vgg19):
        if isinstance(m, nn.MaxPool2d):
            pools += 1
        elif isinstance(m, nn.Conv2d):
            total += 2.0 * 9 * m.in_channels * m.out_channels * (h >> pools) * (w >> pools)
        if i == max(loss.taps):
            break
    return total * 1e-9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(20241021)
    loss = VGG19FeatureLoss()
    with torch.no_grad():
        for m in loss.vgg19:
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
                m.bias.normal_(0.0, 0.1)
    loss = loss.to(dev)
    rows = {}
    for b in a.batches:
        p = torch.rand(b, 3, a.hw, a.hw, device=dev, requires_grad=True)
        t = torch.rand(b, 3, a.hw, a.hw, device=dev)
        values = {}

        def step(native, autocast=False):
            def fn():
                p.grad = None
                loss.native(native)
                with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                    v = loss(p, t)
                v.backward()
                return v
            return fn

        legs = {"native": (step(True), None), "torch_fp32_benchmark_off": (step(False), False), "torch_fp32_benchmark_on": (step(False), True),
                "torch_autocast_fp16": (step(False, True), True)}
        v = legs["native"][0]()
        assert isinstance(v.grad_fn, VGG19FeatureLossFn._backward_cls), "the native path was not taken"
        times = {k: [] for k in legs}
        for r in range(a.rounds):
            for name, (fn, bench) in legs.items():
                if bench is not None:
                    torch.backends.cudnn.benchmark = bench
                times[name].append(step_ms(fn, a.warmup, a.steps))
                values[name] = (fn().item(), p.grad.clone())
                print(f"B={b} round {r} {name}: {times[name][-1]:.3f} ms", file=sys.stderr, flush=True)
        peak = {}
        for name, (fn, bench) in legs.items():   # peak allocated memory of one step, above what is held between steps
            if bench is not None:
                torch.backends.cudnn.benchmark = bench
            p.grad = None
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[name] = round((torch.cuda.max_memory_allocated() - held) / 2 ** 20, 1)
        ms = {k: round(statistics.median(v), 3) for k, v in times.items()}
        best = min(ms["torch_fp32_benchmark_off"], ms["torch_fp32_benchmark_on"])
        ref = values["torch_fp32_benchmark_off"]
        rows[f"B{b}"] = {"ms_median": ms, "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
                         "best_torch_fp32_over_native": round(best / ms["native"], 3),
                         "torch_autocast_fp16_over_native": round(ms["torch_autocast_fp16"] / ms["native"], 3),
                         "native_tflops_executed": round(3 * b * gflop(loss, a.hw, a.hw) / ms["native"], 1),
                         "step_peak_mib": peak,
                         "loss": {k: v[0] for k, v in values.items()},
                         "dpred_rel_l2_vs_torch_fp32": {k: ((v[1] - ref[1]).norm() / ref[1].norm()).item() for k, v in values.items()
                                                        if k != "torch_fp32_benchmark_off"}}
        del p, t, values, v
    out = {"what": "VGG19 feature loss, forward + backward to the predicted image: taps after layers 1, 6, 11, 20, 29, widths 64..512",
           "commit": commit(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "H": a.hw, "W": a.hw, "warmup": a.warmup,
           "steps": a.steps, "rounds": a.rounds,
           "timer": "HIP events around `steps` back-to-back forward + backward calls after `warmup` calls, ms per call; legs alternate per round",
           "baseline": "the parent commit has no such module: its user runs the torch_fp32 leg (or autocast) of the same run",
           "gflop_forward_one_image": round(gflop(loss, a.hw, a.hw), 1),
           "native_tflops_executed": "3 * B * gflop_forward_one_image (two forwards, one backward-data) over the native leg's time",
           "fwd_bwd": rows}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
