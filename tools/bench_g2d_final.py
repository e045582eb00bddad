"""Informational: G2d's final GroupNorm-ReLU-conv-sigmoid on [B,64,512,512] — the fused HIP kernels (model.G2dFinalConv) against torch's
own nn.Sequential on the same box, in the same run, interleaved rounds, HIP events, median of the rounds.  Forward at B=8 in fp32 NCHW,
fp16 NCHW and fp16 channels_last (cudnn.benchmark on; the native path copies a channels_last map to NCHW first, and that copy is inside
its time); forward + backward (fp32, all five gradients) at B=4.  Prints one JSON line; --out also writes it to a file.
usage: python tools/bench_g2d_final.py [--b 8] [--b-train 4] [--steps 10] [--rounds 5] [--out profiles/g2d_final_timing.json]"""
import argparse, copy, json, os, statistics, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
from megaportrait_hack_amd import model as M


def step_ms(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        r = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        return r.stdout.strip() or os.environ.get("MPHIP_COMMIT", "unknown")
    except OSError:
        return os.environ.get("MPHIP_COMMIT", "unknown")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--b-train", type=int, default=4)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = True
    torch.manual_seed(20240917)
    seq32 = nn.Sequential(nn.GroupNorm(32, 64), nn.ReLU(inplace=True), nn.Conv2d(64, 3, 3, padding=1), nn.Sigmoid()).to(dev).eval()
    with torch.no_grad():
        seq32[0].weight.uniform_(0.5, 1.5)
        seq32[0].bias.normal_(0.0, 0.5)
    seq16 = copy.deepcopy(seq32).half()
    seq16cl = copy.deepcopy(seq16).to(memory_format=torch.channels_last)
    nat32, nat16 = M.G2dFinalConv.from_sequential(copy.deepcopy(seq32)), M.G2dFinalConv.from_sequential(copy.deepcopy(seq16))
    x32 = torch.randn(a.b, 64, a.hw, a.hw, device=dev)
    x16 = x32.half()
    x16cl = x16.contiguous(memory_format=torch.channels_last)
    legs = {
        "fwd_fp32_nchw": (lambda: seq32(x32), lambda: nat32(x32)),
        "fwd_fp16_nchw": (lambda: seq16(x16), lambda: nat16(x16)),
        "fwd_fp16_channels_last": (lambda: seq16cl(x16cl), lambda: nat16(x16cl)),
    }
    res = {k: ([], []) for k in legs}
    with torch.no_grad():
        for t, n in legs.values():
            for _ in range(3):
                t(), n()
        for _ in range(a.rounds):
            for k, (t, n) in legs.items():
                res[k][0].append(step_ms(t, a.steps))
                res[k][1].append(step_ms(n, a.steps))
    del x16, x16cl, x32
    torch.cuda.empty_cache()

    # training: forward + backward, all five gradients, fp32
    seq_t, nat_t = copy.deepcopy(seq32).train(), M.G2dFinalConv.from_sequential(copy.deepcopy(seq32)).train()
    xt = torch.randn(a.b_train, 64, a.hw, a.hw, device=dev, requires_grad=True)
    dy = torch.randn(a.b_train, 3, a.hw, a.hw, device=dev)

    def train(m):
        def fn():
            xt.grad = None
            for p in m.parameters():
                p.grad = None
            m(xt).backward(dy)
        return fn

    tt, tn = train(seq_t), train(nat_t)
    res["fwd_bwd_fp32_nchw"] = ([], [])
    for _ in range(3):
        tt(), tn()
    for _ in range(a.rounds):
        res["fwd_bwd_fp32_nchw"][0].append(step_ms(tt, a.steps))
        res["fwd_bwd_fp32_nchw"][1].append(step_ms(tn, a.steps))

    out = {"what": "G2d final_conv: GroupNorm(32,64)-ReLU-Conv2d(64,3,3,p=1)-Sigmoid", "commit": commit(), "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "B_forward": a.b, "B_train": a.b_train, "H": a.hw, "W": a.hw, "steps": a.steps, "rounds": a.rounds,
           "timer": "HIP events around `steps` back-to-back calls, median of `rounds` interleaved rounds, ms per call", "legs": {}}
    for k, (t, n) in res.items():
        mt, mn = statistics.median(t), statistics.median(n)
        out["legs"][k] = {"torch_ms": round(mt, 4), "native_ms": round(mn, 4), "torch_over_native": round(mt / mn, 3),
                          "torch_ms_min_max": [round(min(t), 4), round(max(t), 4)], "native_ms_min_max": [round(min(n), 4), round(max(n), 4)]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
