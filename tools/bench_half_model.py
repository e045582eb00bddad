"""Informational: B=8 step time of a .half() / .bfloat16() GbaseHotSlice (typed boundaries, single-product convs) against the fp32
module under torch.autocast(float16) fed the same fp16 inputs — same box, same seeds, interleaved rounds.  Prints one JSON line.
usage: python tools/bench_half_model.py [--b 8] [--steps 30] [--rounds 3]"""
import argparse, copy, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(20240501)
    hot32 = M.GbaseHotSlice().to(dev).eval()
    hot16, hotbf = copy.deepcopy(hot32).half(), copy.deepcopy(hot32).bfloat16()
    g = torch.Generator(device="cpu").manual_seed(7)
    B = a.b
    inp = dict(vs=torch.randn(B, 96, 16, 64, 64, generator=g), es=torch.randn(B, 512, generator=g), zs=torch.randn(B, 512, generator=g),
               zd=torch.randn(B, 512, generator=g), Rs=torch.rand(B, 3, generator=g) * 60 - 30, Rd=torch.rand(B, 3, generator=g) * 60 - 30,
               ts=torch.randn(B, 3, generator=g) * 0.1, td=torch.randn(B, 3, generator=g) * 0.1)
    in16 = {k: v.to(dev, torch.float16) for k, v in inp.items()}
    inbf = {k: v.to(dev, torch.bfloat16) for k, v in inp.items()}

    def autocast32():
        with torch.autocast("cuda", dtype=torch.float16):
            hot32(**in16)

    legs = {"fp32_module_autocast_fp16": autocast32, "half_module_fp16": lambda: hot16(**in16), "half_module_bf16": lambda: hotbf(**inbf)}
    res = {k: [] for k in legs}
    with torch.no_grad():
        for fn in legs.values():
            for _ in range(3):
                fn()
        for _ in range(a.rounds):
            for k, fn in legs.items():
                res[k].append(step_ms(fn, a.steps))
    out = {"B": B, "steps": a.steps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    out.update({f"{k}_ms": round(statistics.median(v), 4) for k, v in res.items()})
    out["half_fp16_vs_autocast"] = round(out["half_module_fp16_ms"] / out["fp32_module_autocast_fp16_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
