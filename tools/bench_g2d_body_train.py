"""Informational: forward + backward of G2d's ResBlock2D body, [B,512,64,64] -> [B,64,512,512] with a sum loss (8 x ResBlock2D(512) + three
bilinear x2 + ResBlock2D stages), at B = 1 and B = 4, in eval mode (frozen statistics, fine-tuning) and in train mode (batch statistics) —
native_body(trainable=True) (ag.Conv2dFn: forward, backward-data and backward-weight on the matrix cores, csrc/conv2d_bwd_f16x3.hip)
against torch's own modules on the same box and commit, in the same run: torch fp32 with cudnn.benchmark off and on (the baseline: what
the fused blocks did under autograd before the keyword, and still do without it), then the native leg.  Eval mode comes first, because
the train legs step the running statistics of the two copies a different number of times.  There is no torch autocast-fp16 leg: half
and one-product training are not built, so no native leg would stand beside it.  Every leg is printed to stderr as it finishes.
The gradient differences in the output (relative L2, native against torch fp32 on the GPU) are for information.  On maps of this size
a ReLU whose argument is within rounding of zero flips between any two implementations, torch on the GPU against torch on the CPU
included, so the figures say that the legs compute the same thing, not how accurately; the tests do that.
Also one backward-weight launch of the dominant conv, 512 -> 512 at 64x64 (19.3 GFLOP per frame, three f16 products per multiply), with
its TFLOP/s, against ATen's weight gradient.  HIP events over `steps` calls after `warmup`.  Prints one JSON line; --out also writes it.
usage: python tools/bench_g2d_body_train.py [--warmup 3] [--steps 10] [--out profiles/g2d_body_train_timing.json]"""
import argparse, copy, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
from megaportrait_hack_amd import encoders2d as E, model as M, ops
from bench_g2d_body import Body, commit, step_ms


def train_step(body, x):
    def fn():
        x.grad = None
        body.zero_grad(set_to_none=True)
        body(x).sum().backward()
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(20241020)
    g2d = E.G2d()
    with torch.no_grad():
        for m in g2d.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.normal_(0.0, 0.5)
    body = Body(g2d).to(dev)
    native = copy.deepcopy(body)
    assert M.native_g2d_body(native, True, trainable=True)
    rows = {}
    for mode in ("eval", "train"):
        body.train(mode == "train")
        native.train(mode == "train")
        for b in a.batches:
            x = torch.randn(b, 512, a.hw, a.hw, device=dev, requires_grad=True)
            legs = {}

            def leg(name, module):
                legs[name] = step_ms(train_step(module, x), a.warmup, a.steps)
                print(f"{mode} B={b} {name}: {legs[name]:.3f} ms", file=sys.stderr, flush=True)

            for bench in (False, True):
                torch.backends.cudnn.benchmark = bench
                leg(f"torch_fp32_benchmark_{'on' if bench else 'off'}", body)
            train_step(body, x)()
            want_dx, want_dw = x.grad.clone(), body.res_blocks[0].conv1.weight.grad.clone()
            leg("native_trainable", native)
            dx, dw = x.grad, native.res_blocks[0].conv1.weight.grad
            best = min(legs["torch_fp32_benchmark_off"], legs["torch_fp32_benchmark_on"])
            rows[f"{mode}_B{b}"] = {"ms": {k: round(v, 3) for k, v in legs.items()},
                                    "best_torch_fp32_over_native": round(best / legs["native_trainable"], 3),
                                    "native_vs_torch_fp32_rel_l2": {"dx": ((dx - want_dx).norm() / want_dx.norm()).item(),
                                                                    "d_res_blocks0_conv1_weight": ((dw - want_dw).norm() / want_dw.norm()).item()}}
            del x, dx, dw, want_dx, want_dw
            native.zero_grad(set_to_none=True)
            body.zero_grad(set_to_none=True)
    # one backward-weight launch of the dominant conv: 512 -> 512 at 64x64, the input's descriptor and the gradient's scale at hand
    launches = {}
    torch.backends.cudnn.benchmark = True
    with torch.no_grad():
        for b in a.batches:
            x, dy = torch.randn(b, 512, a.hw, a.hw, device=dev), torch.randn(b, 512, a.hw, a.hw, device=dev)
            w = torch.randn(512, 512, 3, 3, device=dev)
            rng = ops.absmax_range(x)
            _, scale = ops.grad_prep(dy, want_bias=False)
            ms = step_ms(lambda: ops.conv2d_bwd_weight(x, dy, scale, rng), a.warmup + 5, a.steps * 5)
            prep_ms = step_ms(lambda: ops.grad_prep(dy), a.warmup + 5, a.steps * 5)
            torch_ms = step_ms(lambda: torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                                            [False, True, False]), a.warmup + 5, a.steps * 5)
            flop = 2.0 * 9 * 512 * 512 * a.hw * a.hw * b
            launches[f"B{b}"] = {"native_ms": round(ms, 4), "native_tflops": round(flop / ms * 1e-9, 1), "grad_prep_ms": round(prep_ms, 4),
                                 "torch_fp32_ms": round(torch_ms, 4), "torch_fp32_tflops": round(flop / torch_ms * 1e-9, 1),
                                 "plan_kernel_splits_tps_tiles": list(_plan(b, a.hw))}
    out = {"what": "G2d body forward + backward (sum loss): 8 x ResBlock2D(512) @64x64, bilinear x2 + ResBlock2D 512->256, 256->128, 128->64",
           "commit": commit(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "H": a.hw, "W": a.hw, "warmup": a.warmup,
           "steps": a.steps, "timer": "HIP events around `steps` back-to-back forward + backward calls after `warmup` calls, ms per call",
           "baseline": "the parent commit's behaviour is the torch_fp32 leg of the same run",
           "body_fwd_bwd": rows, "bwd_weight_512_512_64x64": launches, "gflop_per_frame": round(2.0 * 9 * 512 * 512 * a.hw * a.hw * 1e-9, 2)}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def _plan(b, hw):
    import ctypes
    from megaportrait_hack_amd import _lib

    out = (ctypes.c_int * 4)()
    _lib.load().mphip_debug_conv2d_bwd_weight_plan(b, 512, 512, hw, hw, out)
    return tuple(out)


if __name__ == "__main__":
    main()
