"""Informational: G2d's ResBlock2D body, [B,512,64,64] -> [B,64,512,512] (8 x ResBlock2D(512) + three bilinear x2 + ResBlock2D stages) —
model.ResBlock2DFused (BatchNorm folded, 3x3 convs of csrc/conv2d_f16x3.hip) against torch's own modules on the same box and commit, in the
same run: torch fp32 with cudnn.benchmark off and on, NCHW and channels_last, torch under autocast-fp16 (for information: a different
arithmetic), the native body, and one 512->512 conv launch at 64x64 (19.3 GFLOP per frame) with its TFLOP/s — in three and in one product.
Half-precision legs (half_precision=True): torch under autocast-fp16 against the native body under autocast-fp16, and a .half() body,
native against torch.  fuse_upsample legs ("fuse_upsample" in the output): at B = 1 and B = --b, the whole body and each of the three
Sequential(Upsample, ResBlock2D) stages on its own input, as torch fp32, native_body() and native_body(fuse_upsample=True)
(model.Up2ResBlock2DFused: the up-sample folded into the convs of csrc/conv2d_up2_f16x3.hip), the three legs back to back.  HIP events over `steps` calls after `warmup`.  Prints one JSON line; --out also writes it to a file.
usage: python tools/bench_g2d_body.py [--b 8] [--warmup 20] [--steps 50] [--out profiles/g2d_body_timing.json]"""
import argparse, copy, json, os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
from megaportrait_hack_amd import encoders2d as E, model as M, ops


def step_ms(fn, warmup, steps):
    for _ in range(warmup):
        fn()
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


class Body(nn.Module):
    """G2d between its head and its final_conv."""

    def __init__(self, g2d):
        super().__init__()
        self.res_blocks, self.upsample1, self.upsample2, self.upsample3 = g2d.res_blocks, g2d.upsample1, g2d.upsample2, g2d.upsample3

    def forward(self, x):
        return self.upsample3(self.upsample2(self.upsample1(self.res_blocks(x))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--hw", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(20241018)
    g2d = E.G2d()
    with torch.no_grad():
        for m in g2d.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.normal_(0.0, 0.5)
    body = Body(g2d).to(dev).eval()
    body_cl = copy.deepcopy(body).to(memory_format=torch.channels_last)
    native = copy.deepcopy(body)
    assert M.native_g2d_body(native, True)
    x = torch.randn(a.b, 512, a.hw, a.hw, device=dev)
    x_cl = x.contiguous(memory_format=torch.channels_last)
    legs = {}
    with torch.no_grad():
        for bench in (False, True):
            torch.backends.cudnn.benchmark = bench
            tag = "benchmark_on" if bench else "benchmark_off"
            legs[f"torch_fp32_nchw_{tag}"] = step_ms(lambda: body(x), a.warmup, a.steps)
            legs[f"torch_fp32_channels_last_{tag}"] = step_ms(lambda: body_cl(x_cl), a.warmup, a.steps)
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            legs["torch_autocast_fp16_nchw_benchmark_on"] = step_ms(lambda: body(x), a.warmup, a.steps)
            legs["torch_autocast_fp16_channels_last_benchmark_on"] = step_ms(lambda: body_cl(x_cl), a.warmup, a.steps)
        legs["native_fp32"] = step_ms(lambda: native(x), a.warmup, a.steps)
        err = (native(x) - body(x)).abs().max().item()
        # the half-precision form: the same process, torch's leg first, then the native one, for each of the two modes
        native_hp = copy.deepcopy(body)
        assert M.native_g2d_body(native_hp, True, half_precision=True)
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            legs["torch_autocast_fp16_nchw_again"] = step_ms(lambda: body(x), a.warmup, a.steps)
            legs["native_half_precision_autocast_fp16"] = step_ms(lambda: native_hp(x), a.warmup, a.steps)
            err_autocast = (native_hp(x).float() - body(x).float()).abs().max().item()
        body_h, xh = copy.deepcopy(body).half(), x.half()
        native_h = copy.deepcopy(body_h)
        assert M.native_g2d_body(native_h, True, half_precision=True)
        legs["torch_half_module_nchw"] = step_ms(lambda: body_h(xh), a.warmup, a.steps)
        legs["native_half_precision_half_module"] = step_ms(lambda: native_h(xh), a.warmup, a.steps)
        err_half = (native_h(xh).float() - body_h(xh).float()).abs().max().item()
        # the up-samples folded into the convs: whole body and the three stages, torch / native / native + fuse_upsample, per batch size
        fused = copy.deepcopy(body)
        assert M.native_g2d_body(fused, True, fuse_upsample=True) and all(isinstance(s, M.Up2ResBlock2DFused) for s in (fused.upsample1, fused.upsample2, fused.upsample3))
        torch.backends.cudnn.benchmark = True
        up2 = {}
        for b in sorted({1, a.b}):
            xb = x[:b].contiguous()
            rows = {"body": {"torch_fp32_nchw": step_ms(lambda: body(xb), a.warmup, a.steps),
                             "native": step_ms(lambda: native(xb), a.warmup, a.steps),
                             "native_fuse_upsample": step_ms(lambda: fused(xb), a.warmup, a.steps),
                             "fused_vs_native_max_abs": (fused(xb) - native(xb)).abs().max().item()}}
            xs = native.res_blocks(xb)
            for name in ("upsample1", "upsample2", "upsample3"):
                t, n, f = getattr(body, name), getattr(native, name), getattr(fused, name)
                xin = xs.clone()      # (no descriptor on it: both native legs scan their input, as after a torch producer)
                rows[name] = {"input": list(xin.shape), "torch_fp32_nchw": step_ms(lambda: t(xin), a.warmup, a.steps),
                              "native": step_ms(lambda: n(xin), a.warmup, a.steps),
                              "native_fuse_upsample": step_ms(lambda: f(xin), a.warmup, a.steps)}
                xs = n(xin)
            for r in rows.values():
                r["native_over_native_fuse_upsample"] = round(r["native"] / r["native_fuse_upsample"], 3)
            up2[f"B{b}"] = {k: {kk: (round(vv, 4) if isinstance(vv, float) and kk != "fused_vs_native_max_abs" else vv) for kk, vv in r.items()}
                            for k, r in rows.items()}
            del xs, xin
        # one launch of the dominant conv: 512 -> 512 at 64x64, bias + ReLU epilogue, the input's descriptor at hand
        blk = native.res_blocks[0]
        p1 = blk._folded()[0]
        rng = ops.absmax_range(x)
        conv_ms = step_ms(lambda: ops.conv2d(x, p1, relu=True, x_range=rng, want_range=True), a.warmup, a.steps)
        conv1_ms = step_ms(lambda: ops.conv2d(x, p1, relu=True, x_range=rng, want_range=True, products=1), a.warmup, a.steps)
        conv_torch_ms = step_ms(lambda: torch.relu_(nn.functional.conv2d(x, p1.weight, p1.bias, padding=1)), a.warmup, a.steps)
    flop = 2.0 * 9 * 512 * 512 * a.hw * a.hw * a.b
    best_torch = min(v for k, v in legs.items() if k.startswith("torch_fp32"))
    out = {"what": "G2d body: 8 x ResBlock2D(512) @64x64, bilinear x2 + ResBlock2D 512->256, 256->128, 128->64", "commit": commit(),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": a.b, "H": a.hw, "W": a.hw, "warmup": a.warmup,
           "steps": a.steps, "timer": "HIP events around `steps` back-to-back calls after `warmup` calls, ms per call",
           "body_ms": {k: round(v, 4) for k, v in legs.items()},
           "best_torch_fp32_over_native": round(best_torch / legs["native_fp32"], 3),
           "native_vs_torch_fp32_max_abs": err,
           "torch_autocast_fp16_over_native_half_precision": round(legs["torch_autocast_fp16_nchw_again"] / legs["native_half_precision_autocast_fp16"], 3),
           "torch_half_module_over_native_half_precision": round(legs["torch_half_module_nchw"] / legs["native_half_precision_half_module"], 3),
           "native_half_precision_vs_torch_max_abs": {"autocast_fp16": err_autocast, "half_module": err_half},
           "fuse_upsample": up2,
           "conv_512_512_64x64": {"native_ms": round(conv_ms, 4), "native_tflops": round(flop / conv_ms * 1e-9, 1),
                                  "native_one_product_ms": round(conv1_ms, 4), "native_one_product_tflops": round(flop / conv1_ms * 1e-9, 1),
                                  "torch_fp32_ms": round(conv_torch_ms, 4), "torch_fp32_tflops": round(flop / conv_torch_ms * 1e-9, 1),
                                  "gflop_per_frame": round(flop / a.b * 1e-9, 2)}}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
