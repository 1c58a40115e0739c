#!/usr/bin/env python3
"""Forward + backward of the per-point MLPs alone (Segformer.point_encoder and .fusion_encoder) at the headline row count,
with ops.POINT_BN_ONLOAD off and on in the same process.

    python tools/point_mlp_bench.py [--rows 174633] [--iters 20] [--warmup 5] [--out profiles/point_mlp_bench.json]

point_encoder  = BN(6) L(6->64) BN ReLU L(64->128) BN ReLU L(128->256) BN ReLU L(256->64, bias)
fusion_encoder = L(96->256) BN ReLU L(256->128) BN ReLU L(128->64) BN ReLU
in training mode on random rows, timed between two HIP events on the current stream (the weight-gradient stream joins
before the stop event: every gradient is finished); the two settings alternate within each iteration after a warm-up of
both; medians and minima in microseconds.  Outputs and gradients of the two settings are compared for equality.  The byte
counts are the BatchNorm / activation passes' row traffic from the layer widths (4 bytes x rows x columns per pass:
affine_act reads y and writes z, the backward's reduce and apply passes read dz, y (and z when off) and write dy); the
peak-memory figure is torch's max_memory_allocated over one forward + backward.  "kernels_us" times, per Linear behind a
BatchNorm + ReLU, the affine pass, the six-product Linear and the weight-gradient partials on activated rows against the
two kernels that activate on load, each alone on the device.  Needs a GPU.  Prints one JSON line and
writes its keys to --out, keeping every other key the file already holds."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd import ops, segformer  # noqa: E402

MLPS = {
    "point_encoder": dict(dims=[6, 64, 128, 256, 64], first_bn=6, last_plain=True, input_grad=False),
    "fusion_encoder": dict(dims=[96, 256, 128, 64], first_bn=None, last_plain=False, input_grad=True),
}


def bn_pass_bytes(spec, rows, onload):
    """Row traffic of the BatchNorm + ReLU passes behind the hidden Linears: forward affine_act (2 C), backward reduce
    (3 C) and apply (4 C) as composed; on load the fused pairs drop the affine pass and both backward passes lose the z
    read, the unfused last pair (no Linear behind it) loses the z read only."""
    dims, total = spec["dims"], 0
    n = len(dims) - 1
    for i in range(n):
        if spec["last_plain"] and i == n - 1:
            continue
        c = dims[i + 1]
        fused = onload and i + 1 < n and dims[i + 1] % 32 == 0 and dims[i + 2] % 64 == 0
        fwd = 0 if fused else 2 * c
        bwd = (2 * c + 3 * c) if onload else (3 * c + 4 * c)
        total += (fwd + bwd) * rows * 4
    return total


def unit(mlp, x, dy):
    x.grad = None
    for p in mlp.parameters():
        p.grad = None
    y = mlp(x)
    y.backward(dy)
    return y.detach()


def timed_us(mlp, x, dy):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    unit(mlp, x, dy)
    torch.cuda.current_stream().wait_stream(ops.side_stream(x.device))
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3


PAIRS = [(64, 128), (128, 256), (256, 64), (256, 128), (128, 64)]  # (cin, cout) of the Linears behind a BatchNorm + ReLU


def kernel_pairs(rows, iters, warmup, dev, g):
    """Per shape, alone on the device: the affine pass, the six-product Linear and the dense weight-gradient partials
    on the activated rows against the two kernels that activate on load (medians, us)."""
    from openseg3d_amd import _lib
    from openseg3d_amd.ops import _ptr, _stream, _workspace
    import ctypes

    def med(fn):
        ts = []
        for i in range(warmup + iters):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if i >= warmup:
                ts.append(start.elapsed_time(stop) * 1e3)
        return round(statistics.median(ts), 1)

    out = {}
    for cin, cout in PAIRS:
        x = torch.randn(rows, cin, generator=g).to(dev)
        dy = torch.randn(rows, cout, generator=g).to(dev)
        scale = (torch.rand(cin, generator=g) + 0.5).to(dev)
        shift = (torch.randn(cin, generator=g) * 0.3).to(dev)
        w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(dev)
        z, y = torch.empty_like(x), torch.empty_like(dy)
        packed = ops._linear_pack_x6(w)
        ws_bytes = _lib.query("seg3d_linear_wgrad_workspace_bytes", rows, cin, cout)
        ws = _workspace(ws_bytes, dev)
        chunks = ctypes.c_int32(0)
        rec = {
            "affine_act": med(lambda: _lib.call("seg3d_affine_act", _ptr(x), None, _ptr(scale), _ptr(shift), 1, rows, cin,
                                                _ptr(z), _stream())),
            "linear_x6": med(lambda: _lib.call("seg3d_linear_fwd_x6", _ptr(z), rows, _ptr(packed), None, None, None, 0, cin,
                                               cout, _ptr(y), _stream())),
            "linear_x6_bnrelu": med(lambda: _lib.call("seg3d_linear_fwd_x6_bnrelu", _ptr(x), _ptr(scale), _ptr(shift), rows,
                                                      _ptr(packed), None, cin, cout, _ptr(y), _stream())),
            "wgrad": med(lambda: _lib.call("seg3d_linear_wgrad_partials", _ptr(z), _ptr(dy), rows, cin, cout, 0, _ptr(ws),
                                           ws_bytes, ctypes.byref(chunks), _stream())),
            "wgrad_bnrelu": med(lambda: _lib.call("seg3d_linear_wgrad_partials_bnrelu", _ptr(x), _ptr(scale), _ptr(shift),
                                                  _ptr(dy), rows, cin, cout, 0, _ptr(ws), ws_bytes, ctypes.byref(chunks),
                                                  _stream())),
        }
        out[f"{cin}->{cout}"] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=174633)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_mlp_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("point_mlp_bench: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    result = {"rows": args.rows, "iters": args.iters}
    for name, spec in MLPS.items():
        torch.manual_seed(1)
        mlp = segformer._bn_mlp(spec["dims"], first_bn=spec["first_bn"], last_plain=spec["last_plain"]).to(dev).train()
        x = torch.randn(args.rows, spec["dims"][0], generator=g).to(dev).requires_grad_(spec["input_grad"])
        dy = torch.randn(args.rows, spec["dims"][-1], generator=g).to(dev)
        outs, peaks, times = {}, {}, {False: [], True: []}
        for onload in (False, True):
            ops.POINT_BN_ONLOAD = onload
            for _ in range(args.warmup):
                unit(mlp, x, dy)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            y = unit(mlp, x, dy)
            torch.cuda.synchronize()
            peaks[onload] = torch.cuda.max_memory_allocated() - base
            outs[onload] = [y] + [p.grad.clone() for p in mlp.parameters()] + ([x.grad.clone()] if spec["input_grad"] else [])
        for _ in range(args.iters):
            for onload in (False, True):
                ops.POINT_BN_ONLOAD = onload
                times[onload].append(timed_us(mlp, x, dy))
        ops.POINT_BN_ONLOAD = True
        rec = {"equal": all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))}
        for onload, key in ((False, "off"), (True, "on")):
            rec[key] = {"median_us": round(statistics.median(times[onload]), 1), "min_us": round(min(times[onload]), 1),
                        "bn_pass_bytes": bn_pass_bytes(spec, args.rows, onload), "peak_extra_bytes": int(peaks[onload])}
        rec["peak_memory_diff_bytes"] = int(peaks[True] - peaks[False])
        result[name] = rec
    result["kernels_us"] = kernel_pairs(args.rows, args.iters, args.warmup, dev, g)
    line = json.dumps(result)
    print(line)
    kept = {}
    if os.path.exists(args.out):  # further measurements of the same change ("train_step": bench.py pairs) stay
        with open(args.out) as f:
            kept = json.load(f)
    kept.update(result)
    with open(args.out, "w") as f:
        f.write(json.dumps(kept, indent=1) + "\n")
    if not all(result[n]["equal"] for n in MLPS):
        raise SystemExit("point_mlp_bench: the two settings differ")


if __name__ == "__main__":
    main()
