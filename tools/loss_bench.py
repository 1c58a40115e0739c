#!/usr/bin/env python3
"""FocalLoss and DiceLoss, forward + backward on one sweep's worth of logits: the modules' own torch composition on the
device against the kernels of csrc/loss_pointwise.hip.

    python tools/loss_bench.py [--n 174633] [--classes 22] [--iters 50] [--warmup 10] [--out profiles/loss_bench.json]

Logits float32 [n, C] = normal x 2.5, labels uniform over the classes with 10 % ignored (255); both resident on the
device.  One timed unit = module(x, y) * 0.4 -> backward() -> x.grad, between two CUDA events on the current stream.
  (a) composition: the branch the modules take for inputs the kernels do not (forced here for float32 device tensors);
  (b) kernels: seg3d_focal_loss_fwd / _bwd, seg3d_dice_loss_fwd / _bwd.
(a) and (b) alternate within each iteration, after a warm-up of both; medians and minima in microseconds.  The two routes'
values and gradients are compared on the same inputs.  Needs a GPU: without one the tool fails instead of timing
something else.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd import losses  # noqa: E402


def unit(fn, x, y):
    x.grad = None
    loss = fn(x, y)
    (loss * 0.4).backward()
    return loss.detach(), x.grad


def composed(fn):
    """The module's torch composition on whatever it is given."""
    def call(x, y):
        on_device, losses._on_device_path = losses._on_device_path, lambda *a: False
        try:
            return fn(x, y)
        finally:
            losses._on_device_path = on_device
    return call


def timed_us(fn, x, y):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    unit(fn, x, y)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=174633)
    ap.add_argument("--classes", type=int, default=22)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(args.n, args.classes, generator=g) * 2.5).to(dev).requires_grad_(True)
    y = torch.randint(0, args.classes, (args.n,), generator=g)
    y[torch.rand(args.n, generator=g) < 0.1] = 255
    y = y.to(dev)
    rec = {"tool": "loss_bench", "status": "measured", "device_name": torch.cuda.get_device_name(0), "n": args.n,
           "classes": args.classes, "iters": args.iters, "warmup": args.warmup, "unit": "forward + backward, microseconds"}
    for name, fn in (("focal", losses.FocalLoss()), ("dice", losses.DiceLoss())):
        routes = {"composition": composed(fn), "kernels": fn}
        ref_loss, ref_grad = unit(routes["composition"], x, y)
        ref_loss, ref_grad = float(ref_loss), ref_grad.clone()
        got_loss, got_grad = unit(routes["kernels"], x, y)
        rec[name + "_value_rel_diff"] = abs(float(got_loss) - ref_loss) / abs(ref_loss)
        rec[name + "_grad_max_diff_over_max"] = float((got_grad - ref_grad).abs().max() / ref_grad.abs().max())
        times = {k: [] for k in routes}
        for it in range(args.warmup + args.iters):
            for k, route in routes.items():
                t = timed_us(route, x, y)
                if it >= args.warmup:
                    times[k].append(t)
        for k, v in times.items():
            rec[f"{name}_{k}_us"], rec[f"{name}_{k}_min_us"] = statistics.median(v), min(v)
        rec[name + "_speedup"] = rec[name + "_composition_us"] / rec[name + "_kernels_us"]
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
