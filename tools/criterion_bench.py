#!/usr/bin/env python3
"""The training criterion on the headline sizes, per-term entries against the fused entry.

    python tools/criterion_bench.py [--sizes 174633,108690,19483] [--classes 22] [--iters 20] [--warmup 5]
                                    [--out profiles/criterion_bench.json]

Three heads of float32 logits [n_h, C] = normal x 2.5, labels uniform over the classes with 10 % ignored (255), head
weights 1, 1, 0.4, MODEL.LOSSES = {ohem_ce: 1.0 (keep_thresh 0.7), lovasz: 1.0}; everything resident on the device.
  unfused  the loop of losses.compute_loss over ops.cross_entropy and ops.lovasz_softmax (seg3d_cross_entropy_*,
           seg3d_lovasz_softmax_*), the weighted sum and the gradient sums left to torch
  fused    ops.fused_criterion (seg3d_criterion_fwd / _bwd)
timed forward only and forward + backward between two HIP events on the current stream; the two routes alternate within
each iteration after a warm-up of both; medians and minima in microseconds.  The routes' losses and gradients are compared
for equality on the same inputs.  Needs a GPU: without one the tool fails instead of timing something else.  Prints one
JSON line and writes its keys to --out, keeping every other key the file already holds: further measurements of the same
change (bench.py pairs, the trace's criterion interval) are recorded there under "train_step"."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd import ops  # noqa: E402

HEAD_WEIGHTS = (1.0, 1.0, 0.4)
KEEP, IGN = 0.7, 255


def unfused(xs, ys):
    loss = 0
    for x, y, hw in zip(xs, ys, HEAD_WEIGHTS):
        for t in (ops.cross_entropy(x, y, ignore_index=IGN, keep_thresh=KEEP), 1.0 * ops.lovasz_softmax(x, y, IGN)):
            loss = loss + (t * 1.0 if hw == 1.0 else hw * t * 1.0)
    return loss


def fused(xs, ys):
    return ops.fused_criterion(xs, ys, HEAD_WEIGHTS[:len(xs)], ignore_index=IGN, keep_thresh=KEEP, ce_weight=1.0,
                               lovasz_weight=1.0)


def unit(fn, xs, ys, backward):
    for x in xs:
        x.grad = None
    loss = fn(xs, ys)
    if backward:
        loss.backward()
    return loss.detach()


def timed_us(fn, xs, ys, backward):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    unit(fn, xs, ys, backward)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="174633,108690,19483")
    ap.add_argument("--classes", type=int, default=22)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "criterion_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("criterion_bench: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    sizes = [int(v) for v in args.sizes.split(",")]
    g = torch.Generator().manual_seed(0)
    xs, ys = [], []
    for n in sizes:
        xs.append((torch.randn(n, args.classes, generator=g) * 2.5).to(dev).requires_grad_(True))
        y = torch.randint(0, args.classes, (n,), generator=g)
        y[torch.rand(n, generator=g) < 0.1] = IGN
        ys.append(y.to(dev))
    rec = {"tool": "criterion_bench", "status": "measured", "device_name": torch.cuda.get_device_name(0), "sizes": sizes,
           "classes": args.classes, "iters": args.iters, "warmup": args.warmup, "unit": "microseconds, HIP events"}
    routes = {"unfused": unfused, "fused": fused}
    ref = float(unit(unfused, xs, ys, True))
    ref_grads = [x.grad.clone() for x in xs]
    got = float(unit(fused, xs, ys, True))
    rec["loss_equal"] = got == ref
    rec["grads_equal"] = all(torch.equal(x.grad, r) for x, r in zip(xs, ref_grads))
    for tag, backward in (("fwd", False), ("fwd_bwd", True)):
        times = {k: [] for k in routes}
        for it in range(args.warmup + args.iters):
            for k, route in routes.items():
                t = timed_us(route, xs, ys, backward)
                if it >= args.warmup:
                    times[k].append(t)
        for k, v in times.items():
            rec[f"{k}_{tag}_us"], rec[f"{k}_{tag}_min_us"] = statistics.median(v), min(v)
        rec[f"{tag}_speedup"] = rec[f"unfused_{tag}_us"] / rec[f"fused_{tag}_us"]
    print(json.dumps(rec))
    kept = {}
    if os.path.exists(args.out):  # records other tools merged into the file (the "train_step" series) stay
        try:
            with open(args.out) as f:
                kept = {k: v for k, v in json.load(f).items() if k not in rec}
        except (ValueError, AttributeError):
            kept = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps({**rec, **kept}, indent=1) + "\n")


if __name__ == "__main__":
    main()
