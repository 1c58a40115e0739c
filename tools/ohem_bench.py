#!/usr/bin/env python3
"""Class-weighted cross-entropy and OHEM by keep_ratio on one sweep's worth of logits: the torch composition the modules
used before csrc/loss_select.hip (F.cross_entropy(reduction='none'), a boolean-mask gather, torch.topk or a second
softmax) against the kernels, forward alone and forward + backward, for the four modes of seg3d_ce_select_fwd.

    python tools/ohem_bench.py [--n 174633] [--classes 22] [--iters 50] [--warmup 10] [--out profiles/ohem_bench.json]

Logits float32 [n, C] = normal x 2.5, labels uniform over the classes with one fifth ignored (255), class weights in
[1.16, 11.7]; all resident on the device.  One timed unit = loss = f(x, y) (forward), or that followed by
(loss * 0.4).backward() -> x.grad, between two CUDA events on the current stream.
  (a) composition: the torch ops, on float32 device tensors;
  (b) kernels: ops.cross_entropy_select (seg3d_ce_select_fwd / _bwd).
(a) and (b) alternate within each iteration, after a warm-up of both; medians and minima in microseconds.  Host
synchronisations of one forward + backward unit are counted with torch's sync debug mode (the mask gather has one: the
size of its result).  Values and gradients of the two routes are compared on the same inputs.  Needs a GPU: without one
the tool fails instead of timing something else.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd import ops  # noqa: E402

IGNORE = 255
KEEP_RATIO, KEEP_THRESH = 0.3, 0.7


def composition(w, keep_ratio=None, keep_thresh=None, weighted_mean=False):
    def call(x, y):
        if weighted_mean:
            return F.cross_entropy(x, y, weight=w, ignore_index=IGNORE)
        mask = y != IGNORE
        losses = F.cross_entropy(x, y, weight=w, ignore_index=IGNORE, reduction="none")[mask]
        if keep_ratio:
            losses = torch.topk(losses, int(losses.shape[0] * keep_ratio), sorted=False)[0]
        elif keep_thresh:
            probs = F.softmax(x, dim=1)[mask].gather(1, y[mask].unsqueeze(1)).squeeze(1)
            losses = losses[probs < keep_thresh]
        return losses.mean()
    return call


def kernels(w, keep_ratio=None, keep_thresh=None, weighted_mean=False):
    def call(x, y):
        return ops.cross_entropy_select(x, y, ignore_index=IGNORE, class_weight=w, keep_ratio=keep_ratio,
                                        keep_thresh=keep_thresh, weighted_mean=weighted_mean)
    return call


def unit(fn, x, y, backward):
    x.grad = None
    loss = fn(x, y)
    if backward:
        (loss * 0.4).backward()
    return loss.detach(), x.grad


def timed_us(fn, x, y, backward):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    unit(fn, x, y, backward)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3


def host_syncs(fn, x, y):
    """Synchronising calls of one forward + backward, as torch's sync debug mode reports them; None if it cannot."""
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("warn")
    except Exception:  # noqa: BLE001  (a build without the mode)
        return None
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            unit(fn, x, y, True)
        return sum("synchroniz" in str(c.message).lower() for c in caught)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=174633)
    ap.add_argument("--classes", type=int, default=22)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ohem_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ohem_bench: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(args.n, args.classes, generator=g) * 2.5).to(dev).requires_grad_(True)
    y = torch.randint(0, args.classes, (args.n,), generator=g)
    y[torch.rand(args.n, generator=g) < 0.2] = IGNORE
    y = y.to(dev)
    w = (1.16 + (11.7 - 1.16) * torch.rand(args.classes, generator=g)).to(dev)
    rec = {"tool": "ohem_bench", "status": "measured", "device_name": torch.cuda.get_device_name(0), "n": args.n,
           "classes": args.classes, "ignored_share": 0.2, "iters": args.iters, "warmup": args.warmup,
           "keep_ratio": KEEP_RATIO, "keep_thresh": KEEP_THRESH, "unit": "microseconds, median (and minimum) per call"}
    modes = {"mean_weighted": dict(weighted_mean=True), "mean_all": {}, "thresh": dict(keep_thresh=KEEP_THRESH),
             "ratio": dict(keep_ratio=KEEP_RATIO)}
    for name, kwargs in modes.items():
        routes = {"composition": composition(w, **kwargs), "kernels": kernels(w, **kwargs)}
        ref_loss, ref_grad = unit(routes["composition"], x, y, True)
        ref_loss, ref_grad = float(ref_loss), ref_grad.clone()
        got_loss, got_grad = unit(routes["kernels"], x, y, True)
        rec[name + "_value_rel_diff"] = abs(float(got_loss) - ref_loss) / abs(ref_loss)
        rec[name + "_grad_max_diff_over_max"] = float((got_grad - ref_grad).abs().max() / ref_grad.abs().max())
        for k, route in routes.items():
            rec[f"{name}_{k}_host_syncs"] = host_syncs(route, x, y)
        for backward, tag in ((False, "fwd"), (True, "fwdbwd")):
            times = {k: [] for k in routes}
            for it in range(args.warmup + args.iters):
                for k, route in routes.items():
                    t = timed_us(route, x, y, backward)
                    if it >= args.warmup:
                        times[k].append(t)
            for k, v in times.items():
                rec[f"{name}_{tag}_{k}_us"], rec[f"{name}_{tag}_{k}_min_us"] = statistics.median(v), min(v)
            rec[f"{name}_{tag}_speedup"] = rec[f"{name}_{tag}_composition_us"] / rec[f"{name}_{tag}_kernels_us"]
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
