#!/usr/bin/env python3
"""Gradient-norm clipping over the headline Segformer's parameters: torch.nn.utils.clip_grad_norm_ (foreach and
single-tensor) against openseg3d_amd.optim.GradClipper (seg3d_grad_norm + seg3d_grad_scale).

    python tools/clip_bench.py [--iters 60] [--warmup 10] [--out profiles/clip_bench.json]

The parameter list of segformer.build_segmentor(default config) on the device, one fixed random gradient per parameter,
restored from a copy before every call (outside the timed window) so that every call sees the same norm.  Two cases:
`clip`, max_norm = half the norm, the coefficient is 0.5 and every gradient is rewritten; `noclip`, max_norm = twice the
norm, the coefficient is 1 (torch multiplies by it all the same, seg3d_grad_scale returns at once).  `seg3d_norm_only` is
optim.grad_norm's pass (no scale launch).  The contenders take turns inside each iteration, after a warm-up of all of them.
Per call and contender:
  device_us  between two events on the current stream around the call, enqueued behind a device-side sleep of 4 ms
             (torch.cuda._sleep, its tick count sized by timing a probe sleep first; host_ahead says whether every
             host_us of the contender stayed below it), so that every launch of the call is already queued when the
             first one may start: the call's device time with the host out of the picture;
  host_us    wall time of the call itself, nothing awaited inside it.
Medians and minima over --iters calls.  floor_us is the case's bytes (4 B per element read by the norm, 8 B per element
read and written by the scale) at the measured copy rate of 6.29 TB/s; frac_of_floor = floor_us / device_us.  Needs a GPU:
without one the tool fails instead of timing something else.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd import config, optim, segformer  # noqa: E402

COPY_TBPS = 6.29
SLEEP_MS = 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.json"))
    args = ap.parse_args()
    if args.iters < 50 or args.warmup < 10:
        raise SystemExit("at least 10 warm-up and 50 timed calls")
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = config.default_cfg()
    model = segformer.build_segmentor(cfg, config.DatasetSpec(cfg)).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 0.01
    grads = [p.grad for p in params]
    saved = [g.clone() for g in grads]
    n_elems = sum(p.numel() for p in params)
    norm = float(optim.grad_norm(params))
    norm_torch = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g.double()) for g in grads])))
    clip, noclip = norm * 0.5, norm * 2.0
    torch_clip = torch.nn.utils.clip_grad_norm_
    clippers = {"clip": optim.GradClipper(params, clip), "noclip": optim.GradClipper(params, noclip),
                "norm_only": optim.GradClipper(params, noclip)}
    contenders = {
        "clip": {"torch_foreach": lambda: torch_clip(params, clip, foreach=True),
                 "torch_single": lambda: torch_clip(params, clip, foreach=False),
                 "seg3d": clippers["clip"]},
        "noclip": {"torch_foreach": lambda: torch_clip(params, noclip, foreach=True),
                   "seg3d": clippers["noclip"],
                   "seg3d_norm_only": clippers["norm_only"].norm},
    }
    # the device-side sleep that lets the host get ahead, sized by measurement: SLEEP_MS on this card's counter
    probe = []
    for _ in range(6):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(1_000_000)
        e1.record()
        torch.cuda.synchronize()
        probe.append(e0.elapsed_time(e1))
    sleep_ticks = int(SLEEP_MS / statistics.median(probe[1:]) * 1_000_000)
    flat = [(c, n, f) for c, d in contenders.items() for n, f in d.items()]
    times = {(c, n): ([], []) for c, n, _ in flat}
    coefs = {}
    for it in range(args.warmup + args.iters):
        for c, n, f in flat:
            torch._foreach_copy_(grads, saved)  # the same gradients, at the same addresses, for every call
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(sleep_ticks)
            e0.record()
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[(c, n)][0].append(e0.elapsed_time(e1) * 1e3)
                times[(c, n)][1].append((t1 - t0) * 1e6)
            if n == "seg3d":
                coefs[c] = float(clippers[c].last_coef)
    result = {"tool": "clip_bench", "device": torch.cuda.get_device_name(0), "parameters": len(params), "elements": n_elems,
              "iters": args.iters, "warmup": args.warmup, "copy_rate_TBps": COPY_TBPS, "sleep_ms": SLEEP_MS,
              "sleep_ticks": sleep_ticks, "norm": norm, "norm_torch_fp64": norm_torch, "coef": coefs}
    for c, bytes_per in (("clip", 12), ("noclip", 4)):
        floor_us = n_elems * bytes_per / (COPY_TBPS * 1e12) * 1e6
        rows = {}
        for n in contenders[c]:
            d, h = times[(c, n)]
            rows[n] = {"device_us_median": round(statistics.median(d), 1), "device_us_min": round(min(d), 1),
                       "host_us_median": round(statistics.median(h), 1), "host_us_min": round(min(h), 1),
                       "frac_of_floor": round(floor_us / statistics.median(d), 3), "host_ahead": max(h) < SLEEP_MS * 1e3}
        result[c] = {"bytes_per_element": bytes_per, "floor_us": round(floor_us, 1), **rows}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
