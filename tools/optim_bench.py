#!/usr/bin/env python3
"""The optimizer step over the headline Segformer's parameters: torch's foreach and fused optimizers against
openseg3d_amd.optim (one launch of seg3d_optim_step), for SGD with momentum and for AdamW.

    python tools/optim_bench.py [--iters 60] [--warmup 10] [--out profiles/optim_bench.json]

The parameter list of segformer.build_segmentor(default config) on the device, one fixed random gradient per parameter;
every contender steps the SAME parameter and gradient tensors, each with its own state.  The contenders take turns inside
each iteration, after a warm-up of all of them.  Per step and contender:
  device_us  between two events on the current stream around step(), enqueued behind a device-side sleep of 4 ms
             (torch.cuda._sleep, its tick count sized by timing a probe sleep first; host_ahead says whether every
             host_us of the contender stayed below it) so that every launch of the step is already queued when the
             first one may start: the step's device time with the host out of the picture;
  stream_us  the same two events without the sleep, on an idle device: what the stream sees when the host is not ahead
             (never less than the host time up to the step's last launch);
  host_us    wall time of the step() call itself, nothing awaited inside it; the device is drained between steps.
Medians and minima over --iters steps of each kind (host_us over both kinds).  Those steps find every gradient where the
step before left it, the steady state; seg3d_rebuild_every_step is openseg3d_amd.optim again with every gradient at a new
address each step (two gradient sets taking turns), so that step() fills, pins and uploads its record table every time:
stream_us and host_us of that path.  floor_us is the step's bytes (20 B per
element for SGD with momentum, 28 B for AdamW) at the measured copy rate of 6.29 TB/s; frac_of_floor = floor_us /
device_us.  Needs a GPU: without one the tool fails instead of timing something else.  Prints one JSON line and writes it
to --out."""
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
SGD_KW = dict(lr=1e-4, momentum=0.9, weight_decay=1e-4)
ADAMW_KW = dict(lr=1e-5, weight_decay=1e-2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    args = ap.parse_args()
    if args.iters < 50 or args.warmup < 10:
        raise SystemExit("at least 10 warm-up and 50 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = config.default_cfg()
    model = segformer.build_segmentor(cfg, config.DatasetSpec(cfg)).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 0.01
    n_elems = sum(p.numel() for p in params)
    contenders = {
        "sgd": {"torch_foreach": torch.optim.SGD(params, foreach=True, **SGD_KW),
                "torch_fused": torch.optim.SGD(params, fused=True, **SGD_KW),
                "seg3d": optim.SGD(params, **SGD_KW)},
        "adamw": {"torch_foreach": torch.optim.AdamW(params, foreach=True, **ADAMW_KW),
                  "torch_fused": torch.optim.AdamW(params, fused=True, **ADAMW_KW),
                  "seg3d": optim.AdamW(params, **ADAMW_KW)},
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
    flat = [(a, n, o) for a, d in contenders.items() for n, o in d.items()]
    times = {(a, n): ([], [], []) for a, n, _ in flat}
    for it in range(args.warmup + args.iters):
        for a, n, o in flat:
            for fed in (True, False):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if fed:
                    torch.cuda._sleep(sleep_ticks)
                e0.record()
                t0 = time.perf_counter()
                o.step()
                t1 = time.perf_counter()
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[(a, n)][0 if fed else 1].append(e0.elapsed_time(e1) * 1e3)
                    times[(a, n)][2].append((t1 - t0) * 1e6)
    # the rebuild path: every gradient at another address than in the step before, as after zero_grad(set_to_none=True)
    # whenever the allocator hands out other blocks -- the record table is filled, pinned and uploaded inside step()
    sets = ([p.grad for p in params], [p.grad.clone() for p in params])
    rebuild = {a: ([], []) for a in contenders}
    for it in range(args.warmup + args.iters):
        for a in contenders:
            o = contenders[a]["seg3d"]
            for p, g in zip(params, sets[(it + 1) % 2]):
                p.grad = g
            torch.cuda.synchronize()
            table = o._plans[dev].table
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            o.step()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            assert o._plans[dev].table is not table
            if it >= args.warmup:
                rebuild[a][0].append(e0.elapsed_time(e1) * 1e3)
                rebuild[a][1].append((t1 - t0) * 1e6)
    ok = all(bool(torch.isfinite(p).all()) for p in params)
    result = {"tool": "optim_bench", "device": torch.cuda.get_device_name(0), "parameters": len(params), "elements": n_elems,
              "iters": args.iters, "warmup": args.warmup, "copy_rate_TBps": COPY_TBPS, "sleep_ms": SLEEP_MS,
              "sleep_ticks": sleep_ticks, "finite": ok}
    for a, bytes_per in (("sgd", 20), ("adamw", 28)):
        floor_us = n_elems * bytes_per / (COPY_TBPS * 1e12) * 1e6
        rows = {}
        for n in contenders[a]:
            d, st, h = times[(a, n)]
            rows[n] = {"device_us_median": round(statistics.median(d), 1), "device_us_min": round(min(d), 1),
                       "stream_us_median": round(statistics.median(st), 1),
                       "host_us_median": round(statistics.median(h), 1), "host_us_min": round(min(h), 1),
                       "frac_of_floor": round(floor_us / statistics.median(d), 3), "host_ahead": max(h) < SLEEP_MS * 1e3}
        st, h = rebuild[a]
        rows["seg3d_rebuild_every_step"] = {"stream_us_median": round(statistics.median(st), 1),
                                            "host_us_median": round(statistics.median(h), 1), "host_us_min": round(min(h), 1)}
        result[a] = {"bytes_per_element": bytes_per, "floor_us": round(floor_us, 1), **rows}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
