#!/usr/bin/env python3
"""Furthest-point sampling on one Waymo-sized scene: ops.furthestsampling and ops.sectorized_fps (csrc/sampling.hip), and
the kernel against a torch composition of the same loop.

    python tools/fps_bench.py [--n 175000] [--sectors 16] [--compare-m 512] [--iters 5] [--warmup 2]
                              [--out profiles/fps_bench.json]

The scene is a ring-shaped cloud of n rows (radius 3 .. 60 m, thin in z), resident on the device.  Configurations:
  flat        furthestsampling, one segment of n rows, m = n / 4 picks: the streaming tier (four float planes in L2);
  resident    furthestsampling, one segment of 16 384 rows (the largest the resident tier takes), m = 4 096;
  sectorized  sectorized_fps, the same scene, m = n / 4 over `sectors` sectors: every sector in the resident tier, one
              workgroup each, including the angle, assignment and grouping launches and the wrapper's two host syncs;
  compare     the kernel and a torch composition of the loop (subtract, square, sum, minimum, argmax, index: no host sync
              inside the loop) at --compare-m picks on the full scene and on the 16 384-row cloud, alternating.
One timed unit = one call, host clock around the call and a device synchronise (the wrappers read counts back, so a
call is not a pure enqueue).  Medians and minima over --iters after --warmup; microseconds per pick = call time / picks.
Needs a GPU: without one the tool fails instead of timing something else.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd import ops  # noqa: E402


def scene(n, seed):
    rng = np.random.default_rng(seed)
    a, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(3.0, 60.0, n)
    return np.stack([r * np.sin(a), r * np.cos(a), rng.normal(0.0, 1.0, n)], axis=1).astype(np.float32)


def composition(xyz, m):
    """The loop as a user of torch would write it on the device; picks int64 [m]."""
    tmp = torch.full((xyz.shape[0],), 1e10, dtype=torch.float32, device=xyz.device)
    idx = torch.zeros((m,), dtype=torch.int64, device=xyz.device)
    last = idx[0]
    for j in range(1, m):
        tmp = torch.minimum(tmp, ((xyz - xyz[last]) ** 2).sum(1))
        last = tmp.argmax()
        idx[j] = last
    return idx


def timed_ms(fn, warmup, iters):
    out = []
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def alternating_ms(fns, warmup, iters):
    out = {k: [] for k in fns}
    for it in range(warmup + iters):
        for k, fn in fns.items():
            t = timed_ms(fn, 0, 1)[0]
            if it >= warmup:
                out[k].append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=175000)
    ap.add_argument("--sectors", type=int, default=16)
    ap.add_argument("--compare-m", type=int, default=512)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fps_bench: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    n, m = args.n, args.n // 4
    xyz = torch.from_numpy(scene(n, 0)).to(dev)
    small = torch.from_numpy(scene(16384, 1)).to(dev)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    rec = {"tool": "fps_bench", "status": "measured", "device_name": torch.cuda.get_device_name(0), "n": n, "m": m,
           "sectors": args.sectors, "iters": args.iters, "warmup": args.warmup, "unit": "one call, milliseconds"}
    try:
        rec["sclk_mhz_at_start"] = torch.cuda.clock_rate()
    except Exception:  # the query needs the SMI bindings
        rec["sclk_mhz_at_start"] = None

    def put(name, times, picks):
        rec[name + "_ms"], rec[name + "_min_ms"] = statistics.median(times), min(times)
        rec[name + "_us_per_pick"] = rec[name + "_ms"] * 1e3 / picks

    off, noff = i32(n), i32(m)
    put("flat", timed_ms(lambda: ops.furthestsampling(xyz, off, noff), args.warmup, args.iters), m)
    s_off, s_noff = i32(16384), i32(4096)
    put("resident", timed_ms(lambda: ops.furthestsampling(small, s_off, s_noff), args.warmup, args.iters), 4096)
    put("sectorized", timed_ms(lambda: ops.sectorized_fps(xyz, off, noff, args.sectors), args.warmup, args.iters), m)
    rec["sectorized_us_per_pick_per_sector"] = rec["sectorized_ms"] * 1e3 / (m / args.sectors)
    rec["flat_over_sectorized"] = rec["flat_ms"] / rec["sectorized_ms"]

    cm = args.compare_m
    rec["compare_m"] = cm
    for tag, cloud, c_off in (("scene", xyz, off), ("resident", small, s_off)):
        c_noff = i32(cm)
        got = ops.furthestsampling(cloud, c_off, c_noff).long()
        rec[f"compare_{tag}_picks_equal"] = float((got == composition(cloud, cm)).float().mean())
        t = alternating_ms({"kernel": lambda: ops.furthestsampling(cloud, c_off, c_noff),
                            "composition": lambda: composition(cloud, cm)}, args.warmup, args.iters)
        for k, v in t.items():
            put(f"compare_{tag}_{k}", v, cm)
        rec[f"compare_{tag}_speedup"] = rec[f"compare_{tag}_composition_ms"] / rec[f"compare_{tag}_kernel_ms"]
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
