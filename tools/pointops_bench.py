#!/usr/bin/env python3
"""query_and_group and interpolation on one Waymo-sized scene: the kernels of csrc/pointops.hip against the torch
composition a user had before them (the same quantities from torch indexing: int64 index gathers, a broadcast
subtraction and a concatenation; K gather, multiply and add passes into a zero-filled result).

    python tools/pointops_bench.py [--n 175000] [--iters 7] [--warmup 3] [--out profiles/pointops_bench.json]

The scene is fps_bench's ring-shaped cloud of n rows.  The neighbour tables come from ops.knn_query once, outside every
timed window.  Rows:
  group           query_and_group, m = n queries (the cloud on itself), K = 16, c = 32, with xyz: out [n, 16, 35];
  interp_c64/256  interpolation's sum (knn_interpolate) of n queries over the cloud's n / 4 sectorized_fps picks, K = 3,
                  c = 64 and c = 256.
Per row: forward, and forward + backward (the gradient of feat, dout given), kernel path and composition alternating in
the same run; one timed unit = one call, host clock around the call and a device synchronise; medians and minima over
--iters after --warmup.  The backward of the kernel path includes building the inverse neighbour lists
(seg3d_group_index).  Each C entry is also timed on its own between two device events (the backward entries with the
lists prebuilt and every gradient asked for), and its algorithmic bytes -- rows read + rows written + index / weight
bytes, entry_bytes() below -- over that time are set against the 6.29 TB/s measured copy rate of the card.
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

from openseg3d_amd import _lib, ops  # noqa: E402
from openseg3d_amd.ops import _ptr, _stream  # noqa: E402

COPY_RATE_TBS = 6.29


def scene(n, seed):
    rng = np.random.default_rng(seed)
    a, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(3.0, 60.0, n)
    return np.stack([r * np.sin(a), r * np.cos(a), rng.normal(0.0, 1.0, n)], axis=1).astype(np.float32)


def group_composition(xyz, new_xyz, feat, idx):
    """What a user composes from torch indexing today: one int64 copy of the table, two row gathers of [m K] rows, a
    broadcast subtraction and a concatenation into [m, K, 3 + c]."""
    m, k = idx.shape
    rows = idx.reshape(m * k).to(torch.int64)
    offsets = torch.index_select(xyz, 0, rows).reshape(m, k, 3) - new_xyz[:, None, :]
    gathered = torch.index_select(feat, 0, rows).reshape(m, k, -1)
    return torch.cat([offsets, gathered], dim=2)


def interp_composition(feat, idx, dist):
    """What a user composes today: inverse-distance weights normalised per query, then K passes of gather, multiply and
    add into a zero-filled [m, c] result, slot 0 first."""
    inv = (dist + 1e-8).reciprocal()
    w = inv / inv.sum(dim=1, keepdim=True)
    acc = torch.zeros((idx.shape[0], feat.shape[1]), dtype=torch.float32, device=feat.device)
    for slot in range(idx.shape[1]):
        acc = acc + torch.index_select(feat, 0, idx[:, slot].to(torch.int64)) * w[:, slot:slot + 1]
    return acc


def entry_bytes(kind, n, m, k, c):
    """Algorithmic bytes of one C entry: rows read + rows written + index / weight bytes."""
    p = m * k
    if kind == "group_fwd":      # gathered xyz and feat rows, the queries, idx; the [m, K, 3 + c] store
        return p * (3 + c) * 4 + m * 12 + p * 4 + p * (3 + c) * 4
    if kind == "group_bwd":      # dout rows through the lists (+ their first 3 columns again and idx for dnew_xyz), order,
        return p * (3 + c) * 4 + p * 12 + p * 4 + p * 4 + (n + 1) * 4 + n * (3 + c) * 4 + m * 12  # offsets; the gradients
    if kind == "interp_fwd":     # K feat rows per query, idx and dist; out and the weights
        return p * c * 4 + p * 8 + m * c * 4 + p * 4
    if kind == "interp_bwd":     # one dout row per list entry, order and weight, offsets; dfeat
        return p * c * 4 + p * 8 + (n + 1) * 4 + n * c * 4
    raise KeyError(kind)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternating_ms(fns, warmup, iters):
    out = {k: [] for k in fns}
    for it in range(warmup + iters):
        for k, fn in fns.items():
            t = wall_ms(fn)
            if it >= warmup:
                out[k].append(t)
    return out


def event_ms(fn, warmup, iters):
    out = []
    for it in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=175000)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointops_bench.json"))
    args = ap.parse_args()
    if args.iters < 5:
        raise SystemExit("pointops_bench: medians of at least 5 calls")
    if not torch.cuda.is_available():
        raise SystemExit("pointops_bench: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    n = args.n
    rng = np.random.default_rng(7)
    xyz = torch.from_numpy(scene(n, 0)).to(dev)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    rec = {"tool": "pointops_bench", "status": "measured", "device_name": torch.cuda.get_device_name(0), "n": n,
           "iters": args.iters, "warmup": args.warmup, "unit": "one call, milliseconds", "copy_rate_tbs": COPY_RATE_TBS,
           "rows": {}}

    def put(row, name, times):
        rec["rows"][row][name + "_ms"], rec["rows"][row][name + "_min_ms"] = statistics.median(times), min(times)

    def entry(row, kind, fn, dims):
        times = event_ms(fn, args.warmup, args.iters)
        put(row, "entry_" + kind, times)
        nbytes = entry_bytes(kind, *dims)
        r = rec["rows"][row]
        r["entry_" + kind + "_bytes"] = nbytes
        r["entry_" + kind + "_tbs"] = nbytes / (statistics.median(times) * 1e-3) / 1e12
        r["entry_" + kind + "_of_copy_rate"] = r["entry_" + kind + "_tbs"] / COPY_RATE_TBS

    def compare(row, kernel_fwd, comp_fwd, feat, dout):
        """forward, and forward + backward (feat's gradient), kernel path and composition alternating."""
        feat.requires_grad_(False)
        t = alternating_ms({"kernel": lambda: kernel_fwd(feat), "composition": lambda: comp_fwd(feat)}, args.warmup, args.iters)
        put(row, "fwd_kernel", t["kernel"])
        put(row, "fwd_composition", t["composition"])
        feat.requires_grad_(True)

        def both(f):
            feat.grad = None
            f(feat).backward(dout)

        t = alternating_ms({"kernel": lambda: both(kernel_fwd), "composition": lambda: both(comp_fwd)}, args.warmup, args.iters)
        put(row, "fwdbwd_kernel", t["kernel"])
        put(row, "fwdbwd_composition", t["composition"])
        both(kernel_fwd)
        g = feat.grad.clone()
        both(comp_fwd)
        r = rec["rows"][row]
        r["grad_max_abs_diff_vs_composition"] = float((g - feat.grad).abs().max())
        for w in ("fwd", "fwdbwd"):
            r[w + "_speedup"] = r[w + "_composition_ms"] / r[w + "_kernel_ms"]
            # the run's own spread: the larger median-to-minimum gap of the two alternating series
            r[w + "_spread_ms"] = max(r[w + "_kernel_ms"] - r[w + "_kernel_min_ms"],
                                      r[w + "_composition_ms"] - r[w + "_composition_min_ms"])
            r[w + "_not_slower"] = r[w + "_kernel_ms"] <= r[w + "_composition_ms"] + r[w + "_spread_ms"]
        feat.requires_grad_(False)
        feat.grad = None

    # ---- grouping: the cloud on itself, K = 16, c = 32, with xyz
    k, c = 16, 32
    off = i32(n)
    idx, _ = ops.knn_query(k, xyz, xyz, off, off)
    feat = torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32)).to(dev)
    dout = torch.from_numpy(rng.standard_normal((n, k, 3 + c)).astype(np.float32)).to(dev)
    rec["rows"]["group"] = {"n": n, "m": n, "k": k, "c": c}
    out = ops.query_and_group(k, xyz, xyz, feat, idx, off, off)
    rec["rows"]["group"]["fwd_equal_to_composition"] = bool(torch.equal(out, group_composition(xyz, xyz, feat, idx)))
    compare("group", lambda f: ops.query_and_group(k, xyz, xyz, f, idx, off, off),
            lambda f: group_composition(xyz, xyz, f, idx), feat, dout)
    order, offsets = ops._pair_lists(idx, n, "cuda")
    lengths = (offsets[1:] - offsets[:-1]).float()
    rec["rows"]["group"]["list_length_median_max"] = [float(lengths.median()), float(lengths.max())]
    dxyz, dnew, dfeat = torch.empty_like(xyz), torch.empty_like(xyz), torch.empty_like(feat)
    ws = ops._workspace(_lib.query("seg3d_pointops_scratch_bytes", n, k, 3 + c), dev)
    entry("group", "group_fwd", lambda: _lib.call("seg3d_group_points_fwd", _ptr(xyz), _ptr(xyz), _ptr(feat), _ptr(idx), n, n,
                                                  k, c, _ptr(out), _stream()), (n, n, k, c))
    entry("group", "group_bwd", lambda: _lib.call("seg3d_group_points_bwd", _ptr(dout), _ptr(idx), _ptr(order), _ptr(offsets),
                                                  n, n, k, c, 1, _ptr(dxyz), _ptr(dnew), _ptr(dfeat), _ptr(ws), ws.numel(),
                                                  _stream()), (n, n, k, c))
    del out, dout, dxyz, dnew, dfeat, order, offsets, idx, feat

    # ---- interpolation: n queries over the n / 4 sectorized_fps picks, K = 3
    mp = n // 4
    picks = ops.sectorized_fps(xyz, off, i32(mp), 16)
    picked_xyz = xyz[picks].contiguous()
    k = 3
    idx, dist = ops.knn_query(k, picked_xyz, xyz, i32(mp), off)
    for c in (64, 256):
        row = f"interp_c{c}"
        rec["rows"][row] = {"n": mp, "m": n, "k": k, "c": c}
        feat = torch.from_numpy(rng.standard_normal((mp, c)).astype(np.float32)).to(dev)
        dout = torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32)).to(dev)
        out = ops.knn_interpolate(feat, idx, dist)
        rec["rows"][row]["fwd_max_abs_diff_vs_composition"] = float((out - interp_composition(feat, idx, dist)).abs().max())
        compare(row, lambda f: ops.knn_interpolate(f, idx, dist), lambda f: interp_composition(f, idx, dist), feat, dout)
        order, offsets = ops._pair_lists(idx, mp, "cuda")
        lengths = (offsets[1:] - offsets[:-1]).float()
        rec["rows"][row]["list_length_median_max"] = [float(lengths.median()), float(lengths.max())]
        weight, dfeat = torch.empty_like(dist), torch.empty_like(feat)
        ws = ops._workspace(_lib.query("seg3d_pointops_scratch_bytes", n, k, c), dev)
        entry(row, "interp_fwd", lambda: _lib.call("seg3d_knn_interpolate_fwd", _ptr(feat), _ptr(idx), _ptr(dist), mp, n, k, c,
                                                   _ptr(out), _ptr(weight), _stream()), (mp, n, k, c))
        entry(row, "interp_bwd", lambda: _lib.call("seg3d_knn_interpolate_bwd", _ptr(dout), _ptr(weight), _ptr(idx), _ptr(order),
                                                   _ptr(offsets), mp, n, k, c, _ptr(dfeat), _ptr(ws), ws.numel(), _stream()),
              (mp, n, k, c))
    # the condition: kernel median <= composition median + the spread the same run shows, on every timed row
    rec["kernel_not_slower_anywhere"] = all(r[w + "_not_slower"] for r in rec["rows"].values() for w in ("fwd", "fwdbwd"))
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
