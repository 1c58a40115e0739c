#!/usr/bin/env python3
"""SALayer on the four levels of the headline 175 k-point scene (C = 48, 96, 192, 384): the fused op of csrc/sa_gate.hip
(ops.sa_gate) against the only composition available without it -- the [1, 3, 3, 3, C] weight zero-padded to 16 output
columns through the implicit-GEMM path (SubMConv3d(C, 16) -> ops.sparse_conv), column 0, torch.sigmoid and a multiply.

    python tools/sa_bench.py [--iters 15] [--warmup 5] [--out profiles/sa_bench.json]

Per level: forward (no grad), and forward + backward (gradients of x and of the weight, dy given), fused op and
composition alternating in the same run; one timed unit = one call, host clock around the call and a device synchronise;
medians and minima over --iters after --warmup.  Each C entry is also timed on its own between two device events, and its
algorithmic bytes (entry_bytes() below: every array read or written once, whatever the number of times a row is gathered)
over that time are set against 8 TB/s.  The site levels and their tables are built once, outside every timed window.
Needs a GPU: without one the tool fails instead of timing something else.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd import _lib, batch as B, config, ops, scene, segformer, spconv  # noqa: E402
from openseg3d_amd.ops import _ptr, _stream  # noqa: E402

PEAK_TBS = 8.0
ROWS = 128  # SEG3D_SUBM_DOT_ROWS


def entry_bytes(kind, m, c, nnz):
    """Algorithmic bytes of one C entry; nnz = present entries of the table (the gathered-row count, reported beside it)."""
    table = 27 * m * 4
    if kind == "fwd":      # x, the table, w; s and y
        return m * c * 4 + table + 27 * c * 4 + m * 4 + m * c * 4
    if kind == "bwd_ds":   # dy, x, s; ds
        return 2 * m * c * 4 + 2 * m * 4
    if kind == "bwd":      # dy, x, s, ds, the table, w; dx; the block partials written and read back; dw
        blocks = -(-m // ROWS)
        return 2 * m * c * 4 + 2 * m * 4 + table + 27 * c * 4 + m * c * 4 + 2 * blocks * 27 * c * 4 + 27 * c * 4
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
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa_bench.json"))
    args = ap.parse_args()
    if args.iters < 5:
        raise SystemExit("sa_bench: medians of at least 5 calls")
    if not torch.cuda.is_available():
        raise SystemExit("sa_bench: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    cfg = config.default_cfg()
    ds = config.DatasetSpec(cfg)
    b = B.make_batch([scene.make_scene(0)], ds.voxel_size, ds.point_cloud_range)
    shape = [int(g) for g in ops.grid_size(ds.voxel_size, ds.point_cloud_range)][::-1]
    level = spconv.SiteLevel(b["voxel_coords"].int(), shape, b["batch_size"])
    level.seed_chain(3)
    rec = {"tool": "sa_bench", "status": "measured", "device_name": torch.cuda.get_device_name(0), "iters": args.iters,
           "warmup": args.warmup, "unit": "one call, microseconds", "peak_tbs": PEAK_TBS, "rows": {}}
    torch.manual_seed(0)
    for c in (48, 96, 192, 384):
        nbr = level.subm()
        m = int(nbr.shape[1])
        nnz = int((nbr >= 0).sum())
        row = rec["rows"][f"c{c}"] = {"m": m, "c": c, "table_entries": nnz, "neighbours_per_row": nnz / max(m, 1)}
        x = torch.randn(m, c, device=dev)
        dy = torch.randn(m, c, device=dev)
        sa = segformer.SALayer(c).to(dev)
        conv16 = spconv.SubMConv3d(c, 16, 3, padding=1, bias=False).to(dev)
        with torch.no_grad():
            conv16.weight.zero_()
            conv16.weight[0].copy_(sa.conv.weight[0])

        def fused(xi):
            return sa(spconv.SparseConvTensor(xi, level.coords, level.shape, level.batch_size, level)).features

        def composed(xi):
            s = conv16(spconv.SparseConvTensor(xi, level.coords, level.shape, level.batch_size, level)).features[:, :1]
            return xi * torch.sigmoid(s)

        def put(name, times):
            row[name + "_us"], row[name + "_min_us"] = statistics.median(times) * 1e3, min(times) * 1e3

        with torch.no_grad():
            row["fwd_max_abs_diff_vs_composition"] = float((fused(x) - composed(x)).abs().max())
            t = alternating_ms({"fused": lambda: fused(x), "composition": lambda: composed(x)}, args.warmup, args.iters)
        put("fwd_fused", t["fused"])
        put("fwd_composition", t["composition"])
        xg = x.clone().requires_grad_()

        def both(f, mod):
            xg.grad = None
            mod.weight.grad = None
            f(xg).backward(dy)

        t = alternating_ms({"fused": lambda: both(fused, sa.conv), "composition": lambda: both(composed, conv16)},
                           args.warmup, args.iters)
        put("fwdbwd_fused", t["fused"])
        put("fwdbwd_composition", t["composition"])
        both(fused, sa.conv)
        gx, gw = xg.grad.clone(), sa.conv.weight.grad.clone()
        both(composed, conv16)
        row["dx_max_abs_diff_vs_composition"] = float((gx - xg.grad).abs().max())
        row["dw_max_abs_diff_vs_composition"] = float((gw[0] - conv16.weight.grad[0]).abs().max())
        for w in ("fwd", "fwdbwd"):
            row[w + "_speedup"] = row[w + "_composition_us"] / row[w + "_fused_us"]
            row[w + "_spread_us"] = max(row[w + "_fused_us"] - row[w + "_fused_min_us"],
                                        row[w + "_composition_us"] - row[w + "_composition_min_us"])
            row[w + "_fused_not_slower"] = row[w + "_fused_us"] <= row[w + "_composition_us"] + row[w + "_spread_us"]
        # the C entries on their own
        wf = sa.conv.weight.detach().reshape(27, c).contiguous()
        s, dsv = torch.empty(m, device=dev), torch.empty(m, device=dev)
        y, dx, dw = torch.empty_like(x), torch.empty_like(x), torch.empty_like(wf)
        ws = ops._workspace(_lib.query("seg3d_subm_dot_scratch_bytes", m, c), dev)
        entries = {
            "fwd": lambda: _lib.call("seg3d_subm_dot_fwd", _ptr(x), _ptr(nbr), _ptr(wf), None, m, c, _ptr(s), _ptr(y), _stream()),
            "bwd_ds": lambda: _lib.call("seg3d_subm_dot_bwd_ds", _ptr(dy), _ptr(x), _ptr(s), m, c, _ptr(dsv), _stream()),
            "bwd": lambda: _lib.call("seg3d_subm_dot_bwd", _ptr(dy), _ptr(x), _ptr(s), _ptr(dsv), _ptr(nbr), _ptr(wf), m, c,
                                     _ptr(dx), _ptr(dw), None, _ptr(ws), ws.numel(), _stream()),
        }
        for kind, fn in entries.items():
            times = event_ms(fn, args.warmup, args.iters)
            put("entry_" + kind, times)
            nbytes = entry_bytes(kind, m, c, nnz)
            row["entry_" + kind + "_bytes"] = nbytes
            row["entry_" + kind + "_tbs"] = nbytes / (statistics.median(times) * 1e-3) / 1e12
            row["entry_" + kind + "_of_peak"] = row["entry_" + kind + "_tbs"] / PEAK_TBS
        row["fwd_gathered_row_bytes"] = nnz * c * 4  # what the forward's loads ask the caches for
        del x, dy, y, dx, xg, gx
        if c != 384:
            level = level.down()[0]
    rec["fused_not_slower_anywhere"] = all(r[w + "_fused_not_slower"] for r in rec["rows"].values() for w in ("fwd", "fwdbwd"))
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
