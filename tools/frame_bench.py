#!/usr/bin/env python3
"""Frame assembly, ms per frame of the 175 k-point scene: the numpy restatements of tests/frame_ref.py on the host
against the device entries of csrc/frame.hip.

    python tools/frame_bench.py [--iters N] [--warmup W] [--out FILE]

Scene: the seeded Waymo-shaped scene of the benchmark (scene.make_scene, ~175 k points per sweep), widened to the raw
float64 [N, 15] rows of a lidar file; history sweeps carry a real pose product.  Reported, at 3 and 5 sweeps:

  merge_numpy_ms        frame_ref.merge_sweeps on the host (per sweep a copy, tanh, three dot products, a concatenate)
  merge_resident_ms     seg3d_frame_assemble with the raw rows already in HBM, writing the collated float32 layout
  merge_with_upload_ms  the same including the upload of each sweep's [:, :6] columns from pageable host memory
  fraction_of_8TBps     the kernel's algorithmic bytes (rows read once, the collated rows written once) over the
                        resident time, as a fraction of 8 TB/s
then the range-image loop (frame_ref.range_images, the reference's per-point Python loop) against
seg3d_range_image_labels on one sweep's points, and WaymoDataset(device="cuda").assemble end to end for a validation
batch of 2 multi-sweep frames read from a temporary directory (file reading timed apart).  Last, 8 consecutive frames
in frame order, one ``load_raw`` + ``assemble`` each, at NUM_SWEEPS = 3 and 5: ``sweep_cache`` off (every history sweep
read and uploaded again) against on (each file read and uploaded once), ms per frame with the file reads, bytes uploaded
per frame and files read.
Times are medians over the iterations after a warm-up; one stream, synchronised around each call.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frame_ref  # noqa: E402
from openseg3d_amd import config, ops, scene  # noqa: E402
from openseg3d_amd.dataset import WaymoDataset  # noqa: E402

DIM = 6


def raw_sweep(seed):
    pts = scene.make_scene(seed).astype(np.float64)
    rs = np.random.RandomState(seed)
    n = len(pts)
    raw = np.zeros((n, 15))
    raw[:, :DIM] = pts[:, :DIM]
    raw[:, 4] = 6.0 * rs.rand(n) ** 3
    raw[:, 6:12] = rs.randint(0, 1900, (n, 6))
    raw[:, 12], raw[:, 13], raw[:, 14] = rs.randint(0, 2650, n), rs.randint(0, 64, n), rs.randint(0, 2, n)
    return raw


def pose(i):
    yaw = 0.02 * (i + 1)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    m[:3, 3] = [35.0 + 1.7 * i, -62.0 + 0.9 * i, 3.0 + 0.05 * i]
    return m


def median_ms(fn, warmup, iters, sync):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def merge_numbers(raws, n_sweeps, dev, args):
    raws = raws[:n_sweeps]
    mats = [None] + [np.linalg.inv(pose(0)) @ pose(i) for i in range(1, n_sweeps)]
    lags = [0.1 * i for i in range(n_sweeps)]
    views = [r[:, :DIM] for r in raws]
    resident = [torch.from_numpy(r).to(dev)[:, :DIM] for r in raws]
    table = ops.sweep_table(resident, mats, lags)

    def with_upload():
        up = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in views]
        return ops.frame_assemble(ops.sweep_table(up, mats, lags), want=("collated",))

    rows = sum(len(r) for r in raws)
    numpy_ms = median_ms(lambda: frame_ref.merge_sweeps(raws, mats, lags, DIM), 1, max(3, args.iters // 4), False)
    res_ms = median_ms(lambda: ops.frame_assemble(table, want=("collated",)), args.warmup, args.iters, True)
    up_ms = median_ms(with_upload, args.warmup, args.iters, True)
    nbytes = rows * (DIM * 8 + (DIM + 1) * 4)
    return {"rows": rows, "merge_numpy_ms": numpy_ms, "merge_resident_ms": res_ms, "merge_with_upload_ms": up_ms,
            "algorithmic_bytes": nbytes, "fraction_of_8TBps": nbytes / (res_ms * 1e-3) / 8e12}


def write_dataset(root, raws):
    for d in ("lidar", "label", "pose"):
        os.makedirs(os.path.join(root, d))
    rs = np.random.RandomState(0)
    for i, raw in enumerate(raws):
        name = f"bench-{1550083467346370 + 100000 * i}-{i}"
        np.save(os.path.join(root, "lidar", name + ".npy"), raw)
        np.save(os.path.join(root, "label", name + ".npy"), rs.randint(0, 23, (len(raw), 2)).astype(np.int32))
        np.savetxt(os.path.join(root, "pose", name + ".txt"), pose(i))


def sweep_cache_numbers(root, n_sweeps, dev, passes):
    """One pass over the directory's frames in frame order, ``load_raw`` + ``assemble`` of one frame at a time, from a
    cold cache: per frame the wall time (files included: the cache moves the history reads from ``load_raw`` into
    ``assemble`` and drops most of them), the bytes uploaded and the lidar files read."""
    cfg = config.default_cfg()
    cfg.DATASET.USE_MULTI_SWEEPS = True
    cfg.DATASET.NUM_SWEEPS = n_sweeps

    def one_pass(cache):
        ds = WaymoDataset(cfg, root, "validation", device=dev, sweep_cache=cache)
        order = sorted(range(len(ds)), key=lambda i: ds.parse_filename(ds.filenames[i])[1])
        count = {"bytes": 0, "files": 0}
        upload, raw_points = ds._upload, ds._raw_points

        def counting_upload(a):
            t = upload(a)
            count["bytes"] += t.numel() * t.element_size()
            return t

        def counting_read(name):
            count["files"] += 1
            return raw_points(name)

        ds._upload, ds._raw_points = counting_upload, counting_read
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in order:
            ds.assemble([ds[i]])
        torch.cuda.synchronize()
        n = len(order)
        return {"ms_per_frame": (time.perf_counter() - t0) * 1e3 / n, "uploaded_bytes_per_frame": count["bytes"] / n,
                "lidar_files_read": count["files"], "frames": n}

    out = {}
    for key, cache in (("cache_off", None), ("cache_on", cfg.DATASET.MAX_NUM_SWEEPS)):
        one_pass(cache)  # warm-up: the page cache holds the files afterwards, for both
        runs = [one_pass(cache) for _ in range(passes)]
        ms = [r["ms_per_frame"] for r in runs]
        out[key] = dict(runs[0], ms_per_frame=statistics.median(ms), ms_per_frame_min=min(ms), ms_per_frame_max=max(ms),
                        passes=passes)
    out["speedup"] = out["cache_off"]["ms_per_frame"] / out["cache_on"]["ms_per_frame"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    raws = [raw_sweep(s) for s in range(8)]
    out = {"tool": "frame_bench", "status": "measured", "device_name": torch.cuda.get_device_name(0), "iters": args.iters,
           "warmup": args.warmup, "input_dtype": "float64", "dim": DIM}
    for n_sweeps in (3, 5):
        out[f"sweeps{n_sweeps}"] = merge_numbers(raws, n_sweeps, dev, args)

    ri = np.ascontiguousarray(raws[0][:, -3:].astype(np.int32))
    pred = np.random.RandomState(1).randint(0, 22, len(ri))
    pred_d, ri_d = torch.from_numpy(pred).to(dev), torch.from_numpy(ri).to(dev)
    out["range_image"] = {
        "points": int(len(ri)),
        "numpy_loop_ms": median_ms(lambda: frame_ref.range_images(pred, ri), 0, 3, False),
        "device_ms": median_ms(lambda: ops.range_image_labels(pred_d, ri_d, 22), args.warmup, args.iters, True)}

    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, raws[:4])
        cfg = config.default_cfg()
        cfg.DATASET.USE_MULTI_SWEEPS = True
        ds = WaymoDataset(cfg, root, "validation", device=dev)
        order = sorted(range(len(ds)), key=lambda i: ds.filenames[i])
        pair = [order[2], order[3]]  # two frames with two history sweeps each
        load_ms = median_ms(lambda: [ds[i] for i in pair], 1, 3, False)
        raw_list = [ds[i] for i in pair]
        asm_ms = median_ms(lambda: ds.assemble(raw_list), args.warmup, max(5, args.iters // 2), True)
        batch = ds.assemble(raw_list)
        out["assemble_batch2"] = {"rows": int(batch["points"].shape[0]), "voxels": int(batch["voxel_coords"].shape[0]),
                                  "load_raw_ms": load_ms, "assemble_ms": asm_ms}

    with tempfile.TemporaryDirectory() as root:  # 8 consecutive frames: WaymoDataset(sweep_cache=...) off against on
        write_dataset(root, raws)
        out["sweep_cache_8_frames"] = {f"sweeps{n}": sweep_cache_numbers(root, n, dev, 10) for n in (3, 5)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
