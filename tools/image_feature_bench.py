#!/usr/bin/env python3
"""The per-point image-feature query on one Waymo-sized frame: the reference's Python loop, the host twin and the device
entry of csrc/image_features.hip, and the two file formats as the dataset reads them.

    python tools/image_feature_bench.py [--n 175000] [--iters 9] [--warmup 3] [--out profiles/image_feature_bench.json]

The frame: n float64 rows of 15 columns in range-image order (row = beam * 2650 + azimuth), C = 28, five (C, H, W) float32
maps of Waymo's image sizes (three of 1280 x 1920, two of 886 x 1920).  The projections are generated so that
neighbouring rows are neighbouring pixels: the azimuth sweeps each camera's width, the beam its height; rows near a
camera's edge carry a second projection into the neighbouring camera, 3 % carry none.  Every device row is timed twice:
rows in that order, and the same rows shuffled.
Per frame:
  numpy_loop     tests/image_feature_ref.query, the restatement of tools/extract_image_feature.py:84-100 (host clock);
  host_twin      ops.point_image_features_host (host clock);
  device_*       seg3d_point_image_features between two device events, maps resident: CHW float32 (what the image model
                 returns), HWC float32 (the same values, channel last), CHW float16;
  files          np.save of the dict and save_packed; then WaymoDataset._raw_image_features on the dict file and on the
                 packed file (host clock, this host's CPU and page cache).
Algorithmic bytes of the entry: n * 6 * point_bytes + hits * C * elem_bytes + n * C * 4 + n * 4, set against the 6.29 TB/s
measured copy rate of the card.  Medians and minima over --iters after --warmup.
Needs a GPU: without one the tool fails instead of timing something else.  Prints one JSON line and writes it to --out."""
import argparse
import ctypes
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

import image_feature_ref  # noqa: E402
from openseg3d_amd import _lib, config, image_features, ops  # noqa: E402
from openseg3d_amd.dataset import WaymoDataset  # noqa: E402
from openseg3d_amd.ops import _ptr, _stream  # noqa: E402

COPY_RATE_TBS = 6.29
CHANNELS = 28
IMAGE_SHAPES = ((1280, 1920), (1280, 1920), (1280, 1920), (886, 1920), (886, 1920))
BEAM_COLS = 2650


def frame_rows(n, shapes, seed=0):
    """float64 [n, 15] in range-image order with the six projection columns filled as described above."""
    rs = np.random.RandomState(seed)
    rows = rs.randn(n, 15)
    i = np.arange(n)
    beam, az = i // BEAM_COLS, i % BEAM_COLS
    beams = int(beam.max()) + 1
    span = BEAM_COLS / len(shapes)  # azimuth columns per camera
    cam = np.minimum((az / span).astype(np.int64), len(shapes) - 1)
    frac = az / span - cam
    h = np.array([s[0] for s in shapes])[cam]
    w = np.array([s[1] for s in shapes])[cam]
    rows[:, 6] = cam + 1
    rows[:, 7] = frac * (w - 1) + rs.rand(n) * 0.9
    rows[:, 8] = (beam + rs.rand(n) * 0.9) / beams * (h - 1)
    near = frac > 0.9  # the neighbouring camera sees the row too
    cam2 = (cam + 1) % len(shapes)
    h2 = np.array([s[0] for s in shapes])[cam2]
    w2 = np.array([s[1] for s in shapes])[cam2]
    rows[:, 9] = np.where(near, cam2 + 1, 0)
    rows[:, 10] = np.where(near, (frac - 0.9) * 0.5 * (w2 - 1), 0)
    rows[:, 11] = np.where(near, beam / beams * (h2 - 1), 0)
    none = rs.rand(n) < 0.03
    rows[none, 6:12] = 0
    return rows


def entry_bytes(n, hits, channels, point_bytes, elem_bytes):
    return n * 6 * point_bytes + hits * channels * elem_bytes + n * channels * 4 + n * 4


def host_ms(fn, warmup, iters):
    times = []
    for it in range(warmup + iters):
        t0 = time.perf_counter()
        fn()
        if it >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return times


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
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shrink", type=int, default=1, help="divide the image sizes (a rehearsal; the record says so)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_feature_bench.json"))
    args = ap.parse_args()
    if args.iters < 5:
        raise SystemExit("image_feature_bench: medians of at least 5 calls")
    if not torch.cuda.is_available():
        raise SystemExit("image_feature_bench: no GPU visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    n, C = args.n, CHANNELS
    shapes = [(h // args.shrink, w // args.shrink) for h, w in IMAGE_SHAPES]
    rec = {"tool": "image_feature_bench", "status": "measured" if args.shrink == 1 else "rehearsal",
           "device_name": torch.cuda.get_device_name(0), "n": n, "channels": C, "image_shapes": shapes,
           "row_dtype": "float64", "row_stride": 15, "iters": args.iters, "warmup": args.warmup,
           "unit": "one frame, milliseconds", "copy_rate_tbs": COPY_RATE_TBS, "rows": {}}

    def put(row, times, extra=None):
        rec["rows"][row] = {"ms": statistics.median(times), "min_ms": min(times)}
        rec["rows"][row].update(extra or {})

    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    chw = {k: torch.randn((C, h, w), generator=gen, device=dev) for k, (h, w) in enumerate(shapes)}
    host_maps = {k: m.cpu().numpy() for k, m in chw.items()}
    rows = frame_rows(n, shapes)
    shuffled = rows[np.random.RandomState(1).permutation(n)]

    # ---- host: the restatement loop and the twin
    loop_times = host_ms(lambda: image_feature_ref.query(rows, host_maps), 0, 3)
    features, cameras, outside = image_feature_ref.query(rows, host_maps)
    hits = len(features)
    rec["hits"], rec["outside"] = hits, outside
    put("numpy_loop", loop_times, {"calls": 3})
    twin = ops.point_image_features_host(rows, host_maps)
    put("host_twin", host_ms(lambda: ops.point_image_features_host(rows, host_maps), 1, 5), {"calls": 5})
    want_dense, want_cam = image_feature_ref.dense(features, cameras, n, C)
    rec["twin_equals_loop"] = bool(np.array_equal(twin[0], want_dense) and np.array_equal(twin[1], want_cam))
    twin_shuffled = ops.point_image_features_host(shuffled, host_maps)

    # ---- device: the entry between two events, maps resident
    dense = torch.empty((n, C), dtype=torch.float32, device=dev)
    camera = torch.empty((n,), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    d_rows = {"ordered": torch.from_numpy(rows).to(dev), "shuffled": torch.from_numpy(shuffled).to(dev)}
    expect = {"ordered": twin, "shuffled": twin_shuffled}

    def device_rows(tag, maps, elem_bytes, cast):
        table = ops.feature_map_table(maps, False, dev)
        for order, r in d_rows.items():
            fn = lambda: _lib.call("seg3d_point_image_features", ctypes.byref(table), _ptr(r), 8, n, 15, 6, _ptr(dense),
                                   _ptr(camera), _ptr(count), _stream())
            times = event_ms(fn, args.warmup, args.iters)
            nbytes = entry_bytes(n, hits, C, 8, elem_bytes)
            tbs = nbytes / (statistics.median(times) * 1e-3) / 1e12
            exp_dense = cast(expect[order][0])
            put(f"device_{tag}_{order}", times,
                {"bytes": nbytes, "tbs": tbs, "of_copy_rate": tbs / COPY_RATE_TBS,
                 "equals_twin": bool(np.array_equal(dense.cpu().numpy(), exp_dense)
                                     and np.array_equal(camera.cpu().numpy(), expect[order][1])),
                 "outside": int(count.item())})

    same = lambda a: a
    device_rows("chw_f32", chw, 4, same)
    hwc = {k: m.permute(1, 2, 0).contiguous().permute(2, 0, 1) for k, m in chw.items()}
    device_rows("hwc_f32", hwc, 4, same)
    del hwc
    torch.cuda.empty_cache()
    half = {k: m.half() for k, m in chw.items()}
    device_rows("chw_f16", half, 2, lambda a: a.astype(np.float16).astype(np.float32))
    del half
    torch.cuda.empty_cache()
    r = rec["rows"]
    rec["hwc_over_chw_ordered"] = r["device_hwc_f32_ordered"]["ms"] / r["device_chw_f32_ordered"]["ms"]
    rec["hwc_over_chw_shuffled"] = r["device_hwc_f32_shuffled"]["ms"] / r["device_chw_f32_shuffled"]["ms"]
    rec["shuffled_over_ordered_chw"] = r["device_chw_f32_shuffled"]["ms"] / r["device_chw_f32_ordered"]["ms"]
    rec["shuffled_over_ordered_hwc"] = r["device_hwc_f32_shuffled"]["ms"] / r["device_hwc_f32_ordered"]["ms"]

    # ---- files: the dict format against the packed one, through the dataset's reader
    with tempfile.TemporaryDirectory() as root:
        for d in ("lidar", "label", "image_feature"):
            os.makedirs(os.path.join(root, d))
        cfg = config.default_cfg()
        cfg.DATASET.USE_MULTI_SWEEPS, cfg.DATASET.USE_IMAGE_FEATURE, cfg.DATASET.DIM_IMAGE_FEATURE = True, True, C
        ds = WaymoDataset(cfg, root, "validation")
        stem = os.path.join(root, "image_feature", "frame_dict")
        put("save_dict", host_ms(lambda: image_features.save_dict(stem, twin[0], twin[1]), 0, 3), {"calls": 3})
        packed_stem = os.path.join(root, "image_feature", "frame_packed")
        put("save_packed", host_ms(lambda: image_features.save_packed(packed_stem, twin[0], twin[1]), 0, 3), {"calls": 3})
        put("load_dict_file", host_ms(lambda: ds._raw_image_features("frame_dict"), 1, 5),
            {"calls": 5, "file_bytes": os.path.getsize(stem + ".npy")})
        put("load_packed_file", host_ms(lambda: ds._raw_image_features("frame_packed"), 1, 5),
            {"calls": 5, "file_bytes": os.path.getsize(packed_stem + ".npz")})
        a, b = ds._raw_image_features("frame_dict"), ds._raw_image_features("frame_packed")
        rec["packed_equals_dict"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
        rec["load_dict_over_packed"] = r["load_dict_file"]["ms"] / r["load_packed_file"]["ms"]
    rec["host_cpus"] = os.cpu_count()
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
