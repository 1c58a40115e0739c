#!/usr/bin/env python3
"""Training augmentation, ms per frame: the reference's order of operations in numpy against TrainAugmentation.apply.

    python tools/aug_bench.py [--iters N] [--warmup W] [--out FILE]

Scenes: the seeded Waymo-shaped scene (scene.make_scene, ~175 k points) with PolarMix against a second scene, and the
3-sweep scene (scene.make_multi_sweep_scene) with cur_point_indices; uint8 labels, 28 image-feature columns.

(a) numpy: a restatement, written for this tool, of what the reference does per frame (polarmix.py:4-111, then
    transforms.py:79-258 in the order of waymo_dataset.py:44-50): np.delete / np.concatenate copies, the float64 paste
    rotation, float32 rotation / scale / translation / flips, np.random.shuffle, points_random_sampling, and for the
    multi-sweep frame the two dict loops over every point (get_shuffled_indices);
(b) device: TrainAugmentation.apply(rng="device") on frames already in HBM, and the same including the upload of the
    frame(s), labels and features from pageable host memory;
(c) the apply kernel alone, and its fraction of the 8 TB/s HBM peak by its algorithmic bytes
    (per output row: 4 B of map + 1 B of op + D input elements read + D float32 written).
Times are medians over the iterations after a warm-up; one stream, synchronised around each frame.  Prints one JSON line.
"""
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

from openseg3d_amd import ops, scene  # noqa: E402
from openseg3d_amd.augment import PolarMix, TrainAugmentation  # noqa: E402

ROT_RANGE, SCALE_RANGE, TRANSLATE_STD, SAMPLE_RATIO, SAMPLE_RANGE = [-0.78539816, 0.78539816], [0.95, 1.05], 0.5, 0.95, 50.0
INSTANCE_CLASSES = list(range(13))
PASTE_ANGLES = [0.9, 3.3]
HBM_PEAK = 8.0e12


def labels_of(seed, n):
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 22, n).astype(np.uint8)
    lab[rs.rand(n) < 0.1] = 255
    return lab


# ------------------------------------------------------------------------------------------------ (a) numpy
def np_polarmix(p1, f1, l1, p2, f2, l2, rs):
    out_p, out_f, out_l = p1, f1, l1
    if rs.random() < 0.5:
        alpha = (rs.random() - 1) * np.pi
        beta = alpha + np.pi
        yaw1, yaw2 = -np.arctan2(p1[:, 1], p1[:, 0]), -np.arctan2(p2[:, 1], p2[:, 0])
        i1, i2 = np.where((yaw1 > alpha) & (yaw1 < beta)), np.where((yaw2 > alpha) & (yaw2 < beta))
        out_p = np.concatenate((np.delete(p1, i1, axis=0), p2[i2]))
        out_l = np.concatenate((np.delete(l1, i1), l2[i2]))
        out_f = np.concatenate((np.delete(f1, i1, axis=0), f2[i2]))
    rs.random()
    sel = [np.where(l2 == c) for c in INSTANCE_CLASSES]
    pi, li, fi = (np.concatenate([a[s] for s in sel], axis=0) for a in (p2, l2, f2))
    pc, lc, fc = [pi], [li], [fi]
    for a in PASTE_ANGLES:
        m = np.array([[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1]])
        q = np.zeros_like(pi)
        q[:, :3] = np.dot(pi[:, :3], m)
        q[:, 3:] = pi[:, 3:]
        pc.append(q)
        lc.append(li)
        fc.append(fi)
    return (np.concatenate([out_p] + pc, axis=0), np.concatenate([out_f] + fc, axis=0), np.concatenate([out_l] + lc, axis=0))


def np_shuffled_indices(cur_point_indices, point_indices):
    point_to_cur = {}
    for i, p in enumerate(cur_point_indices):
        point_to_cur[p] = i
    cur_idx, glb_idx = [], []
    for i, p in enumerate(point_indices):
        if p in point_to_cur:
            cur_idx.append(point_to_cur[p])
            glb_idx.append(i)
    return np.array(cur_idx), np.array(glb_idx)


def np_transforms(points, feats, labels, cur, rs):
    a = np.float32(rs.uniform(*ROT_RANGE))
    c, s = np.cos(a), np.sin(a)
    pts = points.astype(np.float32)
    rot = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], np.float32)
    pts = np.concatenate((pts[:, :3] @ rot, pts[:, 3:]), axis=-1)
    pts[:, :3] *= rs.uniform(*SCALE_RANGE)
    for j in range(3):
        pts[:, j] += rs.normal(0, TRANSLATE_STD, 1)
    if rs.choice([False, True], replace=False, p=[0.5, 0.5]):
        pts[:, 1] = -pts[:, 1]
    if rs.choice([False, True], replace=False, p=[0.5, 0.5]):
        pts[:, 0] = -pts[:, 0]
    for step in range(2):
        n = pts.shape[0]
        if step == 0:
            idx = np.array(range(n))
            rs.shuffle(idx)
        else:
            num = min(int(n * SAMPLE_RATIO), n)
            dist = np.linalg.norm(pts[:, :2], axis=1)
            far, near = np.where(dist >= SAMPLE_RANGE)[0], np.where(dist < SAMPLE_RANGE)[0]
            if len(far) > num:
                far = rs.choice(far, num, replace=False)
            idx = np.concatenate((far, rs.choice(near, num - len(far), replace=False)))
            rs.shuffle(idx)
        pts = pts[idx]
        if cur is not None:
            sel, cur = np_shuffled_indices(cur, idx)
        else:
            sel = idx
        feats, labels = feats[sel], labels[sel]
    return pts, feats, labels, cur


# ------------------------------------------------------------------------------------------------ timing
def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times)


def bench_scene(name, frame, labels, feats, frame2, labels2, feats2, cur, args, dev):
    pm = None if cur is not None else PolarMix(INSTANCE_CLASSES, PASTE_ANGLES)
    aug = TrainAugmentation(ROT_RANGE, SCALE_RANGE, TRANSLATE_STD, SAMPLE_RATIO, SAMPLE_RANGE, polar_mix=pm, rng="device")
    rs = np.random.RandomState(0)

    def host():
        if cur is None:
            p, f, lab = np_polarmix(frame, feats, labels, frame2, feats2, labels2, rs)
            return np_transforms(p, f, lab, None, rs)
        return np_transforms(frame, feats, labels, cur, rs)

    np_ms, np_min = median_ms(host, 1, max(2, args.iters // 5))

    def up(a):
        return None if a is None else torch.from_numpy(a).to(dev)

    res = [up(a) for a in (frame, labels, feats, frame2, labels2, feats2, cur)]
    seeds = iter(range(10 ** 6))

    def resident():
        return aug.apply(res[0], res[1], res[2], res[3], res[4], res[5], cur_point_indices=res[6], seed=next(seeds))

    def with_upload():
        t = [up(a) for a in (frame, labels, feats, frame2, labels2, feats2, cur)]
        return aug.apply(t[0], t[1], t[2], t[3], t[4], t[5], cur_point_indices=t[6], seed=next(seeds))

    dev_ms, dev_min = median_ms(resident, args.warmup, args.iters)
    up_ms, up_min = median_ms(with_upload, args.warmup, args.iters)

    # (c) the apply kernel alone, on the map of one frame
    out = resident()
    src = out["source_rows"]
    p = aug._params(out["draw"], None)
    op = torch.zeros_like(src, dtype=torch.uint8)
    n_out, d = int(src.shape[0]), int(frame.shape[1])
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        ops.aug_apply(res[0], res[3], src, op, p)
    reps = 50
    start.record()
    for _ in range(reps):
        ops.aug_apply(res[0], res[3], src, op, p)
    stop.record()
    torch.cuda.synchronize()
    k_ms = start.elapsed_time(stop) / reps  # launch-to-launch average of back-to-back launches, output buffers from the pool
    nbytes = n_out * (4 + 1 + d * frame.itemsize + d * 4)
    return {"scene": name, "n_points": int(frame.shape[0]), "n_points2": 0 if frame2 is None else int(frame2.shape[0]),
            "n_out": n_out, "input_dtype": str(frame.dtype),
            "numpy_ms": np_ms, "numpy_min_ms": np_min, "device_resident_ms": dev_ms, "device_resident_min_ms": dev_min,
            "device_with_upload_ms": up_ms, "device_with_upload_min_ms": up_min,
            "speedup_resident": np_ms / dev_ms, "speedup_with_upload": np_ms / up_ms,
            "apply_kernel_ms": k_ms, "apply_algorithmic_bytes": nbytes,
            "apply_fraction_of_hbm_peak": nbytes / (k_ms * 1e-3) / HBM_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    results = []
    f1, f2 = scene.make_scene(1), scene.make_scene(2)
    results.append(bench_scene("one_sweep_polarmix", f1, labels_of(1, len(f1)), scene.make_image_features(1, len(f1)),
                               f2, labels_of(2, len(f2)), scene.make_image_features(2, len(f2)), None, args, dev))
    ms, n_cur = scene.make_multi_sweep_scene(1)
    results.append(bench_scene("three_sweeps", ms, labels_of(3, n_cur), scene.make_image_features(3, n_cur), None, None,
                               None, np.arange(n_cur), args, dev))
    line = json.dumps({"tool": "aug_bench", "device_name": torch.cuda.get_device_name(0), "iters": args.iters,
                       "warmup": args.warmup, "rng": "device", "scenes": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
