#!/usr/bin/env python3
"""Instance copy-paste augmentation, ms per frame: a vectorised numpy restatement against InstanceAugmentation.__call__
on the device.

    python tools/instaug_bench.py [--iters N] [--warmup W] [--out FILE]

Scene: the seeded Waymo-shaped scene of the benchmark (scene.make_scene, ~175 k points, float32, 6 columns) with uint8
labels whose low rows are ground classes, and a synthetic bank (labels 3, 4, 10 x 8 clusters of 100-600 points: the
bank is only a dict of arrays, tools/extract_instances.py:65-76).  Every frame draws afresh from a seeded RandomState,
the same draws for both sides.

(a) numpy: a restatement, written for this tool, of instance_augmentation.py:25-107 with the per-point Python loop of
    :35-43 replaced by masks (the loop itself is what makes the reference class take seconds per frame on a host CPU);
    per instance two masked copies of the frame, per candidate two distance passes;
(b) device: InstanceAugmentation.__call__ on a frame already in HBM (bank uploaded once): 2 k + 1 launches and the one
    host read of the counts; also the same through the host entry of the library (no GPU).
Times are medians over the iterations after a warm-up; one stream, synchronised around each frame.  Prints one JSON
line with the launch count."""
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

from openseg3d_amd import scene  # noqa: E402
from openseg3d_amd.augment import InstanceAugmentation, InstanceBank  # noqa: E402

GROUND_IDS = [17, 18, 19, 20, 21]
INSTANCE_IDS = [3, 4, 10]


def labels_of(points, seed):
    """Ground classes for the lowest third of the rows, object classes above, a tenth ignored."""
    rs = np.random.RandomState(seed)
    n = len(points)
    lab = rs.randint(0, 17, n).astype(np.uint8)
    low = points[:, 2] < np.percentile(points[:, 2], 35)
    lab[low] = rs.randint(17, 22, int(low.sum())).astype(np.uint8)
    lab[rs.rand(n) < 0.1] = 255
    return lab


def make_bank(points, labels, seed, dim):
    rs = np.random.RandomState(seed)
    zg = float(np.median(points[np.isin(labels, GROUND_IDS), 2]))
    bank = {}
    for lab in INSTANCE_IDS:
        bank[lab] = []
        for _ in range(8):
            m = rs.randint(100, 601)
            d, a = rs.uniform(6, 40), rs.rand() * 2 * np.pi
            h, s = rs.uniform(0.8, 1.8), rs.uniform(0.3, 0.9)
            xyz = np.stack([d * np.cos(a) + s * rs.randn(m), d * np.sin(a) + s * rs.randn(m), zg + h * rs.rand(m)], axis=1)
            pts = np.concatenate([xyz, rs.randn(m, dim - 3)], axis=1).astype(np.float32)
            bank[lab].append({"cluster_points": pts, "cluster_height": float(xyz[:, 2].mean() - zg)})
    return bank


def np_rot(xyz, r):
    out = xyz.copy()
    out[:, 0] = xyz[:, 0] * np.cos(r) + xyz[:, 1] * np.sin(r)
    out[:, 1] = -xyz[:, 0] * np.sin(r) + xyz[:, 1] * np.cos(r)
    return out


def np_instance_aug(points, labels, bank, draw):
    for i in range(len(draw)):
        keep = labels != 255
        ground = keep & np.isin(labels, GROUND_IDS)
        gp, op = points[ground, :3], points[keep & ~ground, :3]
        inst = bank[draw.label[i]][draw.index[i]]
        pts = inst["cluster_points"].copy()
        xyz, feat = pts[:, :3], pts[:, 3:]
        feat[:, 0] = 0
        feat[:, 1] = np.tanh(feat[:, 1])
        c0 = np.mean(xyz, axis=0)
        xyz = np_rot(xyz - c0, draw.rot_noise[i]) + draw.loc_noise[i][None, :] + c0
        if draw.flip_type[i] == 3:
            ax = np.array([c0[0], c0[1]]) / (c0[0] ** 2 + c0[1] ** 2) ** 0.5
            a, b = -ax[1], ax[0]
            m = np.array([[b ** 2 - a ** 2, -2 * a * b], [-2 * a * b, a ** 2 - b ** 2]])
            xyz[:, :2] = (xyz[:, :2] - c0[:2]) @ m.T + c0[:2]
        center = np.mean(xyz, axis=0)
        radius = np.max(np.linalg.norm(xyz - center, axis=1))
        for r in draw.angles[i]:
            c = np_rot(center[None, :], r)[0]
            if not np.all(np.linalg.norm(op - c, axis=1) > radius):
                continue
            gd = np.linalg.norm(gp - c, axis=1)
            if not np.any(gd < 1.2 * radius):
                continue
            xyz[:, 2] += gp[np.argmin(gd), 2] + inst["cluster_height"] - c[2]
            xyz = np_rot(xyz, r)
            points = np.concatenate((points, np.concatenate((xyz, feat), axis=1)), axis=0)
            labels = np.concatenate((labels, np.full(len(xyz), draw.label[i], labels.dtype)))
            break
    return points, labels


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
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    frame = scene.make_scene(1)
    labels = labels_of(frame, 1)
    bank = make_bank(frame, labels, 5, frame.shape[1])
    ia = InstanceAugmentation(InstanceBank(bank).to(dev))
    draws = [ia.draw(np.random.RandomState(1000 + i)) for i in range(args.warmup + args.iters)]

    def cycle(fn):
        it = iter(draws * 2)
        return lambda: fn(next(it))

    placed = []

    def on_device(d):
        out = ia(frame_d, None, labels_d, draw=d)
        placed.append(sum(c >= 0 for c in ia.last_decisions))
        return out

    frame_d, labels_d = torch.from_numpy(frame).to(dev), torch.from_numpy(labels).to(dev)
    np_ms, np_min = median_ms(cycle(lambda d: np_instance_aug(frame, labels, bank, d)), 1, max(3, args.iters // 4), False)
    host_ms, host_min = median_ms(cycle(lambda d: ia(frame, None, labels, draw=d)), 1, max(3, args.iters // 4), False)
    dev_ms, dev_min = median_ms(cycle(on_device), args.warmup, args.iters, True)
    k = ia.add_count
    line = json.dumps({"tool": "instaug_bench", "device_name": torch.cuda.get_device_name(0), "iters": args.iters,
                       "warmup": args.warmup, "n_points": int(frame.shape[0]), "input_dtype": str(frame.dtype),
                       "instances_per_frame": k, "launches_per_frame": 2 * k + 1,
                       "mean_instances_placed": float(np.mean(placed[args.warmup:])),
                       "numpy_ms": np_ms, "numpy_min_ms": np_min, "host_entry_ms": host_ms, "host_entry_min_ms": host_min,
                       "device_resident_ms": dev_ms, "device_resident_min_ms": dev_min, "speedup_resident": np_ms / dev_ms})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
