#!/usr/bin/env python3
"""Instance bank extraction, ms per frame: the reference's loop (tools/extract_instances.py:46-76, once per label)
against InstanceBankBuilder.add on the device.

    python tools/instbank_bench.py [--iters N] [--warmup W] [--out FILE]

Frame: the seeded Waymo-shaped scene of the benchmark (scene.make_scene, ~175 k points, float32, 6 columns).  Its lowest
rows get ground labels; around 36 seeded spots on the ground, clumps of a few hundred rows each are relabelled 3, 4 or
10 (a few thousand target rows per label), the rest get other object classes.

(a) reference loop: a restatement, written for this tool, of :46-76 run for the three labels one after the other, as the
    script has to be: the per-point Python loop of :47-50 for the ground rows, sklearn's DBSCAN when sklearn imports and
    otherwise the brute-force numpy rule of the tests (``"dbscan"`` in the record says which), numpy for the rest;
(b) the same with the ground rows taken by a mask (what one would write first), so that the DBSCAN + statistics part
    shows on its own;
(c) device: InstanceBankBuilder.add on a frame already in HBM -- one call for all labels, the read-back of the table
    and of the kept rows included; also the same through the host entry of the library (no GPU).
Times are medians over the iterations after a warm-up; one stream, synchronised around each frame.  Prints one JSON
line; ``status`` is "measured" only when it ran on a GPU."""
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
from openseg3d_amd.augment import InstanceBankBuilder  # noqa: E402

GROUND_IDS = [17, 18, 19, 20, 21]
TARGETS = {3: 120, 4: 30, 10: 30}  # the script's three comment values
EPS = 0.25

try:
    from sklearn.cluster import DBSCAN
    DBSCAN_IMPL = "sklearn"
except ImportError:
    DBSCAN = None
    DBSCAN_IMPL = "numpy"


def np_dbscan(xy, eps, min_points):
    """The DBSCAN rule of include/seg3d_hip.h by brute force (tests/instbank_ref.py: dbscan_ref)."""
    xy = xy.astype(np.float64)
    m = len(xy)
    out = np.full(m, -1, dtype=np.int64)
    dx, dy = xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1]
    nb = (dx * dx + dy * dy) <= eps * eps
    core = nb.sum(1) >= min_points
    cnb = nb & core[None, :]
    nxt = 0
    for i in range(m):
        if not core[i] or out[i] >= 0:
            continue
        seen = np.zeros(m, dtype=bool)
        seen[i] = True
        front = np.array([i])
        while len(front):
            new = cnb[front].any(0) & ~seen
            seen |= new
            front = np.nonzero(new)[0]
        out[seen] = nxt
        nxt += 1
    for i in np.nonzero(~core)[0]:
        ids = out[cnb[i]]
        if len(ids):
            out[i] = ids.min()
    return out


def make_frame(seed):
    rs = np.random.RandomState(seed)
    points = scene.make_scene(seed)
    n = len(points)
    labels = rs.randint(0, 17, n).astype(np.uint8)
    labels[np.isin(labels, list(TARGETS))] = 0
    low = points[:, 2] < np.percentile(points[:, 2], 35)
    labels[low] = rs.randint(17, 22, int(low.sum())).astype(np.uint8)
    zg = float(np.median(points[low, 2]))
    free = np.nonzero(~low)[0]
    rs.shuffle(free)
    at = 0
    for i in range(36):
        m = rs.randint(150, 500)
        rows = free[at:at + m]
        at += m
        d, a = rs.uniform(6, 45), rs.rand() * 2 * np.pi
        s = 0.15 if i % 3 == 0 else 0.35  # label 3 needs 120 rows within eps
        points[rows, 0] = d * np.cos(a) + s * rs.randn(m)
        points[rows, 1] = d * np.sin(a) + s * rs.randn(m)
        points[rows, 2] = zg + 1.5 * rs.rand(m)
        labels[rows] = list(TARGETS)[i % 3]
    labels[rs.rand(n) < 0.05] = 255
    return points, labels


def reference_loop(points, labels, python_ground_loop):
    out = {}
    for target, min_points in TARGETS.items():  # the script is edited and run once per label
        if python_ground_loop:
            ground = []
            for i in range(points.shape[0]):
                if labels[i] in GROUND_IDS:
                    ground.append(points[i, :3])
            ground = np.stack(ground)
        else:
            ground = points[np.isin(labels, GROUND_IDS), :3]
        tp = points[labels == target]
        out[target] = []
        if tp.shape[0] < min_points:
            continue
        ids = DBSCAN(eps=EPS, min_samples=min_points).fit(tp[:, :2]).labels_ if DBSCAN else np_dbscan(tp[:, :2], EPS, min_points)
        for c in set(ids.tolist()) - {-1}:
            cp = tp[ids == c]
            center = np.mean(cp[:, :3], axis=0)
            radius = np.max(np.linalg.norm(cp[:, :3] - center, axis=1))
            dist = np.linalg.norm(ground - center, axis=1)
            ind = dist < 1.2 * radius
            if ind.any():
                out[target].append({"cluster_height": center[2] - ground[ind][np.argmin(dist[ind])][2], "cluster_points": cp})
    return out


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
    points, labels = make_frame(1)
    rec = {"tool": "instbank_bench", "status": "unmeasured", "dbscan": DBSCAN_IMPL, "iters": args.iters, "warmup": args.warmup,
           "n_points": int(points.shape[0]), "input_dtype": str(points.dtype),
           "target_rows": {str(t): int((labels == t).sum()) for t in TARGETS}}

    def builder():
        return InstanceBankBuilder(list(TARGETS), TARGETS, GROUND_IDS, EPS)

    want = reference_loop(points, labels, False)
    b = builder()
    b.add(points, labels)
    rec["instances_per_frame"] = {str(t): len(b.instances[t]) for t in TARGETS}
    rec["clusters_found"], rec["clusters_kept"] = b.last_counts[0], b.last_counts[1]
    rec["same_instances_as_the_loop"] = all(
        len(b.instances[t]) == len(want[t]) and
        sorted(len(i["cluster_points"]) for i in b.instances[t]) == sorted(len(i["cluster_points"]) for i in want[t]) for t in TARGETS)
    few = max(3, args.iters // 4)
    rec["reference_loop_ms"], rec["reference_loop_min_ms"] = median_ms(lambda: reference_loop(points, labels, True), 0, 3, False)
    rec["masked_loop_ms"], rec["masked_loop_min_ms"] = median_ms(lambda: reference_loop(points, labels, False), 1, few, False)
    rec["host_entry_ms"], rec["host_entry_min_ms"] = median_ms(lambda: builder().add(points, labels), 1, few, False)
    if torch.cuda.is_available():
        dev = torch.device("cuda:0")
        pd, ld = torch.from_numpy(points).to(dev), torch.from_numpy(labels).to(dev)
        rec["device_resident_ms"], rec["device_resident_min_ms"] = median_ms(lambda: builder().add(pd, ld), args.warmup,
                                                                             args.iters, True)
        rec.update(status="measured", device_name=torch.cuda.get_device_name(0),
                   speedup_vs_reference_loop=rec["reference_loop_ms"] / rec["device_resident_ms"],
                   speedup_vs_masked_loop=rec["masked_loop_ms"] / rec["device_resident_ms"])
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
