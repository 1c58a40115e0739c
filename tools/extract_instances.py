#!/usr/bin/env python3
"""Build the instance bank of ``InstanceAugmentation`` from a training split: the reference's tools/extract_instances.py
for all labels in one pass, with the per-frame work in the library (csrc/instance_extract.hip).

    python tools/extract_instances.py --data_dir DIR --out lidar_instances.pkl [--device cuda|cpu]
                                      [--labels 3 4 10] [--min_points 120 30 30] [--eps 0.25]

Reads ``DIR/label/*.npy`` and the ``DIR/lidar/*.npy`` beside each, as the reference's load_points / load_label do
(``[:, :6]``; label column 1, minus one, 0 -> 255), and writes ONE pickle ``{label_id: [{'cluster_points',
'cluster_height'}, ...]}`` -- the dict ``InstanceAugmentation(instance_path)`` indexes, which the reference obtains by
running its script once per label and merging the lists by hand.  ``--device cpu`` uses the library's host entry (no
GPU needed); both give the same bank."""
import argparse
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd.augment import InstanceBankBuilder  # noqa: E402


def load_points(lidar_file):
    return np.ascontiguousarray(np.load(lidar_file)[:, :6])


def load_label(label_file):
    labels = np.load(label_file)[:, 1]
    labels -= 1
    labels[labels == -1] = 255
    return np.ascontiguousarray(labels.astype(np.uint8 if labels.dtype.kind in "iu" and labels.max(initial=0) < 256 else np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_dir", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", choices=["cuda", "cpu"], default="cuda")
    ap.add_argument("--labels", type=int, nargs="+", default=[3, 4, 10])  # other-vehicle, motorcyclist, cone
    ap.add_argument("--min_points", type=int, nargs="+", default=[120, 30, 30])
    ap.add_argument("--ground_labels", type=int, nargs="+", default=[17, 18, 19, 20, 21])
    ap.add_argument("--eps", type=float, default=0.25)
    args = ap.parse_args()
    if len(args.labels) != len(args.min_points):
        ap.error("one --min_points value per --labels value")
    builder = InstanceBankBuilder(args.labels, args.min_points, args.ground_labels, args.eps)
    label_files = sorted(glob.glob(os.path.join(args.data_dir, "label", "*.npy")))
    if args.device == "cuda":
        import torch
    for k, label_file in enumerate(label_files):
        lidar_file = os.path.join(args.data_dir, "lidar", os.path.basename(label_file))
        points, labels = load_points(lidar_file), load_label(label_file)
        if points.dtype not in (np.float32, np.float64):
            points = points.astype(np.float64)
        if args.device == "cuda":
            points, labels = torch.from_numpy(points).cuda(), torch.from_numpy(labels).cuda()
        added = builder.add(points, labels)
        if (k + 1) % 100 == 0 or k + 1 == len(label_files):
            print(f"{k + 1} / {len(label_files)} frames, +{added}, "
                  + ", ".join(f"label {t}: {len(v)}" for t, v in builder.instances.items()), flush=True)
    builder.save(args.out)
    print(f"{args.out}: {sum(len(v) for v in builder.instances.values())} instances from {builder.frames} frames")


if __name__ == "__main__":
    main()
