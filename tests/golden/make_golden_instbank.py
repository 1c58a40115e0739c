#!/usr/bin/env python3
"""Generate tests/golden/instbank.npz (build container only; see make_golden.py): what sklearn and the REFERENCE's own
``tools/extract_instances.py`` give on the fixture clouds of tests/instbank_ref.py (``make_cases``).

Per cloud and target label with at least ``min_points`` rows, as the script calls it (:52-57):

  <case>_<label>_ids      ``DBSCAN(eps=0.25, min_samples=min_points).fit(target_points[:, :2]).labels_``  (int16)
  <case>_<label>_center   ``np.mean(cluster_points[:, :3], axis=0)`` per cluster (:66)
  <case>_<label>_radius   the reference's ``get_instance_radius`` (:26-33, imported from the reference tree) per cluster (:67)

and per cloud ``<case>_check`` = (rows, sum of row index * coordinates) so that a test notices a fixture that has drifted
from the record.  The script asserts that the numpy restatement reproduces sklearn on every cloud, on float64 and on
float32 input: the clouds are on the 1/64 lattice, so every squared distance is exact in both.  Data only.

Usage:  python tests/golden/make_golden_instbank.py
"""
import os
import sys

import numpy as np
from sklearn.cluster import DBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (reference loader)
import instbank_ref as ir  # noqa: E402


def checksum(points):
    return np.array([len(points), float((points * np.arange(1, len(points) + 1)[:, None]).sum())])


def main():
    ref = mg._load("extract_instances", "tools/extract_instances.py")  # its work is under __main__: importing runs nothing
    arrays = {}
    for name, case in ir.make_cases().items():
        points, labels = case["points"], case["labels"]
        arrays[f"{name}_check"] = checksum(points)
        for target, min_points in zip(case["target_ids"], case["min_points"]):
            target_points = points[labels == target]
            if target_points.shape[0] < min_points:
                continue
            ids = DBSCAN(eps=case["eps"], min_samples=min_points).fit(target_points[:, :2]).labels_
            ids32 = DBSCAN(eps=case["eps"], min_samples=min_points).fit(target_points[:, :2].astype(np.float32)).labels_
            mine = ir.dbscan_ref(target_points[:, :2], case["eps"], min_points)
            assert np.array_equal(ids, mine) and np.array_equal(ids32, mine), (name, target)
            centers, radii = [], []
            for c in sorted(set(ids.tolist()) - {-1}):
                cluster_points = target_points[ids == c]
                centers.append(np.mean(cluster_points[:, :3], axis=0))
                radii.append(ref.get_instance_radius(cluster_points[:, :3], centers[-1]))
            arrays[f"{name}_{target}_ids"] = ids.astype(np.int16)
            arrays[f"{name}_{target}_center"] = np.array(centers).reshape(-1, 3)
            arrays[f"{name}_{target}_radius"] = np.array(radii)
            print(f"{name} label {target}: {len(ids)} rows, {len(radii)} clusters, {(ids < 0).sum()} noise")
    mg.save("instbank.npz", **arrays)


if __name__ == "__main__":
    main()
