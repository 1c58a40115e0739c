#!/usr/bin/env python3
"""Generate tests/golden/augment.npz from the REFERENCE's own Python (build container only; see make_golden.py).

Runs the reference's PolarMix (polarmix.py) and its composed training transforms (transforms.py, transform_utils.py; the
list of waymo_dataset.py:44-50) from a seeded ``numpy.random`` on small float64 frames and records the inputs, every
number drawn and the output after each stage.  Three cases:

  swap_on   n1 = 1003, n2 = 701: PolarMix with the sector swap, then the transforms
  swap_off  the same frames, a seed whose first draw turns the swap off
  sweeps    n = 1501 with 611 current-sweep rows (cur_point_indices, labels and features sized to them), no PolarMix;
            its sample range leaves more far rows than PointSample keeps

The drawn numbers are recovered by replaying the reference's call order on a second RandomState of the same seed; the
script asserts that they reproduce the reference's outputs (so the record is the reference's, not ours), and that the
comparison is well conditioned: no yaw within 1e-9 rad of the sector bounds, no planar distance within 1e-3 of the
sample range, both distance sets non-empty.  Seeds are stepped until all of it holds.

Usage:  python tests/golden/make_golden_aug.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (reference loader)
from openseg3d_amd import scene  # noqa: E402

INSTANCE_CLASSES = [3, 0, 7, 12, 5, 1]  # not ascending: the block is class-major in LIST order
ROT_RANGE = [-0.78539816, 0.78539816]
SCALE_RANGE = [0.95, 1.05]
TRANSLATE_STD = 0.5
DIM, FEAT = 6, 4


def load():
    for pkg in ("seg3d", "seg3d.datasets", "seg3d.datasets.transforms"):
        if pkg not in sys.modules:
            mg._shell(pkg)
    tu = mg._load("seg3d.datasets.transforms.transform_utils", "seg3d/datasets/transforms/transform_utils.py")
    sys.modules["seg3d.datasets.transforms"].transform_utils = tu
    tr = mg._load("seg3d.datasets.transforms.transforms", "seg3d/datasets/transforms/transforms.py")
    pm = mg._load("seg3d.datasets.transforms.polarmix", "seg3d/datasets/transforms/polarmix.py")
    return tu, tr, pm


def frame(seed, n):
    pts = scene.make_small_scene(seed, n, extent=12.0, dtype=np.float64)
    rs = np.random.RandomState(700 + seed)
    labels = rs.randint(0, 22, n).astype(np.uint8)
    labels[rs.rand(n) < 0.15] = 255
    feats = rs.randn(n, FEAT).astype(np.float32)
    feats[rs.rand(n) < 0.4] = 0
    return pts, labels, feats


class Reject(Exception):
    pass


def run_case(tr, pm, seed, want_swap, sample_ratio, sample_range, want_far_over, multi):
    out = {"seed": np.array(seed), "sample_ratio": np.array(sample_ratio), "sample_range": np.array(sample_range)}
    if multi:
        p1, _, _ = frame(31, 1501)
        n_cur = 611
        _, l1, f1 = frame(32, n_cur)
        out.update(points1=p1, labels1=l1, feats1=f1, cur_point_indices=np.arange(n_cur))
    else:
        p1, l1, f1 = frame(11, 1003)
        p2, l2, f2 = frame(12, 701)
        out.update(points1=p1, labels1=l1, feats1=f1, points2=p2, labels2=l2, feats2=f2)

    np.random.seed(seed)
    replay = np.random.RandomState(seed)
    if multi:
        points, labels, feats = p1.copy(), l1.copy(), f1.copy()
    else:
        angles = [0.7, 2.9]
        mix = pm.PolarMix(instance_classes=INSTANCE_CLASSES, rot_angle_range=angles)
        points, feats, labels = mix(p1.copy(), f1.copy(), l1.copy(), p2.copy(), f2.copy(), l2.copy())
        assert points.dtype == np.float64  # columns 3.. are copies of the inputs' (polarmix.py:54): only xyz is recorded
        swap = replay.random() < 0.5
        alpha = (replay.random() - 1) * np.pi if swap else 0.0
        beta = alpha + np.pi if swap else 0.0
        replay.random()
        if swap != want_swap:
            raise Reject("swap")
        if swap:
            for p in (p1, p2):
                yaw = -np.arctan2(p[:, 1], p[:, 0])
                if min(np.abs(yaw - alpha).min(), np.abs(yaw - beta).min()) < 1e-9:
                    raise Reject("yaw on a sector bound")
        out.update(swap=np.array(swap), alpha=np.array(alpha), beta=np.array(beta), paste_angles=np.array(angles),
                   instance_classes=np.array(INSTANCE_CLASSES), pm_xyz=points[:, :3].copy(), pm_labels=labels, pm_feats=feats)

    d = {"points": points.copy(), "point_labels": labels.copy(), "point_image_features": feats.copy()}
    if multi:
        d["cur_point_indices"] = out["cur_point_indices"].copy()
    stages = [("rot", tr.RandomGlobalRotation(ROT_RANGE)), ("scale", tr.RandomGlobalScaling(SCALE_RANGE)),
              ("translate", tr.RandomGlobalTranslation(TRANSLATE_STD)), ("flip", tr.RandomFlip()),
              ("shuffle", tr.PointShuffle()), ("sample", tr.PointSample(sample_ratio, sample_range))]
    for name, t in stages:
        d = t(d)
        assert d["points"].dtype == np.float32
        if name not in ("shuffle", "sample"):  # those two only reorder rows: perm / choices and out_points cover them
            out["xyz_" + name] = d["points"][:, :3].copy()
        if name == "flip":
            before_shuffle = d["points"].copy()
        if name == "shuffle":
            shuffled = d["points"].copy()
            out["shuffle_labels"] = d["point_labels"].copy()
            if multi:
                out["shuffle_cur"] = np.asarray(d["cur_point_indices"]).copy()

    # the draws, replayed in the reference's call order
    rot = replay.uniform(ROT_RANGE[0], ROT_RANGE[1])
    scale = replay.uniform(SCALE_RANGE[0], SCALE_RANGE[1])
    offsets = [replay.normal(0, TRANSLATE_STD, 1)[0] for _ in range(3)]
    flips = [bool(replay.choice([False, True], replace=False, p=[0.5, 0.5])) for _ in range(2)]
    n = before_shuffle.shape[0]
    perm = np.array(range(n))
    replay.shuffle(perm)
    assert np.array_equal(before_shuffle[perm], shuffled)
    dist = np.linalg.norm(shuffled[:, :2], axis=1)
    if np.abs(dist - sample_range).min() < 1e-3:
        raise Reject("distance on the sample range")
    far, near = np.where(dist >= sample_range)[0], np.where(dist < sample_range)[0]
    num = min(int(n * sample_ratio), n)
    if len(far) == 0 or len(near) == 0 or (len(far) > num) != want_far_over:
        raise Reject("far / near sets")
    if len(far) > num:
        far = replay.choice(far, num, replace=False)
    choices = np.concatenate((far, replay.choice(near, num - len(far), replace=False)))
    replay.shuffle(choices)
    assert np.array_equal(shuffled[choices], d["points"])
    next_draw = np.random.random()
    assert next_draw == replay.random()  # both generators consumed the same numbers

    out.update(rot=np.array(rot), scale=np.array(scale), offsets=np.array(offsets), flips=np.array(flips), perm=perm,
               choices=choices, n_far=np.array(int((dist >= sample_range).sum())), next_draw=np.array(next_draw),
               out_points=d["points"], out_labels=d["point_labels"], out_feats=d["point_image_features"])
    if multi:
        out["out_cur"] = np.asarray(d["cur_point_indices"])
    return out


def main():
    _, tr, pm = load()
    arrays = {}
    cases = (("swap_on", True, 0.95, 9.0, False, False), ("swap_off", False, 0.95, 9.0, False, False),
             ("sweeps", None, 0.6, 4.0, True, True))
    for name, want_swap, ratio, rng, far_over, multi in cases:
        for seed in range(100, 400):
            try:
                case = run_case(tr, pm, seed, want_swap, ratio, rng, far_over, multi)
                break
            except Reject as e:
                print(f"{name}: seed {seed} rejected ({e})")
        else:
            raise SystemExit(f"{name}: no seed fits")
        for k, v in case.items():
            arrays[f"{name}_{k}"] = v
    mg.save("augment.npz", **arrays)


if __name__ == "__main__":
    main()
