#!/usr/bin/env python3
"""Generate tests/golden/instaug.npz from the REFERENCE's own InstanceAugmentation (build container only; see
make_golden.py).

The reference class (seg3d/datasets/transforms/instance_augmentation.py) is imported unchanged, its ``.instances`` is
set to a synthetic bank (labels 3, 4, 10 x 4 clusters: the bank is only a dict of arrays, tools/extract_instances.py:65-76)
and it runs under ``np.random.seed`` on a synthetic 1 500-row float64 scene (tests/instaug_ref.py: make_scene, make_bank).
The draws are recovered by replaying the reference's call order on a second RandomState of the same seed; the script
asserts that a numpy restatement fed with the replayed draws reproduces the reference's output (so the record is the
reference's, not ours).  Three cases, seeds stepped until each shows what it is for:

  feats   image features given; an instance accepted at a candidate index > 0 and an ACCEPTED instance with flip_type 3
  plain   image features None; an instance that fails all 20 candidates
  ground  image features given; an evaluated candidate that is free of occlusion but off the ground

and until every case is well conditioned: over all evaluated candidates the nearest object distance is more than
1e-6 * radius away from radius, the nearest ground distance more than 1e-6 * radius away from 1.2 * radius, the two
smallest ground distances of an accepted candidate more than 1e-9 m apart, and rounding the frame to float32 changes no
decision -- so no decision hangs on the last bit of a mean.

Usage:  python tests/golden/make_golden_instaug.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (reference loader)
import instaug_ref as ir  # noqa: E402

FEAT = 4
BANK_SEED = 7


class Reject(Exception):
    pass


def load():
    for pkg in ("seg3d", "seg3d.datasets", "seg3d.datasets.transforms"):
        if pkg not in sys.modules:
            mg._shell(pkg)
    return mg._load("seg3d.datasets.transforms.instance_augmentation",
                    "seg3d/datasets/transforms/instance_augmentation.py")


def run_case(ia, bank, name, seed):
    points, labels = ir.make_scene(seed)
    feats = None if name == "plain" else np.random.RandomState(seed).randn(len(points), FEAT).astype(np.float32)
    aug = ia.InstanceAugmentation("/nonexistent/bank.pkl")  # the path is only opened when it exists (:21)
    aug.instances = bank
    np.random.seed(seed)
    res = aug(points.copy(), None if feats is None else feats.copy(), labels.copy())
    out_points, out_labels = res[0], res[-1]
    # only the pasted rows are recorded: the frame's own rows, labels and features come back unchanged
    assert out_points.dtype == np.float64 and np.array_equal(out_points[:len(points)], points)
    assert np.array_equal(out_labels[:len(points)], labels)  # (numpy promotes the reference's uint8 labels to int64, :97)

    replay = np.random.RandomState(seed)
    items = ir.replay_draws(replay, bank)
    next_draw = np.random.random()
    assert next_draw == replay.random()  # both generators consumed the same numbers
    got_points, got_labels, decisions, info = ir.np_instance_paste(points, labels, bank, items)
    assert got_points.shape == out_points.shape and np.array_equal(got_labels, out_labels)
    assert np.abs(got_points - out_points).max() < 1e-12 and np.array_equal(got_points[:, 3:], out_points[:, 3:])
    if feats is not None:
        assert res[1].shape == (len(out_points), FEAT) and not res[1][len(points):].any()
        assert np.array_equal(res[1][:len(points)], feats)

    ground_only = 0
    for it, dec, rec in zip(items, decisions, info):
        r = rec["radius"]
        for ci in range(len(rec["obj"])):
            if abs(rec["obj"][ci] - r) <= 1e-6 * r or abs(rec["g0"][ci] - 1.2 * r) <= 1e-6 * r:
                raise Reject("a distance on a threshold")
            if rec["obj"][ci] > r and not rec["g0"][ci] < 1.2 * r:
                ground_only += 1
        if dec >= 0 and rec["g1"][dec] - rec["g0"][dec] <= 1e-9:
            raise Reject("two ground rows at the same distance")
    if ir.np_instance_paste(points.astype(np.float32), labels, bank, items)[2] != decisions:
        raise Reject("float32 rounding of the frame changes a decision")
    if name == "feats" and not (max(decisions) > 0 and any(it["flip_type"] == 3 and d >= 0
                                                           for it, d in zip(items, decisions))):
        raise Reject("no acceptance past candidate 0 or no accepted flip")
    if name == "plain" and -1 not in decisions:
        raise Reject("no failed instance")
    if name == "ground" and not (ground_only > 0 and max(decisions) >= 0):
        raise Reject("no candidate rejected for the ground test alone")
    print(f"{name}: seed {seed}, decisions {decisions}, flips {[it['flip_type'] for it in items]}, "
          f"{ground_only} candidates off the ground only, {len(out_points) - len(points)} rows pasted")
    out = {"seed": np.array(seed), "points": points, "labels": labels, "add_points": out_points[len(points):],
           "add_labels": out_labels[len(points):],
           "decisions": np.array(decisions, np.int32), "next_draw": np.array(next_draw),
           "draw_label": np.array([it["label"] for it in items]), "draw_index": np.array([it["index"] for it in items]),
           "draw_loc": np.array([it["loc_noise"] for it in items]), "draw_rot": np.array([it["rot_noise"] for it in items]),
           "draw_flip": np.array([it["flip_type"] for it in items]), "draw_angles": np.array([it["angles"] for it in items])}
    if feats is not None:
        out.update(feats=feats)
    return out


def main():
    ia = load()
    bank = ir.make_bank(BANK_SEED)
    arrays = {}
    clusters = [(lab, inst) for lab in sorted(bank) for inst in bank[lab]]
    arrays["bank_rows"] = np.concatenate([inst["cluster_points"] for _, inst in clusters])
    arrays["bank_offsets"] = np.cumsum([0] + [len(inst["cluster_points"]) for _, inst in clusters])
    arrays["bank_heights"] = np.array([inst["cluster_height"] for _, inst in clusters])
    arrays["bank_labels"] = np.array([lab for lab, _ in clusters])
    first = 100
    for name in ir.CASES:
        for seed in range(first, 400):
            try:
                case = run_case(ia, bank, name, seed)
                break
            except Reject as e:
                print(f"{name}: seed {seed} rejected ({e})")
        else:
            raise SystemExit(f"{name}: no seed fits")
        first = seed + 1
        for k, v in case.items():
            arrays[f"{name}_{k}"] = v
    mg.save("instaug.npz", **arrays)


if __name__ == "__main__":
    main()
