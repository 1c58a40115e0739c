#!/usr/bin/env python3
"""Generate tests/golden/dataset.npz from the REFERENCE's own WaymoDataset (build container only; see make_golden.py).

tests/dataset_fixture.py writes a tiny dataset in the reference's directory layout into a temporary directory; the
reference's class (seg3d/datasets/waymo_dataset.py, with its real transforms, PolarMix and InstanceAugmentation) is
loaded the way make_golden_tta.py loads it and ``__getitem__`` is recorded for the cases of dataset_fixture.CASES, plus
``collate_batch`` of two validation samples.  For the seeded training cases ``numpy.random`` is seeded BEFORE the
constructor (which draws PolarMix's two angles); the next ``random()`` after the constructor and after ``__getitem__``
is recorded without consuming it, so a test can compare generator states.  ``filenames`` (glob order: a property of the
file system) is recorded for the training case that indexes it with a random number.

The record must be well conditioned: no transformed coordinate of a history sweep lies within the double-precision
bound 8 * 2^-53 * (|x||m0| + |y||m1| + |z||m2| + |t|) of a float32 rounding boundary, so after the float32 cast the
fixture is bit-equal however the three-term product is evaluated; likewise no tanh of an intensity lies within 16 of its
own ulp of such a boundary.  The fixture seed is stepped until both hold.

Usage:  python tests/golden/make_golden_dataset.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (reference loader)
import dataset_fixture as fx  # noqa: E402
import frame_ref  # noqa: E402


def load():
    ref = mg.load_reference()
    for pkg in ("seg3d.datasets", "seg3d.datasets.transforms"):
        mg._shell(pkg)
    sys.modules["seg3d.core"].VoxelGenerator = ref.voxel.VoxelGenerator
    tu = mg._load("seg3d.datasets.transforms.transform_utils", "seg3d/datasets/transforms/transform_utils.py")
    sys.modules["seg3d.datasets.transforms"].transform_utils = tu
    mg._load("seg3d.datasets.transforms.transforms", "seg3d/datasets/transforms/transforms.py")
    mg._load("seg3d.datasets.transforms.polarmix", "seg3d/datasets/transforms/polarmix.py")
    mg._load("seg3d.datasets.transforms.instance_augmentation", "seg3d/datasets/transforms/instance_augmentation.py")
    return mg._load("seg3d.datasets.waymo_dataset", "seg3d/datasets/waymo_dataset.py")


def peek():
    st = np.random.get_state()
    v = np.random.random()
    np.random.set_state(st)
    return v


class Reject(Exception):
    pass


def check_conditioning(ds, name, points, n_cur, n_sweeps):
    """The history sweeps the validation path merges: the recorded float64 coordinates lie within the bound of the
    stated recipe.  Every history sweep a training draw may pick: no coordinate within the bound of a float32 rounding
    boundary."""
    file_idx, frame_idx, _ = ds.parse_filename(name)
    t_cur = ds.load_pose(name)
    row = n_cur
    for i in range(min(frame_idx, ds.cfg.DATASET.MAX_NUM_SWEEPS - 1)):
        sweep = ds.file_idx_to_name[(file_idx, frame_idx - 1 - i)]
        raw = np.load(os.path.join(ds.data_root, "lidar", sweep + ".npy"))
        m = np.linalg.inv(t_cur) @ ds.load_pose(sweep)
        ours = frame_ref.merge_sweeps([raw], [m], [0.0], 6)
        bound = frame_ref.transform_bound(raw[:, :3], m)
        xyz = ours[:, :3]
        if (xyz - bound).astype(np.float32).tobytes() != (xyz + bound).astype(np.float32).tobytes():
            raise Reject(f"{name}: a coordinate of sweep {sweep} within the bound of a float32 rounding boundary")
        if i < n_sweeps - 1:
            assert (np.abs(xyz - points[row:row + len(raw), :3]) <= bound).all(), "the recipe is outside its own bound"
            row += len(raw)
    assert row == len(points)


TANH_ULPS = 16  # in ulp of the value: any tanh library worth the name is far inside


def check_tanh(root):
    """No intensity's tanh within TANH_ULPS ulp of a float32 rounding boundary: the float32 cast of column 4 is the same for
    numpy's, the C library's and the device's tanh."""
    for name in fx.all_names():
        t = np.tanh(np.load(os.path.join(root, "lidar", name + ".npy"))[:, 4])
        slack = TANH_ULPS * np.spacing(t)
        if (t - slack).astype(np.float32).tobytes() != (t + slack).astype(np.float32).tobytes():
            raise Reject(f"{name}: a tanh within 16 ulp of a float32 rounding boundary")


def record(waymo, root):
    check_tanh(root)
    arrays = {}
    samples = {}
    for case, (mode, multi, cyl, image, _, seed) in fx.CASES.items():
        cfg = fx.make_cfg(multi, cyl, image)
        if seed is not None:
            np.random.seed(seed)
        ds = waymo.WaymoDataset(cfg, root, mode=mode)
        arrays[case + "_next_draw_init"] = np.array(peek())
        name = fx.case_name(case)
        sample = ds[ds.filenames.index(name)]
        arrays[case + "_next_draw"] = np.array(peek())
        arrays[case + "_filenames"] = np.array(ds.filenames)
        assert sample["filename"] == name
        if case.startswith("val_ms"):
            assert sample["points"].dtype == np.float64
            check_conditioning(ds, name, sample["points"], sample["cur_point_count"], cfg.DATASET.NUM_SWEEPS)
        samples[case] = sample
        for k, v in sample.items():
            if k == "filename" or (case == "test_ms" and k in ("points", "point_image_features", "voxel_coords",
                                                               "point_voxel_ids", "cur_point_indices")):
                continue  # test_ms: the same frame and path as val_ms5, asserted below
            arrays[f"{case}_{k}"] = np.asarray(v)
        print(case, {k: (np.asarray(v).dtype, np.asarray(v).shape) for k, v in sample.items() if k != "filename"})
    for k in ("points", "point_image_features", "voxel_coords", "point_voxel_ids", "cur_point_indices"):
        assert np.array_equal(samples["test_ms"][k], samples["val_ms5"][k])
    batch = waymo.WaymoDataset.collate_batch([{k: np.copy(v) for k, v in samples[c].items()} for c in fx.COLLATE])
    for k in ("point_voxel_ids", "voxel_id_offset", "point_id_offset", "batch_size"):
        arrays["collate_" + k] = np.asarray(batch[k])
    for k in ("points", "voxel_coords", "point_labels", "voxel_labels", "point_image_features"):
        arrays[f"collate_{k}_shape"] = np.array(batch[k].shape)
        arrays[f"collate_{k}_dtype"] = np.array(str(batch[k].dtype))
    assert batch["filename"] == [fx.case_name(c) for c in fx.COLLATE]
    return arrays


def main():
    waymo = load()
    for seed in range(0, 50):
        with tempfile.TemporaryDirectory() as root:
            fx.write(root, seed)
            try:
                arrays = record(waymo, root)
            except Reject as e:
                print(f"fixture seed {seed} rejected ({e})")
                continue
        arrays["fixture_seed"] = np.array(seed)
        mg.save("dataset.npz", **arrays)
        return
    raise SystemExit("no fixture seed fits")


if __name__ == "__main__":
    main()
