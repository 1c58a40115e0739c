#!/usr/bin/env python3
"""Generate tests/golden/tta_views.npz from the REFERENCE's own Python (build container only; see make_golden.py).

Records, on a ~1 k-point cartesian scene (make_small_scene, rows [x, y, z, 0, tanh(i), elongation]):
  * the 36 views of the reference's MultiScaleFlipAug (test_time_aug.py:15-35) with tools/eval.py's arguments
    (scales [0.95, 1.0, 1.05], angles [-pi/4, 0, pi/4], flip_x, flip_y): the view coordinates, and what the reference's
    WaymoDataset.prepare_data / collate_batch made of each (voxel_coords, point_voxel_ids);
  * rotate_points_along_z (transform_utils.py:11-32) of the frame by each angle, and its float32 cos / sin;
  * IOUMetric (iou_metric.py) on the reference's own __main__ case and on a 22-class case with absent classes and
    ignored (255) labels: confusion matrix and per-class IoU.  IOUMetric.add calls np.int, gone from numpy >= 1.24:
    np.int = int is patched in for the run.

Usage:  python tests/golden/make_golden_tta.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (reference loader; REF / ROOT / CART_* constants)
from openseg3d_amd import scene  # noqa: E402

SCALES = [0.95, 1.0, 1.05]
ANGLES = [-0.78539816, 0, 0.78539816]  # tools/eval.py:104-107


def load():
    ref = mg.load_reference()
    for pkg in ("seg3d.datasets", "seg3d.datasets.transforms", "seg3d.core.evaluation"):
        mg._shell(pkg)
    sys.modules["seg3d.core"].VoxelGenerator = ref.voxel.VoxelGenerator
    # waymo_dataset.py imports the training augmentations; validation-mode prepare_data never calls them
    for name, attr in (("transforms", None), ("instance_augmentation", "InstanceAugmentation"), ("polarmix", "PolarMix")):
        m = types.ModuleType("seg3d.datasets.transforms." + name)
        if attr:
            setattr(m, attr, object)
        sys.modules[m.__name__] = m
        setattr(sys.modules["seg3d.datasets.transforms"], name, m)
    ref.tu = mg._load("seg3d.datasets.transforms.transform_utils", "seg3d/datasets/transforms/transform_utils.py")
    ref.tta = mg._load("seg3d.datasets.transforms.test_time_aug", "seg3d/datasets/transforms/test_time_aug.py")
    ref.waymo = mg._load("seg3d.datasets.waymo_dataset", "seg3d/datasets/waymo_dataset.py")
    ref.iou = mg._load("seg3d.core.evaluation.iou_metric", "seg3d/core/evaluation/iou_metric.py")
    return ref


def validation_dataset(ref):
    """A WaymoDataset in validation mode without its file list (prepare_data reads cfg, mode, voxel_generator)."""
    cfg = types.SimpleNamespace(DATASET=types.SimpleNamespace(AUG_DATA=True, USE_MULTI_SWEEPS=False, USE_CYLINDER=False))
    ds = object.__new__(ref.waymo.WaymoDataset)
    ds.cfg, ds.mode = cfg, "validation"
    ds.voxel_generator = ref.voxel.VoxelGenerator(voxel_size=mg.CART_VOXEL, point_cloud_range=mg.CART_RANGE)
    return ds


def iou_case(ref, class_names, adds):
    np.int = int  # iou_metric.py:52-53
    try:
        m = ref.iou.IOUMetric(class_names)
        for p, g in adds:
            m.add(torch.from_numpy(p), torch.from_numpy(g))
        hist = sum(m.hist_list)
        return hist.astype(np.int64), m.per_class_iou(hist), m.get_metric()["mIOU"]
    finally:
        del np.int


def main():
    ref = load()
    ds = validation_dataset(ref)
    frame = scene.make_small_scene(77, 1000, extent=12.0)
    points = np.pad(frame, ((0, 0), (1, 0)), constant_values=0.0).astype(np.float32)  # collated, batch column 0
    aug = ref.tta.MultiScaleFlipAug(ds, scales=SCALES, angles=ANGLES, flip_x=True, flip_y=True)
    views = aug({"points": points, "point_image_features": np.zeros((points.shape[0], 0), np.float32)})
    assert len(views) == 36
    view_xyz = np.stack([v["points"][:, 1:4] for v in views]).astype(np.float32)
    assert all(np.array_equal(v["points"][:, 4:], points[:, 4:]) for v in views)
    coords = [v["voxel_coords"].astype(np.int32) for v in views]
    rot = np.stack([ref.tu.rotate_points_along_z(frame[np.newaxis], np.array([a]))[0][:, :3] for a in ANGLES])
    ang = torch.from_numpy(np.array(ANGLES)).float()
    cos_sin = torch.stack([torch.cos(ang), torch.sin(ang)], dim=1).numpy()

    rs = np.random.RandomState(3)
    p1, g1 = rs.randint(0, 22, 400), rs.randint(0, 22, 400)
    g1[g1 == 7] = 255  # class 7: never labelled ...
    p1[p1 == 7] = 8    # ... nor predicted -> empty union, NaN
    g1[rs.rand(400) < 0.1] = 255
    p2, g2 = rs.randint(0, 22, 300), rs.randint(0, 22, 300).astype(np.uint8)
    g2[g2 == 7] = 255
    p2[p2 == 7] = 9
    hist22, iou22, miou22 = iou_case(ref, [f"c{i}" for i in range(22)], [(p1, g1), (p2, g2)])
    main_case = [(np.array([1, 2, 3]), np.array([1, 1, 3])), (np.array([0, 2, 3]), np.array([1, 3, 3]))]
    hist4, iou4, miou4 = iou_case(ref, ["c0", "c1", "c2", "c3"], main_case)

    mg.save("tta_views.npz", points=points, scales=np.array(SCALES), angles=np.array(ANGLES), cos_sin=cos_sin,
            view_xyz=view_xyz, rot_xyz=rot.astype(np.float32),
            voxel_coords=np.concatenate(coords), voxel_offsets=np.cumsum([0] + [c.shape[0] for c in coords]),
            point_voxel_ids=np.stack([v["point_voxel_ids"] for v in views]).astype(np.int32),
            iou22_preds=np.concatenate([p1, p2]), iou22_labels=np.concatenate([g1, g2]), iou22_split=np.array([400]),
            iou22_hist=hist22, iou22_iou=iou22, iou22_miou=np.array(miou22),
            iou4_hist=hist4, iou4_iou=iou4, iou4_miou=np.array(miou4))


if __name__ == "__main__":
    main()
