"""A tiny dataset in the reference's directory layout (seg3d/datasets/waymo_dataset.py:101-154, 204-211), written from
seeds into a directory the caller names.  Nothing of it is committed.

  lidar/<name>.npy          float64 [N, 15]: x, y, z, range, intensity, elongation, 6 camera-projection columns, then
                            (col, row, return index) of the range image; some rows (-1, -1, -1)
  label/<name>.npy          int32 [N, 2]: (instance id, semantic label with 0 = unlabelled); one frame has none
  pose/<name>.txt           4 x 4 sensor-to-local matrix (np.savetxt)
  image_feature/<name>.npy  pickled dict row -> float32 [DIM_IMAGE_FEATURE], about half the rows
  3d_semseg_test_set_frames.txt, instances/lidar_instances_with_height.pkl

Two segments of 6 and 2 frames, names <file_idx>-<timestamp>-<frame_idx>."""
import os
import pickle

import numpy as np

import instaug_ref as ir

SEGMENTS = (("segA0001", 6, 1550083467346370), ("segB0002", 2, 1550090000123456))
UNLABELLED = ("segA0001", 2)
TEST_FRAMES = (("segA0001", 2), ("segA0001", 5), ("segB0002", 0))
BANK_SEED = 7
DIM_IMAGE_FEATURE = 8  # a config value (DATASET.DIM_IMAGE_FEATURE); 8 keeps the record small
RI_ROWS, RI_COLS = 64, 2650


def frame_name(file_idx, frame_idx, t0):
    return f"{file_idx}-{t0 + 100000 * frame_idx + 37 * frame_idx}-{frame_idx}"


def all_names():
    return [frame_name(f, i, t0) for f, n, t0 in SEGMENTS for i in range(n)]


def pose(seg, i):
    yaw = 0.02 * (i + 1) + 0.3 * seg
    c, s = np.cos(yaw), np.sin(yaw)
    m = np.eye(4)
    m[:3, :3] = [[c, -s, 0.001 * i], [s, c, -0.002], [-0.001 * i * c - 0.002 * s, 0.002 * c - 0.001 * i * s, 1.0]]
    m[:3, 3] = [35.0 + 1.7 * i + 50 * seg, -62.0 + 0.9 * i * i, 3.0 + 0.05 * i]
    return m


def write(root, seed=0, lidar_dtype=np.float64):
    """Write the dataset under ``root``; returns the frame names in (segment, frame) order."""
    for d in ("lidar", "label", "pose", "image_feature", "instances"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    names = []
    k = 0
    for seg, (file_idx, n_frames, t0) in enumerate(SEGMENTS):
        for i in range(n_frames):
            name = frame_name(file_idx, i, t0)
            names.append(name)
            rs = np.random.RandomState(1000 * seed + 10 * k + 1)
            pts, labels = ir.make_scene(100 * seed + k, n_ground=380 + 100 * k, n_clusters=12 + 2 * k, n_ignored=40 + 5 * k)
            n = len(pts)
            lidar = np.zeros((n, 15))
            lidar[:, :3] = pts[:, :3]
            lidar[:, 3] = np.linalg.norm(pts[:, :3], axis=1)
            lidar[:, 4] = 6.0 * rs.rand(n) ** 3
            lidar[:, 5] = rs.rand(n)
            lidar[:, 6:12] = rs.randint(0, 1900, (n, 6))
            ri = np.stack([rs.randint(0, RI_COLS, n), rs.randint(0, RI_ROWS, n), rs.randint(0, 2, n)], axis=1)
            ri[rs.rand(n) < 0.1] = -1
            lidar[:, 12:] = ri
            np.save(os.path.join(root, "lidar", name + ".npy"), lidar.astype(lidar_dtype))
            if (file_idx, i) != UNLABELLED:
                sem = np.where(labels == 255, 0, labels.astype(np.int32) + 1).astype(np.int32)
                np.save(os.path.join(root, "label", name + ".npy"),
                        np.stack([rs.randint(0, 50, n).astype(np.int32), sem], axis=1))
            np.savetxt(os.path.join(root, "pose", name + ".txt"), pose(seg, i))
            rows = np.sort(rs.choice(n, n // 2, replace=False))
            feats = rs.randn(len(rows), DIM_IMAGE_FEATURE).astype(np.float32)
            np.save(os.path.join(root, "image_feature", name + ".npy"), {int(r): feats[j] for j, r in enumerate(rows)},
                    allow_pickle=True)
            k += 1
    with open(os.path.join(root, "3d_semseg_test_set_frames.txt"), "w") as fp:
        for file_idx, i in TEST_FRAMES:
            t0 = dict((f, t) for f, _, t in SEGMENTS)[file_idx]
            fp.write(f"{file_idx},{t0 + 100000 * i + 37 * i}\n")
    with open(os.path.join(root, "instances", "lidar_instances_with_height.pkl"), "wb") as fp:
        pickle.dump(ir.make_bank(BANK_SEED), fp)
    return names


# name -> (mode, multi-sweep, cylinder, image features, (file_idx, frame_idx), numpy seed or None)
CASES = {
    "val_ms0": ("validation", True, False, True, ("segA0001", 0), None),    # no history
    "val_ms1": ("validation", True, False, True, ("segA0001", 1), None),    # one history sweep
    "val_ms5": ("validation", True, False, True, ("segA0001", 5), None),    # more history than NUM_SWEEPS - 1
    "val_cyl": ("validation", False, True, False, ("segA0001", 3), None),
    "test_ms": ("testing", True, False, True, ("segA0001", 5), None),
    "train_ms": ("training", True, False, True, ("segA0001", 5), 1234),     # the history choice is drawn
    "train_single": ("training", False, False, False, ("segA0001", 4), 4321),  # instance bank, PolarMix
}
COLLATE = ("val_ms1", "val_ms5")
CYL_RANGE = [0, -3.1415926, -2, 75.2, 3.1415926, 5.2]
CYL_VOXEL = [0.05, 0.012, 0.1]


def make_cfg(multi, cylinder, image):
    from openseg3d_amd import config
    cfg = config.default_cfg()
    d = cfg.DATASET
    d.USE_MULTI_SWEEPS, d.USE_CYLINDER, d.USE_IMAGE_FEATURE = multi, cylinder, image
    d.DIM_IMAGE_FEATURE = DIM_IMAGE_FEATURE
    if cylinder:
        d.POINT_CLOUD_RANGE, d.VOXEL_SIZE = list(CYL_RANGE), list(CYL_VOXEL)
    return cfg


def case_name(case):
    file_idx, i = CASES[case][4]
    return frame_name(file_idx, i, dict((f, t) for f, _, t in SEGMENTS)[file_idx])


def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset.npz")
    return np.load(path)


def peek():
    """The next numpy.random.random() without consuming it."""
    state = np.random.get_state()
    value = np.random.random()
    np.random.set_state(state)
    return value


def make_dataset(case, root, g, **kw):
    """The dataset of a recorded case, numpy.random seeded as the record was; ``filenames`` takes the recorded order (glob
    order belongs to the file system that made the record, and the single-sweep training case indexes it randomly)."""
    from openseg3d_amd.dataset import WaymoDataset
    mode, multi, cyl, image, _, seed = CASES[case]
    if seed is not None:
        np.random.seed(seed)
    ds = WaymoDataset(make_cfg(multi, cyl, image), root, mode, **kw)
    init_draw = peek()
    assert sorted(ds.filenames) == sorted(str(x) for x in g[case + "_filenames"])
    ds.filenames = [str(x) for x in g[case + "_filenames"]]
    return ds, ds.filenames.index(case_name(case)), init_draw
