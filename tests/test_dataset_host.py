"""Host checks of the frame assembly (csrc/frame.hip) and of ``WaymoDataset(device=None)``: the host twins against the
numpy restatements of tests/frame_ref.py, and the dataset against what the reference's own WaymoDataset returned on the
same directory (tests/golden/dataset.npz, tests/golden/make_golden_dataset.py).

Tolerances.  Transformed x, y, z of float64 files against the record: 8 * 2^-53 * (|x||m0| + |y||m1| + |z||m2| + |t|)
-- numpy's BLAS may fuse or reorder the three-term product, two evaluations differ by at most 2 * gamma_3, the final add
rounds once more in each; after the float32 cast the record is bit-equal (its generator asserts the conditioning).
Float32 files: 1 float32 ulp.  Column 4: the C library's tanh against numpy's in the rows' dtype, 2 ulp of 1.0 (tanh
lies in [0, 1), where an ulp of 1.0 is at least two ulps of the value: room for two libraries that are each good to 2 ulp).  Training frames:
x, y within test_augment_host.py's 2 float32 ulp of the planar magnitude.  Everything else is equal."""
import numpy as np
import pytest

import dataset_fixture as fx
import frame_ref
from aug_ref import check_rows

from openseg3d_amd import ops  # noqa: E402
from openseg3d_amd._lib import Seg3dError  # noqa: E402

G = fx.golden()
TANH_ULPS = 2


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("waymo"))
    fx.write(d, int(G["fixture_seed"]))
    return d


def matrix(i):
    return np.linalg.inv(fx.pose(0, 5)) @ fx.pose(0, i)


def raw_sweeps(dtype, counts, seed=0):
    rs = np.random.RandomState(seed)
    out = []
    for n in counts:
        a = rs.randn(n, 15) * ([20, 20, 2] + [1] * 12)
        a[:, 4] = 6 * rs.rand(n) ** 3
        out.append(a.astype(dtype))
    return out


def check_tanh(got, want, what=""):
    assert got.dtype == want.dtype
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / float(np.finfo(want.dtype).eps)
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: tanh column, worst {worst:.2f} ulp of 1.0 against numpy (bound {TANH_ULPS})")
    assert worst <= TANH_ULPS, what


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("stride", [6, 15])
def test_merge_twin_against_numpy(dtype, stride):
    raws = raw_sweeps(dtype, (611, 1, 0, 257))
    sweeps = [r[:, :6] if stride == 15 else np.ascontiguousarray(r[:, :6]) for r in raws]
    mats, lags = [None, matrix(4), matrix(3), matrix(1)], [0.0, 0.1000370000001567, 0.2, 0.4]
    out = ops.frame_assemble_host(ops.sweep_table(sweeps, mats, lags), want=("rows", "f32", "collated"), batch_id=3)
    want = frame_ref.merge_sweeps(raws, mats, lags, 6)
    rows = out["rows"]
    assert rows.dtype == dtype and rows.shape == want.shape == (869, 6)
    keep = [0, 1, 2, 3, 5]
    assert rows[:, keep].tobytes() == want[:, keep].tobytes()  # the stated recipe, bit for bit
    assert rows[:611, :3].tobytes() == raws[0][:, :3].tobytes()  # the current sweep is never multiplied
    check_tanh(rows[:, 4], want[:, 4], f"{np.dtype(dtype).name} stride {stride}")
    assert out["f32"].dtype == np.float32 and np.array_equal(out["f32"], rows.astype(np.float32))
    assert np.array_equal(out["collated"][:, 1:], out["f32"]) and (out["collated"][:, 0] == 3).all()
    # numpy's own matmul, as waymo_dataset.py:196-197 writes it (BLAS may fuse or reorder the product)
    row = 611
    for raw, m in zip(raws[1:], mats[1:]):
        lit = raw[:, :3].copy()
        lit[:, :3] = lit[:, :3] @ m[:3, :3].T
        lit[:, :3] += m[:3, 3]
        err = np.abs(rows[row:row + len(raw), :3].astype(np.float64) - lit.astype(np.float64))
        bound = frame_ref.transform_bound(raw[:, :3], m) if dtype == np.float64 else np.spacing(np.abs(lit)).astype(np.float64)
        assert (err <= bound).all()
        row += len(raw)


def test_merge_wide_rows_and_single_sweep():
    raws = raw_sweeps(np.float64, (300,), seed=3)
    out = ops.frame_assemble_host(ops.sweep_table(raws))["rows"]  # all 15 columns, as load_points returns them
    assert out.shape == (300, 15) and np.array_equal(out[:, 5:], raws[0][:, 5:]) and not out[:, 3].any()
    assert np.array_equal(out[:, :3], raws[0][:, :3])
    eight = raw_sweeps(np.float32, (5, 4, 3, 2, 1, 0, 7, 9), seed=4)
    mats = [None] + [matrix(i % 5) for i in range(7)]
    got = ops.frame_assemble_host(ops.sweep_table(eight, mats, list(range(8)), dim=7))["rows"]
    want = frame_ref.merge_sweeps(eight, mats, list(range(8)), 7)
    assert got[:, [0, 1, 2, 3, 5, 6]].tobytes() == want[:, [0, 1, 2, 3, 5, 6]].tobytes()


def test_error_paths():
    raws = raw_sweeps(np.float64, (3,) * 9)
    with pytest.raises(Seg3dError):
        ops.frame_assemble_host(ops.sweep_table(raws))  # 9 sweeps
    with pytest.raises(Seg3dError):
        ops.frame_assemble_host(ops.sweep_table([r[:, :4] for r in raws[:2]]))  # dim 4
    with pytest.raises(Seg3dError):
        ops.frame_assemble_host(ops.sweep_table([np.zeros((3, 17))]))  # dim 17
    with pytest.raises(Seg3dError):
        ops.frame_assemble_host(ops.sweep_table([raws[0].astype(np.int32)]))
    pred, ri = np.array([1, 2], np.int64), np.array([[5, 3, 0], [7, 1, 1]], np.int32)
    with pytest.raises(Seg3dError):
        ops.range_image_labels_host(pred, ri, 255)  # label + 1 would not fit the packing
    for bad in ([2650, 3, 0], [5, 64, 1], [-1, 3, 0], [5, -1, 1]):
        with pytest.raises(IndexError):
            ops.range_image_labels_host(pred, np.array([[5, 3, 0], bad], np.int32), 22)
    with pytest.raises(IndexError):
        ops.range_image_labels_host(np.array([1, 22], np.int64), ri, 22)  # a label outside [0, C)
    a, b = ops.range_image_labels_host(pred, np.array([[5, 3, 0], [2650, 64, -1]], np.int32), 22)  # skipped, not counted
    assert a[3, 5].tolist() == [0, 2] and a.sum() == 2 and not b.any()


@pytest.mark.parametrize("n", [0, 1, 1000])
@pytest.mark.parametrize("pred_dtype", [np.int64, np.uint8])
def test_range_images_twin_against_numpy(n, pred_dtype):
    pred, ri = range_image_case(n, pred_dtype)
    got = ops.range_image_labels_host(pred, ri, 22)
    want = frame_ref.range_images(pred, ri)
    assert got[0].dtype == np.int32 and got[0].shape == (64, 2650, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not got[0][:, :, 0].any() and not got[1][:, :, 0].any()
    if n == 1000:
        assert want[0].max() == 22 and want[1].max() == 22 and (want[0][:, :, 1] == 1).any()


def range_image_case(n, pred_dtype, seed=5):
    """n points on the real 64 x 2650 geometry; a quarter of them forced onto 8 shared pixels in both returns, a tenth
    without a return index, labels 0 and 21 present."""
    rs = np.random.RandomState(seed + n)
    pred = rs.randint(0, 22, n).astype(pred_dtype)
    ri = np.stack([rs.randint(0, 2650, n), rs.randint(0, 64, n), rs.randint(0, 2, n)], axis=1).astype(np.int32)
    if n >= 8:
        dup = rs.rand(n) < 0.25
        ri[dup, 0], ri[dup, 1] = 2649 - rs.randint(0, 4, dup.sum()), 63 * rs.randint(0, 2, dup.sum())
        ri[rs.rand(n) < 0.1] = -1
        pred[:4] = [0, 21, 0, 21]
        ri[:4] = [[0, 0, 0], [0, 0, 1], [2649, 63, 1], [2649, 63, 0]]
    return pred, ri


# ------------------------------------------------------------------------------------------ the dataset
def check_points(case, got, g, ds, what):
    want = g[case + "_points"]
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if want.dtype == np.float32:  # training: float32 after the transforms
        check_rows(got, want, 2, what)
        return
    c = 2 if ds.use_cylinder else 0  # cylinder rows: rho, phi, z, x, y, f..
    keep = [k for k in range(want.shape[1]) if k != 4 + c]
    n_cur = int(g[case + "_cur_point_count"])
    assert got[:n_cur, keep].tobytes() == want[:n_cur, keep].tobytes(), what  # the current sweep: bit for bit
    check_tanh(got[:, 4 + c], want[:, 4 + c], what)
    rest = [k for k in keep if k >= 3 + c]  # the lag and the copied columns of every sweep
    assert got[:, rest].tobytes() == want[:, rest].tobytes(), what
    assert np.array_equal(got.astype(np.float32), want.astype(np.float32)), what  # the record is well conditioned
    if got.shape[0] > n_cur:  # history sweeps against the double-precision bound
        name = fx.case_name(case)
        file_idx, frame_idx, _ = ds.parse_filename(name)
        row = n_cur
        for i in range(min(frame_idx, ds.cfg.DATASET.NUM_SWEEPS - 1)):
            sweep = ds.file_idx_to_name[(file_idx, frame_idx - 1 - i)]
            raw = ds._raw_points(sweep)
            m = np.linalg.inv(ds.load_pose(name)) @ ds.load_pose(sweep)
            err = np.abs(got[row:row + len(raw), :3] - want[row:row + len(raw), :3])
            bound = frame_ref.transform_bound(raw[:, :3], m)
            print(f"{what} sweep {i + 1}: {int((err > 0).sum())} of {err.size} coordinates differ, worst {err.max():.2e} "
                  f"(bound there {bound.flat[err.argmax()]:.2e})")
            assert (err <= bound).all(), what
            row += len(raw)
        assert row == got.shape[0]


@pytest.mark.parametrize("case", list(fx.CASES))
def test_dataset_against_reference(root, case):
    ds, index, init_draw = fx.make_dataset(case, root, G)
    seeded = fx.CASES[case][5] is not None
    if seeded:
        assert init_draw == float(G[case + "_next_draw_init"])  # the constructor consumed the reference's draws
    sample = ds[index]
    if seeded:
        assert fx.peek() == float(G[case + "_next_draw"])  # ... and so did __getitem__
    recorded = [k[len(case) + 1:] for k in G.files if k.startswith(case + "_") and
                not k.endswith(("_next_draw", "_next_draw_init", "_filenames"))]
    keys = {"val": ["filename", "cur_point_indices", "points", "point_image_features", "point_labels", "cur_point_count",
                    "voxel_coords", "point_voxel_ids", "voxel_labels"],
            "test": ["filename", "cur_point_indices", "points", "point_image_features", "points_ri", "cur_point_count",
                     "voxel_coords", "point_voxel_ids"]}["test" if case == "test_ms" else "val"]
    keys = [k for k in keys if k in recorded or k == "filename" or case == "test_ms"]
    assert list(sample.keys()) == keys, case
    assert sample["filename"] == fx.case_name(case)
    for k in recorded:
        got, want = np.asarray(sample[k]), G[f"{case}_{k}"]
        if k == "points":
            check_points(case, got, G, ds, case)
        else:
            assert got.dtype == want.dtype and np.array_equal(got, want), (case, k)
    if case == "test_ms":  # the same frame as val_ms5 through the same path
        check_points("val_ms5", sample["points"], G, ds, case)
        for k in ("voxel_coords", "point_voxel_ids", "cur_point_indices", "point_image_features"):
            assert np.array_equal(sample[k], G["val_ms5_" + k]), k
        assert (sample["points_ri"] == -1).any() and sample["points_ri"].dtype == np.int32


def test_collate_against_reference(root):
    samples = []
    for case in fx.COLLATE:
        ds, index, _ = fx.make_dataset(case, root, G)
        samples.append(ds[index])
    before = [s["point_voxel_ids"].copy() for s in samples]
    batch = ds.collate_batch(samples)
    for k in ("point_voxel_ids", "voxel_id_offset", "point_id_offset", "batch_size"):
        got, want = np.asarray(batch[k]), G["collate_" + k]
        assert got.dtype == want.dtype and np.array_equal(got, want), k
    for k in ("points", "voxel_coords", "point_labels", "voxel_labels", "point_image_features"):
        assert list(batch[k].shape) == G[f"collate_{k}_shape"].tolist() and str(batch[k].dtype) == str(G[f"collate_{k}_dtype"]), k
    n0 = samples[0]["points"].shape[0]
    assert (batch["points"][:n0, 0] == 0).all() and (batch["points"][n0:, 0] == 1).all()
    assert np.array_equal(batch["points"][:n0, 1:], samples[0]["points"])
    assert batch["filename"] == [fx.case_name(c) for c in fx.COLLATE]
    assert all(np.array_equal(a, s["point_voxel_ids"]) for a, s in zip(before, samples))


def test_public_members(root):
    ds, index, _ = fx.make_dataset("val_ms5", root, G)
    assert len(ds) == 7 and ds.dim_point == 6 and ds.use_multi_sweeps and not ds.use_cylinder and ds.num_classes == 22
    assert ds.ignore_index == 255 and ds.use_image_feature and ds.dim_image_feature == fx.DIM_IMAGE_FEATURE
    assert ds.grid_size.tolist() == [1440, 1440, 64] and ds.voxel_size.dtype == np.float32
    name = fx.case_name("val_ms5")
    assert ds.parse_filename(name) == ("segA0001", 5, np.int64(name.split("-")[1]))
    assert ds.load_pose(name).shape == (4, 4)
    pts = ds.load_points(name)
    assert pts.shape[1] == 15 and pts.dtype == np.float64 and not pts[:, 3].any()
    with pytest.raises(NotImplementedError):
        ds.load_points_from_sweeps(name, pad_empty_sweeps=True)
    labels = ds.load_label(name)
    assert labels.dtype == np.int32 and (labels == 255).any() and labels.max() == 255 and labels.min() >= 0
    test = fx.make_dataset("test_ms", root, G)[0]
    assert sorted(test.filenames) == sorted(fx.frame_name(f, i, dict((a, t) for a, _, t in fx.SEGMENTS)[f])
                                            for f, i in fx.TEST_FRAMES)
    with pytest.raises(Seg3dError):
        ds.assemble([])  # the device path belongs to device="cuda"


@pytest.mark.parametrize("case", ["val_ms5", "test_ms", "train_ms", "train_single"])
def test_load_raw_is_host_only_and_picklable(root, case):
    """The worker half of the device path runs without a GPU: raw arrays, matrices, lags, labels and the draws."""
    import pickle
    ds, index, _ = fx.make_dataset(case, root, G, device="cuda")
    raw = pickle.loads(pickle.dumps(ds[index]))
    assert ds.collate_raw([raw])[0] is raw
    mode, multi, _, image, _, seed = fx.CASES[case]
    name = fx.case_name(case)
    assert raw["filename"] == name and len(raw["sweeps"]) == (3 if multi else 1)
    assert all(s.shape[1] == 6 and s.dtype == np.float64 for s in raw["sweeps"])
    assert raw["matrices"][0] is None and raw["lags"][0] == 0.0
    assert np.array_equal(raw["sweeps"][0], np.load(f"{root}/lidar/{name}.npy")[:, :6])  # untouched: the device does the rest
    if multi:
        assert all(m.shape == (4, 4) for m in raw["matrices"][1:]) and all(0.09 < lag < 0.5 for lag in raw["lags"][1:])
        host, hindex, _ = fx.make_dataset(case, root, G)  # re-seeded: the same history choice
        merged = ops.frame_assemble_host(ops.sweep_table(raw["sweeps"], raw["matrices"], raw["lags"]))["rows"]
        if mode != "training":
            assert np.array_equal(merged, host[hindex]["points"])
    if mode == "testing":
        assert np.array_equal(raw["points_ri"], G["test_ms_points_ri"]) and "labels" not in raw
    else:
        assert raw["labels"].dtype == np.int32 and raw["labels"].min() == 0  # raw: the remap runs on the device
    if image:
        assert raw["image_rows"].dtype == np.int32 and raw["image_feats"].shape == (len(raw["image_rows"]), fx.DIM_IMAGE_FEATURE)
    if seed is not None:
        assert 0 <= raw["seed"] < 2 ** 32 and ("sweeps2" in raw) == (not multi)
    else:
        assert "seed" not in raw
