"""CPU checks of multi-sweep evaluation: the list form of ``MultiScaleFlipAug`` on a multi-sweep ``WaymoDataset(device=None)``
(the reference raises KeyError there: its views carry no ``cur_point_indices``), and the host side of the sweep cache
(``load_raw`` names its history sweeps instead of reading them; the constructor's argument checks)."""
import pickle

import numpy as np
import pytest

import dataset_fixture as fx

from openseg3d_amd import ops  # noqa: E402
from openseg3d_amd.dataset import WaymoDataset  # noqa: E402
from openseg3d_amd.evaluation import MultiScaleFlipAug  # noqa: E402

G = fx.golden()
SCALES, ANGLES = [0.95, 1.0, 1.05], [-0.78539816, 0, 0.78539816]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("waymo"))
    fx.write(d, int(G["fixture_seed"]))
    return d


@pytest.mark.parametrize("case", ["val_ms0", "val_ms5"])
def test_list_form_on_multi_sweep_dataset(root, case):
    ds, index, _ = fx.make_dataset(case, root, G)
    sample = ds[index]
    data = ds.collate_batch([sample])
    n, n_cur = data["points"].shape[0], int(sample["cur_point_count"])
    assert (n > n_cur) == (case != "val_ms0") and data["point_id_offset"].tolist() == [n_cur]
    aug = MultiScaleFlipAug(ds, scales=SCALES, angles=ANGLES, flip_x=True, flip_y=True)
    views = aug(data)
    assert len(views) == aug.n_views == 36
    frame = np.ascontiguousarray(data["points"][:, 1:], dtype=np.float32)
    want = ops.tta_views_host(frame, aug.table())
    for v, d in enumerate(views):
        assert d["batch_size"] == 1 and d["point_id_offset"].tolist() == [n_cur]
        assert d["points"].dtype == np.float32 and d["points"].shape == (n, 1 + ds.dim_point)
        assert not d["points"][:, 0].any() and np.array_equal(d["points"][:, 1:], want[v * n:(v + 1) * n, 1:])
        # lag, intensity, elongation pass through; the lag column still marks the current rows, which come first
        assert np.array_equal(d["points"][:, 4:], frame[:, 3:])
        assert np.array_equal(np.flatnonzero(d["points"][:, 4] == 0), np.arange(n_cur))
        coords, ids = ops.voxelize_host(np.ascontiguousarray(want[v * n:(v + 1) * n, 1:]), ds.voxel_size.tolist(),
                                        ds.point_cloud_range.tolist())
        assert np.array_equal(d["point_voxel_ids"], ids) and np.array_equal(d["voxel_coords"][:, 1:], coords[:, 1:])
        assert not d["voxel_coords"][:, 0].any() and d["voxel_id_offset"].tolist() == [coords.shape[0]]
        assert np.array_equal(d["point_image_features"], data["point_image_features"])
        assert d["point_image_features"].shape[0] == n_cur
    # the identity view (scale 1, angle 0, no flip) is the frame itself
    assert np.array_equal(views[1 * 12 + 1 * 4 + 3]["points"][:, 1:], frame)


def _cached(case, root, **kw):
    """``WaymoDataset(device="cuda")``: neither the constructor nor ``load_raw`` touches the device."""
    mode, multi, cyl, image, _, _ = fx.CASES[case]
    return WaymoDataset(fx.make_cfg(multi, cyl, image), root, mode, device="cuda", **kw)


@pytest.mark.parametrize("case", ["val_ms0", "val_ms1", "val_ms5", "test_ms"])
def test_load_raw_with_sweep_cache_names_its_history(root, case):
    plain, cached = _cached(case, root), _cached(case, root, sweep_cache=5)
    index = plain.filenames.index(fx.case_name(case))
    assert cached.filenames == plain.filenames
    want, got = plain.load_raw(index), cached.load_raw(index)
    n_sweeps = len(want["sweeps"])
    assert n_sweeps == {"val_ms0": 1, "val_ms1": 2}.get(case, 3)
    assert len(got["sweeps"]) == n_sweeps and all(s is None for s in got["sweeps"][1:])
    assert np.array_equal(got["sweeps"][0], want["sweeps"][0])
    file_idx, frame_idx = fx.CASES[case][4]
    t0 = dict((f, t) for f, _, t in fx.SEGMENTS)[file_idx]
    assert got["sweep_names"] == [fx.frame_name(file_idx, frame_idx - s, t0) for s in range(n_sweeps)]
    assert got["lags"] == want["lags"] and got["lags"][0] == 0.0 and all(lag > 0 for lag in got["lags"][1:])
    assert got["matrices"][0] is None and len(got["matrices"]) == n_sweeps
    for a, b in zip(got["matrices"][1:], want["matrices"][1:]):
        assert np.array_equal(a, b)
    for key in set(want) - {"sweeps", "matrices", "lags"}:
        assert np.array_equal(got[key], want[key]), key
    assert set(got) == set(want) | {"sweep_names"} and "sweep_names" not in want
    back = pickle.loads(pickle.dumps(got))
    assert back["sweeps"][1:] == [None] * (n_sweeps - 1) and back["sweep_names"] == got["sweep_names"]
    assert np.array_equal(back["sweeps"][0], got["sweeps"][0]) and back["lags"] == got["lags"]
    assert all(np.array_equal(a, b) for a, b in zip(back["matrices"][1:], got["matrices"][1:]))


def test_sweep_cache_argument_checks(root):
    cfg = fx.make_cfg(True, False, True)
    with pytest.raises(ValueError, match="device"):
        WaymoDataset(cfg, root, "validation", device=None, sweep_cache=5)
    with pytest.raises(ValueError, match="training"):
        WaymoDataset(cfg, root, "training", device="cuda", sweep_cache=5)
    with pytest.raises(ValueError):
        WaymoDataset(cfg, root, "validation", device="cuda", sweep_cache=0)
    assert WaymoDataset(cfg, root, "validation", device="cuda").sweep_cache is None
    assert WaymoDataset(cfg, root, "testing", device="cuda", sweep_cache=1).sweep_cache == 1
