"""GPU checks of the frame assembly (csrc/frame.hip) and of ``WaymoDataset(device="cuda")``: each device entry against its
host twin and the numpy restatements of tests/frame_ref.py, ``assemble`` against what the reference's WaymoDataset
returned (tests/golden/dataset.npz), the training path against the host path, ``segment_test_frame`` end to end.

Tolerances.  Every column of frame_assemble but column 4 is bit-equal to the twin (one shared recipe, contraction off).
Column 4 is tanh from three libraries; device and twin are each compared with numpy in the rows' dtype, in ulp of 1.0.
Measured on the MI355X on these inputs: 0.50 ulp of 1.0 in float32 and in float64 (the twin 1.00 / 1.00);
the bound is 4 x that and at least 2 ulp, so another libm does not fail it: 2 ulp.  ``points`` of ``assemble`` equal
float32(reference): the record is conditioned so that neither the order of the three-term product nor the tanh library
can flip a float32 rounding.  Training: x, y within test_gpu_augment.py's 2 float32 ulp of the planar magnitude, everything else equal."""
import numpy as np
import pytest
import torch

import dataset_fixture as fx
import frame_ref
from aug_ref import check_rows
from test_dataset_host import matrix, range_image_case, raw_sweeps

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = fx.golden()
TANH_ULPS = {np.float32: 2.0, np.float64: 2.0}  # max(2, 4 x the measured 0.50)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("waymo"))
    fx.write(d, int(G["fixture_seed"]))
    return d


def tanh_ulps(got, raw_col):
    want = np.tanh(raw_col)
    assert got.dtype == want.dtype
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / float(np.finfo(want.dtype).eps)
    return float(err.max()) if err.size else 0.0


FRAME_CASES = {
    # name: (rows per sweep, dim, pass the [:, :dim] view of the raw [N, 15] rows)
    "mixed_stride6": ((611, 1, 0, 257), 6, False),
    "mixed_stride15": ((611, 1, 0, 257), 6, True),
    "single": ((333,), 6, True),
    "eight": ((5, 130, 3, 2, 300, 0, 7, 9), 7, True),
    "grid_wraps": ((65537, 65537, 65537), 6, False),  # 769 tiles on a grid capped at 512 workgroups
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(FRAME_CASES))
def test_frame_assemble_device_equals_twin(name, dtype):
    from openseg3d_amd import ops
    counts, dim, view = FRAME_CASES[name]
    raws = raw_sweeps(dtype, counts, seed=len(counts))
    mats = [None] + [matrix((i * 2) % 5) for i in range(1, len(counts))]
    lags = [0.0] + [0.1000370000001567 * i for i in range(1, len(counts))]
    host = [r[:, :dim] if view else np.ascontiguousarray(r[:, :dim]) for r in raws]
    dev = [_t(r)[:, :dim] if view else _t(r[:, :dim]) for r in raws]
    want = ops.frame_assemble_host(ops.sweep_table(host, mats, lags), want=("rows", "f32", "collated"), batch_id=5)
    got = ops.frame_assemble(ops.sweep_table(dev, mats, lags), want=("rows", "f32", "collated"), batch_id=5)
    torch.cuda.synchronize()
    n = sum(counts)
    assert got["rows"].shape == (n, dim) and got["f32"].shape == (n, dim) and got["collated"].shape == (n, dim + 1)
    rows, hrows = got["rows"].cpu().numpy(), want["rows"]
    keep = [k for k in range(dim) if k != 4]
    assert rows.dtype == dtype and rows[:, keep].tobytes() == hrows[:, keep].tobytes()
    raw4 = np.concatenate([r[:, 4] for r in raws])
    d_ulps, h_ulps = tanh_ulps(rows[:, 4], raw4), tanh_ulps(hrows[:, 4], raw4)
    print(f"{name} {np.dtype(dtype).name}: tanh against numpy, device {d_ulps:.2f} / twin {h_ulps:.2f} ulp of 1.0 "
          f"(bound {TANH_ULPS[dtype]})")
    assert d_ulps <= TANH_ULPS[dtype] and h_ulps <= TANH_ULPS[dtype]
    f32, col = got["f32"].cpu().numpy(), got["collated"].cpu().numpy()
    assert f32.tobytes() == rows.astype(np.float32).tobytes()  # .float(): round to nearest of the same values
    assert col[:, 1:].tobytes() == f32.tobytes() and (col[:, 0] == 5).all()
    assert f32[:, keep].tobytes() == want["f32"][:, keep].tobytes()
    # any subset of the outputs gives the same rows
    only = ops.frame_assemble(ops.sweep_table(dev, mats, lags), want=("collated",), batch_id=5)["collated"]
    assert torch.equal(only, got["collated"])


@pytest.mark.parametrize("pred_dtype", [np.int64, np.uint8])
@pytest.mark.parametrize("n", [0, 1, 1000])
def test_range_images_device_equals_twin(n, pred_dtype):
    from openseg3d_amd import ops
    pred, ri = range_image_case(n, pred_dtype)
    got = [t.cpu().numpy() for t in ops.range_image_labels(_t(pred), _t(ri), 22)]
    twin = ops.range_image_labels_host(pred, ri, 22)
    want = frame_ref.range_images(pred, ri)
    for k in range(2):
        assert got[k].dtype == np.int32 and got[k].shape == (64, 2650, 2)
        assert np.array_equal(got[k], twin[k]) and np.array_equal(got[k], want[k])
    if n == 1000:
        assert want[0].max() == 22 and (want[0][:, :, 1] == 1).any() and want[1].max() == 22
    if n:  # one point outside the image: counted, not written, and the wrapper raises
        bad = ri.copy()
        bad[0] = [2650, 0, 0]
        a, b, count = ops.range_image_labels(_t(pred), _t(bad), 22, check=False)
        assert int(count.item()) == 1
        with pytest.raises(IndexError):
            ops.range_image_labels(_t(pred), _t(bad), 22)


def check_sample(batch, case, lo, hi, vlo, vhi, b, n_cur, testing=False):
    """Rows [lo, hi) and voxels [vlo, vhi) of a collated device batch against a recorded sample."""
    pts = batch["points"][lo:hi].cpu().numpy()
    want = G[case + "_points"]
    assert pts.dtype == np.float32 and (pts[:, 0] == b).all()
    assert np.array_equal(pts[:, 1:], want.astype(np.float32)), case
    coords = batch["voxel_coords"][vlo:vhi].cpu().numpy()
    assert (coords[:, 0] == b).all() and np.array_equal(coords[:, 1:], G[case + "_voxel_coords"].astype(np.float32))
    ids = batch["point_voxel_ids"][lo:hi].cpu().numpy()
    rec = G[case + "_point_voxel_ids"].astype(np.int64)
    assert np.array_equal(ids, np.where(rec >= 0, rec + vlo, rec))
    if not testing:
        assert np.array_equal(batch["voxel_labels"][vlo:vhi].cpu().numpy(), G[case + "_voxel_labels"])
    assert n_cur == int(G[case + "_cur_point_count"])


@pytest.mark.parametrize("case", ["val_ms0", "val_ms1", "val_ms5", "val_cyl", "test_ms"])
def test_assemble_against_reference(root, case):
    ds, index, _ = fx.make_dataset(case, root, G, device=DEV)
    raw = ds[index]
    assert all(isinstance(s, np.ndarray) for s in raw["sweeps"]) and ds.collate_raw([raw])[0] is raw
    batch = ds.assemble([raw])
    rec = "val_ms5" if case == "test_ms" else case
    n, m = G[rec + "_points"].shape[0], G[rec + "_voxel_coords"].shape[0]
    assert batch["points"].shape[0] == n and batch["voxel_coords"].shape[0] == m and batch["batch_size"] == 1
    check_sample(batch, rec, 0, n, 0, m, 0, batch["point_row_offsets"][0], testing=case == "test_ms")
    assert batch["filename"] == [fx.case_name(case)]
    if case == "test_ms":
        assert batch["points_ri"].dtype == torch.int32
        assert np.array_equal(batch["points_ri"].cpu().numpy(), G["test_ms_points_ri"]) and "point_labels" not in batch
    else:
        assert np.array_equal(batch["point_labels"].cpu().numpy(), G[case + "_point_labels"])
    if ds.use_image_feature:
        assert np.array_equal(batch["point_image_features"].cpu().numpy(), G[rec + "_point_image_features"])


def test_assemble_collates_two_samples(root):
    raws = []
    for case in fx.COLLATE:
        ds, index, _ = fx.make_dataset(case, root, G, device=DEV)
        raws.append(ds.load_raw(index))
    batch = ds.assemble(raws)
    a, b = fx.COLLATE
    n0, m0 = G[a + "_points"].shape[0], G[a + "_voxel_coords"].shape[0]
    n1, m1 = G[b + "_points"].shape[0], G[b + "_voxel_coords"].shape[0]
    check_sample(batch, a, 0, n0, 0, m0, 0, batch["point_row_offsets"][0])
    check_sample(batch, b, n0, n0 + n1, m0, m0 + m1, 1, batch["point_row_offsets"][1] - batch["point_row_offsets"][0])
    assert np.array_equal(batch["point_voxel_ids"].cpu().numpy(), G["collate_point_voxel_ids"])
    assert batch["voxel_id_offset"].cpu().tolist() == G["collate_voxel_id_offset"].tolist()
    assert batch["point_id_offset"].cpu().tolist() == G["collate_point_id_offset"].tolist()
    assert batch["batch_size"] == int(G["collate_batch_size"]) == 2
    assert list(batch["point_labels"].shape) == G["collate_point_labels_shape"].tolist()
    assert list(batch["point_image_features"].shape) == G["collate_point_image_features_shape"].tolist()


@pytest.mark.parametrize("case", ["train_ms", "train_single"])
def test_training_assemble_reproduces_host_path(root, case):
    host, index, _ = fx.make_dataset(case, root, G)
    sample = host[index]
    dev, index, _ = fx.make_dataset(case, root, G, device=DEV, rng="numpy")  # re-seeded: the same file choices
    raw = dev[index]
    batch = dev.assemble([raw], draws=[host.last_draw])
    pts = batch["points"].cpu().numpy()
    assert (pts[:, 0] == 0).all()
    check_rows(np.ascontiguousarray(pts[:, 1:]), sample["points"], 2, case)
    check_rows(np.ascontiguousarray(pts[:, 1:]), G[case + "_points"], 2, case + " vs the reference")
    assert np.array_equal(batch["point_labels"].cpu().numpy(), sample["point_labels"])
    assert batch["point_row_offsets"] == [int(sample["cur_point_count"])]
    if dev.use_image_feature:
        assert np.array_equal(batch["point_image_features"].cpu().numpy(), sample["point_image_features"])
    same = np.array_equal(pts[:, 1:], sample["points"])
    if same:  # identical rows give identical voxels
        assert np.array_equal(batch["voxel_coords"][:, 1:].cpu().numpy(), sample["voxel_coords"].astype(np.float32))
        assert np.array_equal(batch["point_voxel_ids"].cpu().numpy(), sample["point_voxel_ids"])
        assert np.array_equal(batch["voxel_labels"].cpu().numpy(), sample["voxel_labels"])
    # rng="device": the frame comes out with the same number of rows, from the seed alone
    ds2, index, _ = fx.make_dataset(case, root, G, device=DEV)
    raw2 = ds2[index]
    assert 0 <= raw2["seed"] < 2 ** 32
    b1, b2 = ds2.assemble([raw2]), ds2.assemble([raw2])
    assert torch.equal(b1["points"], b2["points"]) and torch.equal(b1["voxel_labels"], b2["voxel_labels"])


def test_validation_dataset_feeds_model_and_metric(root):
    from oracle import params
    from openseg3d_amd import evaluation, segformer
    ds, index, _ = fx.make_dataset("test_ms", root, G, device=DEV)
    model = segformer.build_segmentor(ds.cfg, ds)
    params.fill_by_name(model, seed=0)
    model = model.to(DEV).eval()
    batch = ds.assemble([ds[index]])
    with torch.no_grad():
        logits = model(dict(batch))["point_out"]
    n_cur = G["test_ms_points_ri"].shape[0]
    assert logits.shape == (n_cur, 22)
    out = evaluation.segment_test_frame(model, batch, n_classes=22)
    pred = logits.argmax(dim=1).cpu().numpy()
    want = frame_ref.range_images(pred, G["test_ms_points_ri"])
    assert np.array_equal(out["ri_return1"], want[0]) and np.array_equal(out["ri_return2"], want[1])
    assert out["ri_return1"].dtype == np.int32 and want[0].any() and want[1].any()
    name = fx.case_name("test_ms")
    assert out["context_name"] == "segA0001" and out["frame_timestamp_micros"] == int(name.split("-")[1])
    # validation frames straight into evaluate(): no hand wiring
    val, vindex, _ = fx.make_dataset("val_ms1", root, G, device=DEV)
    metric = evaluation.evaluate(model, [val.assemble([val[vindex]])], [f"c{i}" for i in range(22)])
    assert 0.0 <= metric["mIOU"] <= 1.0
