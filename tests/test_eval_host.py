"""CPU checks of the evaluation path (openseg3d_amd/evaluation.py, csrc/eval.hip host entries): IOUMetric against the
reference's own numbers, the test-time views against the reference's MultiScaleFlipAug (tests/golden/tta_views.npz,
written by tests/golden/make_golden_tta.py), the list form on a host-voxelizer dataset, the distributed confusion matrix
under gloo, and argument validation of the three new entry points."""
import ctypes
import math
import os
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tta_views.npz")
CART_RANGE = [-72, -72, -2, 72, 72, 4.4]
CART_VOXEL = [0.1, 0.1, 0.1]


def _golden():
    return np.load(GOLDEN)


# ------------------------------------------------------------------------------------------------ IOUMetric
def test_iou_metric_reference_main_case():
    from openseg3d_amd.evaluation import IOUMetric
    m = IOUMetric(["c0", "c1", "c2", "c3"])
    m.add(torch.Tensor([1, 2, 3]), torch.Tensor([1, 1, 3]))  # iou_metric.py:88-100
    m.add(torch.Tensor([0, 2, 3]), torch.Tensor([1, 3, 3]))
    r = m.get_metric()
    assert r["IOU"] == pytest.approx({"c0": 0.0, "c1": 1 / 3, "c2": 0.0, "c3": 2 / 3})
    assert r["mIOU"] == pytest.approx(0.25) and isinstance(r["mIOU"], float)
    g = _golden()
    assert np.array_equal(m.confusion_matrix(), g["iou4_hist"])
    assert np.allclose(list(r["IOU"].values()), g["iou4_iou"]) and r["mIOU"] == pytest.approx(float(g["iou4_miou"]))


def test_iou_metric_absent_class_and_ignored_uint8_labels():
    from openseg3d_amd.evaluation import IOUMetric
    g = _golden()
    names = [f"c{i}" for i in range(22)]
    preds, labels, cut = g["iou22_preds"], g["iou22_labels"], int(g["iou22_split"][0])
    m = IOUMetric(names)
    m.add(torch.from_numpy(preds[:cut]), torch.from_numpy(labels[:cut]))
    m.add(preds[cut:], labels[cut:].astype(np.uint8))  # uint8 labels as the loader delivers them, 255 = ignore
    assert np.array_equal(m.confusion_matrix(), g["iou22_hist"])
    r = m.get_metric()
    iou = np.array([r["IOU"][n] for n in names])
    assert math.isnan(r["IOU"]["c7"]) and np.array_equal(np.isnan(iou), np.isnan(g["iou22_iou"]))
    assert np.allclose(iou[~np.isnan(iou)], g["iou22_iou"][~np.isnan(iou)], rtol=0, atol=1e-15)
    assert r["mIOU"] == pytest.approx(float(np.nanmean(g["iou22_iou"])), abs=1e-15)
    assert r["mIOU"] == pytest.approx(float(g["iou22_miou"]), abs=1e-15)
    # fast_hist / per_class_iou keep their static signatures
    h = IOUMetric.fast_hist(np.array([0, 1, 1]), np.array([0, 1, 255]), 2)
    assert h.tolist() == [[1, 0], [0, 1]] and IOUMetric.per_class_iou(h).tolist() == [1.0, 1.0]


def test_iou_metric_nothing_added():
    from openseg3d_amd.evaluation import IOUMetric
    r = IOUMetric(["a", "b"]).get_metric()
    assert math.isnan(r["mIOU"]) and all(math.isnan(v) for v in r["IOU"].values())


# ------------------------------------------------------------------------------------------------ views
def _recipe(xyz, scale, c, s, fx, fy):
    """Numpy restatement of the view recipe (float32, no fused multiply-add)."""
    f = np.float32
    x, y, z = (xyz[:, 0] * f(scale)).astype(f), (xyz[:, 1] * f(scale)).astype(f), (xyz[:, 2] * f(scale)).astype(f)
    xr = (x * f(c)).astype(f) + (y * f(-s)).astype(f)
    yr = (x * f(s)).astype(f) + (y * f(c)).astype(f)
    if fx:
        yr = -yr
    if fy:
        xr = -xr
    return np.stack([xr, yr, z], axis=1).astype(f)


def _ulp_diff(a, b):
    """|a - b| of rotated [x, y, z] rows in ulps of the row's planar magnitude max(|x|, |y|): the reference's matmul may
    fuse or reorder the two products of a coordinate, which moves it by up to an ulp of the products, and x*c - y*s can
    cancel far below them.  z is not rotated and must agree exactly."""
    assert np.array_equal(a[..., 2], b[..., 2])
    mag = np.maximum(np.abs(a[..., :2]), np.abs(b[..., :2])).max(axis=-1, keepdims=True)
    return np.abs(a[..., :2].astype(np.float64) - b[..., :2].astype(np.float64)) / np.spacing(mag.astype(np.float32))


def test_view_table_order_and_constants():
    from openseg3d_amd import ops
    g = _golden()
    t = ops.tta_table(g["scales"].tolist(), g["angles"].tolist(), True, True)
    assert t.n_views == 36
    order = [(s, a, x, y) for s in range(3) for a in range(3) for x in (1, 0) for y in (1, 0)]
    for v, (s, a, x, y) in enumerate(order):
        w = t.views[v]
        assert (w.flip_x, w.flip_y) == (x, y)
        assert np.float32(w.scale) == np.float32(g["scales"][s])
        assert np.float32(w.cos_a) == g["cos_sin"][a, 0] and np.float32(w.sin_a) == g["cos_sin"][a, 1]
    t1 = ops.tta_table([1.0], [0.0, 0.5], False, True)
    assert t1.n_views == 4 and [(t1.views[v].flip_x, t1.views[v].flip_y) for v in range(4)] == [(0, 1), (0, 0)] * 2
    with pytest.raises(ValueError):
        ops.tta_table([1.0] * 5, [0.0] * 4, True, True)  # 80 views


def test_host_views_against_reference():
    from openseg3d_amd import ops
    g = _golden()
    frame = g["points"][:, 1:]
    n = frame.shape[0]
    t = ops.tta_table(g["scales"].tolist(), g["angles"].tolist(), True, True)
    out = ops.tta_views_host(frame, t)
    assert out.shape == (36 * n, 7) and out.dtype == np.float32
    views = out.reshape(36, n, 7)
    assert np.array_equal(views[:, :, 0], np.repeat(np.arange(36, dtype=np.float32)[:, None], n, axis=1))
    assert np.array_equal(views[:, :, 4:], np.broadcast_to(frame[:, 3:], (36, n, 3)))
    ref = g["view_xyz"]
    for v in range(36):
        a = (v // 4) % 3
        w = t.views[v]
        # the host twin is bit-exact against the recipe restated in numpy
        assert np.array_equal(views[v, :, 1:4], _recipe(frame, w.scale, w.cos_a, w.sin_a, w.flip_x, w.flip_y))
        if g["angles"][a] == 0:  # scale-only views: bit-exact against the reference
            assert np.array_equal(views[v, :, 1:4], ref[v])
        else:  # rotated: within 1 ulp of the reference's torch.matmul
            assert _ulp_diff(views[v, :, 1:4], ref[v]).max() <= 1.0
    # rotate_points_along_z alone (scale 1, no flip)
    t_rot = ops.tta_table([1.0], g["angles"].tolist(), False, False)
    rot = ops.tta_views_host(frame, t_rot).reshape(3, n, 7)[:, :, 1:4]
    assert _ulp_diff(rot, g["rot_xyz"]).max() <= 1.0
    # batch_period: column 0 cycles through 0 .. K-1
    t6 = ops.tta_table(g["scales"].tolist(), g["angles"].tolist(), True, True, batch_period=6)
    out6 = ops.tta_views_host(frame, t6)
    assert np.array_equal(out6[:, 1:], out[:, 1:]) and np.array_equal(out6[:, 0], out[:, 0] % 6)


class _HostDataset:
    """validation-mode WaymoDataset.prepare_data / collate_batch (waymo_dataset.py:248-279, 338-376) on the library's
    host voxelizer (batch.VoxelGenerator with a numpy array)."""

    use_cylinder, use_multi_sweeps, dim_point = False, False, 6

    def __init__(self):
        from openseg3d_amd import batch
        self.voxel_generator = batch.VoxelGenerator(CART_VOXEL, CART_RANGE)
        self.voxel_size, self.point_cloud_range = CART_VOXEL, CART_RANGE

    def prepare_data(self, data_dict):
        data_dict["cur_point_count"] = data_dict["points"].shape[0]
        data_dict["voxel_coords"], data_dict["point_voxel_ids"] = self.voxel_generator.generate(data_dict["points"])
        return data_dict

    @staticmethod
    def collate_batch(batch_list):
        data = defaultdict(list)
        for cur in batch_list:
            for k, v in cur.items():
                data[k].append(v)
        ret = {k: np.concatenate([np.pad(c, ((0, 0), (1, 0)), constant_values=i) for i, c in enumerate(data[k])])
               for k in ("points", "voxel_coords")}
        if "point_image_features" in data:
            ret["point_image_features"] = np.concatenate(data["point_image_features"])
        ids, count = [], 0
        for i, pv in enumerate(data["point_voxel_ids"]):
            ids.append(np.where(pv != -1, pv + count, -1))
            count += data["voxel_coords"][i].shape[0]
        ret["point_voxel_ids"] = np.concatenate(ids)
        ret["point_id_offset"] = np.cumsum(data["cur_point_count"])
        ret["batch_size"] = len(batch_list)
        return ret


@pytest.mark.parametrize("with_images", [False, True])
def test_list_form_call_matches_reference(with_images):
    from openseg3d_amd.evaluation import MultiScaleFlipAug
    g = _golden()
    ds = _HostDataset()
    aug = MultiScaleFlipAug(ds, scales=g["scales"].tolist(), angles=g["angles"].tolist(), flip_x=True, flip_y=True)
    assert repr(aug) == ("MultiScaleFlipAug(scales=[0.95, 1.0, 1.05], (angles=[-0.78539816, 0.0, 0.78539816], "
                         "(flip_x=[True, False], (flip_y=[True, False]")
    data = {"points": g["points"], "batch_size": 1}
    n = g["points"].shape[0]
    if with_images:
        data["point_image_features"] = np.arange(n * 4, dtype=np.float32).reshape(n, 4)
    views = aug(data)  # no point_image_features: the reference raises KeyError here
    assert len(views) == 36
    off = g["voxel_offsets"]
    moved = 0
    for v, d in enumerate(views):
        assert d["batch_size"] == 1 and d["points"].shape == (n, 7) and (d["points"][:, 0] == 0).all()
        assert ("point_image_features" in d) == with_images
        if with_images:
            assert np.array_equal(d["point_image_features"], data["point_image_features"])
        ref_ids, ref_coords = g["point_voxel_ids"][v], g["voxel_coords"][off[v]:off[v + 1]]
        if np.array_equal(d["point_voxel_ids"], ref_ids) and np.array_equal(d["voxel_coords"], ref_coords):
            continue
        # a point whose coordinate differs from the reference's in the last bit may sit on the other side of a voxel face
        xyz, ref_xyz = d["points"][:, 1:4], g["view_xyz"][v]
        diff = np.nonzero((xyz != ref_xyz).any(axis=1))[0]
        lo, vs = np.array(CART_RANGE[:3], np.float32), np.array(CART_VOXEL, np.float32)
        cell = np.floor((xyz[diff] - lo) / vs)
        cell_ref = np.floor((ref_xyz[diff] - lo) / vs)
        crossed = diff[(cell != cell_ref).any(axis=1)]
        moved += crossed.size
        # every other point keeps its voxel: compare the voxel coordinates point by point
        keep = np.setdiff1d(np.arange(n), crossed)
        mine = d["voxel_coords"][d["point_voxel_ids"][keep]]
        theirs = ref_coords[ref_ids[keep]]
        assert np.array_equal(mine[:, 1:], theirs[:, 1:])
    assert moved <= 1e-4 * 36 * n, f"{moved} points moved voxel"


# ------------------------------------------------------------------------------------------------ distributed
def test_distributed_hist_gloo_world_2():
    from openseg3d_amd import dist as D
    env = dict(os.environ, SEG3D_EVAL_RANK_OUT="1")
    port = D.free_port()
    procs = []
    for r in range(2):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_eval_rank.py")], env=e,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    import json
    res = [json.loads(next(ln for ln in o.splitlines() if ln.startswith("EVALRANK "))[len("EVALRANK "):]) for o in outs]
    g = _golden()
    from openseg3d_amd.evaluation import IOUMetric
    full = IOUMetric([f"c{i}" for i in range(22)])
    full.add(g["iou22_preds"], g["iou22_labels"])
    want = full.get_metric()
    for r in res:
        assert np.array_equal(np.array(r["hist"]), g["iou22_hist"])
        assert r["mIOU"] == pytest.approx(want["mIOU"], abs=1e-15)


# ------------------------------------------------------------------------------------------------ validation
def test_eval_entry_points_validate_arguments():
    from openseg3d_amd import _lib, ops
    lib = _lib.load()
    t = ops.tta_table([1.0], [0.0], True, True)
    buf = np.zeros(64, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)  # a valid pointer: only the sizes make these calls invalid
    # null pointers with work to do, bad dims, bad tables
    assert lib.seg3d_tta_views_f32(None, 10, 6, ctypes.byref(t), None, None) == _lib.EINVAL
    assert lib.seg3d_tta_views_host_f32(None, 10, 6, ctypes.byref(t), None) == _lib.EINVAL
    assert lib.seg3d_tta_views_f32(None, 10, 6, None, None, None) == _lib.EINVAL
    assert lib.seg3d_tta_views_f32(None, 0, 2, ctypes.byref(t), None, None) == _lib.EINVAL
    assert lib.seg3d_tta_views_f32(None, 0, 17, ctypes.byref(t), None, None) == _lib.EINVAL
    assert lib.seg3d_tta_views_f32(None, 0, 6, ctypes.byref(t), None, None) == 0  # nothing to do
    bad = ops.tta_table([1.0], [0.0], True, True)
    bad.n_views = 65  # V > 64
    assert lib.seg3d_tta_views_f32(None, 0, 6, ctypes.byref(bad), None, None) == _lib.EINVAL
    bad.n_views, bad.views[0].flip_x = 4, 2
    assert lib.seg3d_tta_views_host_f32(None, 0, 6, ctypes.byref(bad), None) == _lib.EINVAL
    big = ops.tta_table([1.0] * 4, [0.0] * 4, True, True)  # 64 views x 2^26 points overflows V*N
    assert lib.seg3d_tta_views_f32(p, 1 << 26, 6, ctypes.byref(big), p, None) == _lib.EINVAL
    assert lib.seg3d_tta_views_host_f32(p, 1 << 26, 6, ctypes.byref(big), p) == _lib.EINVAL
    # softmax accumulate: C > 64, V > 64, K*N overflow, nulls
    assert lib.seg3d_softmax_accumulate_f32(p, 10, 4, 65, 1, p, None) == _lib.EINVAL
    assert lib.seg3d_softmax_accumulate_f32(p, 10, 65, 22, 1, p, None) == _lib.EINVAL
    assert lib.seg3d_softmax_accumulate_f32(p, 10, 0, 22, 1, p, None) == _lib.EINVAL
    assert lib.seg3d_softmax_accumulate_f32(p, 1 << 26, 64, 22, 1, p, None) == _lib.EINVAL
    assert lib.seg3d_softmax_accumulate_f32(None, 10, 4, 22, 1, None, None) == _lib.EINVAL
    assert lib.seg3d_softmax_accumulate_f32(p, 10, 4, 22, 2, p, None) == _lib.EINVAL
    assert lib.seg3d_softmax_accumulate_f32(None, 0, 4, 22, 0, None, None) == 0
    # argmax + confusion: C > 64, both / neither prediction source, hist without labels, bad label width, nothing out
    assert lib.seg3d_argmax_confusion(p, None, 10, 65, 0, None, 0, p, None, None) == _lib.EINVAL
    assert lib.seg3d_argmax_confusion(p, None, 10, 0, 0, None, 0, p, None, None) == _lib.EINVAL
    assert lib.seg3d_argmax_confusion(p, p, 10, 22, 0, None, 0, None, p, None) == _lib.EINVAL
    assert lib.seg3d_argmax_confusion(None, None, 10, 22, 0, None, 0, p, None, None) == _lib.EINVAL
    assert lib.seg3d_argmax_confusion(p, None, 10, 22, 0, None, 0, None, p, None) == _lib.EINVAL
    assert lib.seg3d_argmax_confusion(p, None, 10, 22, 0, p, 4, None, p, None) == _lib.EINVAL
    assert lib.seg3d_argmax_confusion(p, None, 10, 22, 0, None, 0, None, None, None) == _lib.EINVAL
    assert lib.seg3d_argmax_confusion(None, p, 10, 22, 36, p, 1, None, p, None) == _lib.EINVAL
    assert lib.seg3d_argmax_confusion(p, None, -1, 22, 0, None, 0, p, None, None) == _lib.EINVAL
    assert lib.seg3d_argmax_confusion(p, None, 0, 22, 0, None, 0, p, None, None) == 0  # N = 0: nothing enqueued


def test_predict_argument_checks():
    from openseg3d_amd.evaluation import MultiScaleFlipAug

    class _Model(torch.nn.Module):
        pass

    ds = _HostDataset()
    aug = MultiScaleFlipAug(ds, scales=[0.95, 1.0, 1.05], angles=[-0.78539816, 0, 0.78539816], flip_x=True, flip_y=True)
    assert aug.n_views == 36 and aug.check_views_per_forward(None) >= 1
    for k in (0, 37):
        with pytest.raises(ValueError):
            aug.check_views_per_forward(k)
    with pytest.raises(ValueError):
        aug.check_views_per_forward(36, batch_size=8)  # 288 scenes > 255
    with pytest.raises(RuntimeError):
        aug.predict(_Model().train(), {"points": np.zeros((4, 7), np.float32), "batch_size": 1})
    with pytest.raises(ValueError):
        aug.predict(_Model().eval(), {"points": np.zeros((4, 7), np.float32), "batch_size": 2})
    ds.use_multi_sweeps = True
    with pytest.raises(NotImplementedError):
        aug.predict(_Model().eval(), {"points": np.zeros((4, 7), np.float32), "batch_size": 1})
