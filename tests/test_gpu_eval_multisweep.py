"""Multi-sweep evaluation on the MI355X: ``MultiScaleFlipAug.predict`` / ``segment_frame`` / ``segment_test_frame`` on
frames with history sweeps (configs/waymo_multi_sweeps.yaml with image fusion) against the CPU oracle and across view
splits, the batches the model is handed (current rows, row offsets, the fusion kNN planned view by view), and
``WaymoDataset(sweep_cache=n)`` against the uncached ``assemble``.

Bars.  Probabilities against the oracle: 1e-4, the bar of tests/test_gpu_eval.py on the single-sweep model.  View split
(1 against 6 views per forward): 1e-6, the same test's figure.  Everything else is equality."""
import numpy as np
import pytest
import torch

import dataset_fixture as fx

pytestmark = pytest.mark.gpu

TTA_SCALES = [0.95, 1.0, 1.05]
TTA_ANGLES = [-0.78539816, 0, 0.78539816]
N_CUR, N_HISTORY = 1501, (1200, 1100)  # current rows: not a multiple of 4
REPRESENTATIVE = [(1.0, 0.0, 0, 0), (1.0, -0.78539816, 0, 0), (1.0, 0.78539816, 0, 0), (1.0, 0.0, 1, 0), (1.05, 0.0, 0, 0)]
G = fx.golden()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def built(dev):
    """configs/waymo_multi_sweeps.yaml + image fusion with seeded weights, as tests/test_gpu_parity.py builds it."""
    from oracle import params
    from openseg3d_amd import config, segformer
    cfg = config.default_cfg()
    cfg.DATASET.USE_MULTI_SWEEPS = True
    cfg.DATASET.USE_IMAGE_FEATURE = True
    ds = config.DatasetSpec(cfg)
    model = segformer.build_segmentor(cfg, ds)
    params.fill_by_name(model, seed=0)
    return model.to(dev).eval(), cfg, ds


def make_frame(history=True):
    """(collated rows [N_all, 7] with batch id 0, image features [N_CUR, 28]): 1501 current rows, then two copies of the
    scene's first 1200 and 1100 rows re-posed by a small ego motion, with lags 0.1 and 0.2."""
    from openseg3d_amd import scene
    cur = scene.make_small_scene(41, N_CUR, extent=10.0)
    assert cur.shape == (N_CUR, 6) and not cur[:, 3].any()
    sweeps = [cur]
    rs = np.random.RandomState(41)
    for i, n in enumerate(N_HISTORY if history else (), start=1):
        h = cur[:n].astype(np.float64)
        yaw = 0.01 * i
        c, s = np.cos(yaw), np.sin(yaw)
        h[:, :2] = h[:, :2] @ np.array([[c, -s], [s, c]]) + np.array([0.6 * i, -0.05 * i])
        h[:, :3] += rs.normal(0.0, 0.01, size=(n, 3))
        h[:, 3] = np.float32(0.1 * i)
        sweeps.append(h.astype(np.float32))
    rows = np.concatenate(sweeps, axis=0)
    assert int((rows[:, 3] == 0).sum()) == N_CUR
    return np.pad(rows, ((0, 0), (1, 0))), scene.make_image_features(41, N_CUR)


def frame_dict(history=True, dev=None):
    pts, img = make_frame(history)
    d = {"points": pts, "point_image_features": img, "point_id_offset": np.array([N_CUR]), "batch_size": 1}
    if dev is not None:
        d = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    return d


def _top2_gap(p):
    s = np.sort(p, axis=1)
    return s[:, -1] - s[:, -2]


def _representative(ds):
    from openseg3d_amd import ops
    from openseg3d_amd.evaluation import MultiScaleFlipAug

    class Representative(MultiScaleFlipAug):
        n_views = len(REPRESENTATIVE)

        def table(self, batch_period=0):
            t = ops.tta_table([1.0], [0.0] * 5, False, False, batch_period)
            ang = torch.tensor([a for _, a, _, _ in REPRESENTATIVE], dtype=torch.float32)
            for v, (s, _, fx_, fy) in enumerate(REPRESENTATIVE):
                t.views[v] = ops.TtaView(float(np.float32(s)), float(torch.cos(ang[v])), float(torch.sin(ang[v])), fx_, fy)
            return t

    return Representative(ds, scales=[1.0], angles=[0.0])


# ------------------------------------------------------------------------------------------------ oracle parity
@pytest.mark.parametrize("history", [True, False])
def test_predict_matches_oracle_on_representative_views(dev, built, history):
    """The mean probability over five views in groups of 2, 2, 1 against the oracle's, with and without history sweeps.
    Measured on the MI355X: 4.9e-7 with history, 4.1e-7 without (bar 1e-4)."""
    from oracle import index_ops, model as omodel
    from openseg3d_amd import batch as B, ops
    model, cfg, ds = built
    data = frame_dict(history)
    n_all = data["points"].shape[0]
    assert n_all == N_CUR + (sum(N_HISTORY) if history else 0)
    aug = _representative(ds)
    prob = aug.predict(model, data, views_per_forward=2)  # groups of 2, 2, 1 views
    assert prob.shape == (N_CUR, ds.num_classes) and prob.dtype == torch.float32
    prob = prob.cpu().numpy().astype(np.float64)
    # oracle: each view voxelized and forwarded alone on the CPU, softmaxed and averaged in fp64
    rows = ops.tta_views(torch.from_numpy(data["points"][:, 1:].copy()).to(dev), aug.table(batch_period=1))  # column 0 = 0: each view a one-frame batch
    ocfg = {"grid_size": index_ops.grid_size_of(ds.voxel_size, ds.point_cloud_range),
            "batching_info": [{int(k): v for k, v in lvl.items()} for lvl in cfg.MODEL.BATCHING_INFO],
            "window_shape": cfg.MODEL.WINDOW_SHAPE, "depths": cfg.MODEL.DEPTHS,
            "use_multi_sweeps": True, "use_image_feature": True}
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    img = torch.from_numpy(data["point_image_features"]).to(dev)
    ref = np.zeros_like(prob)
    for v in range(len(REPRESENTATIVE)):
        b = B.batch_from_resident(rows[v * n_all:(v + 1) * n_all], [N_CUR], ds.voxel_size, ds.point_cloud_range, img)
        cpu = {k: (t.cpu() if torch.is_tensor(t) else t) for k, t in b.items() if k != "point_voxel_index"}
        with torch.no_grad():
            lg = omodel.segformer_forward(cpu, sd, ocfg)["point_out"].double().numpy()
        assert lg.shape == prob.shape
        e = np.exp(lg - lg.max(axis=1, keepdims=True))
        ref += e / e.sum(axis=1, keepdims=True)
    ref /= len(REPRESENTATIVE)
    err = float(np.abs(prob - ref).max())
    print(f"history={history}: max |predict - oracle| = {err:.3e} over {N_CUR} x {ds.num_classes} probabilities")
    assert err <= 1e-4
    sure = _top2_gap(ref) > 1e-4
    assert np.array_equal(prob.argmax(axis=1)[sure], ref.argmax(axis=1)[sure])


# ------------------------------------------------------------------------------------------------ view split, metric
def test_view_split_36_views_segment_frame_and_metric(dev, built):
    from openseg3d_amd.evaluation import IOUMetric, MultiScaleFlipAug, segment_frame
    model, cfg, ds = built
    data = frame_dict(True, dev)
    aug = MultiScaleFlipAug(ds, scales=TTA_SCALES, angles=TTA_ANGLES, flip_x=True, flip_y=True)
    p1 = aug.predict(model, data, views_per_forward=1).cpu().numpy()
    p6 = aug.predict(model, data, views_per_forward=6).cpu().numpy()
    assert p1.shape == p6.shape == (N_CUR, ds.num_classes)
    err = float(np.abs(p6.astype(np.float64) - p1).max())
    print(f"36 views, 6 per forward against 1: max difference {err:.3e}")
    assert err < 1e-6
    assert np.abs(p1.astype(np.float64).sum(axis=1) - 1).max() < 1e-5
    rs = np.random.RandomState(2)
    labels = rs.randint(0, ds.num_classes, N_CUR).astype(np.uint8)
    labels[rs.rand(N_CUR) < 0.05] = 255
    names = [f"c{i}" for i in range(ds.num_classes)]
    metric = IOUMetric(names)
    pred = segment_frame(model, dict(data, point_labels=torch.from_numpy(labels).to(dev)), aug, metric,
                         views_per_forward=6).cpu().numpy()
    assert pred.shape == (N_CUR,) and np.array_equal(pred, p6.argmax(axis=1))
    assert np.array_equal(metric.confusion_matrix(), IOUMetric.fast_hist(pred, labels, ds.num_classes))
    assert metric.confusion_matrix().sum() == int((labels != 255).sum())


# ------------------------------------------------------------------------------------------------ what the model is handed
def test_batches_carry_current_rows(dev, built):
    from openseg3d_amd.evaluation import MultiScaleFlipAug
    model, cfg, ds = built
    data = frame_dict(True, dev)
    n_all = data["points"].shape[0]
    cur = torch.nonzero(data["points"][:, 4] == 0).view(-1)
    assert cur.shape[0] == N_CUR
    seen = []

    def hook(module, args):
        b = args[0]
        k = b["batch_size"]
        want = (torch.arange(k, device=dev).view(-1, 1) * n_all + cur.view(1, -1)).reshape(-1)
        assert torch.equal(b["cur_rows"], want) and b["cur_rows"].dtype == torch.int64
        assert b["point_row_offsets"] == [N_CUR * (j + 1) for j in range(k)]
        assert b["point_id_offset"].tolist() == b["point_row_offsets"]
        assert b["points"].shape == (k * n_all, 7) and b["point_image_features"].shape[0] == k * N_CUR
        assert torch.equal(b["points"][b["cur_rows"], 0], torch.arange(k, device=dev).repeat_interleave(N_CUR).float())
        assert not b["points"][b["cur_rows"], 4].any()
        # every view's fusion neighbours are rows of that view (searched with the batch, the reference's stride-3 read of
        # the [N, 6] rows would put the neighbours of view j > 0 among other views' rows)
        knn = b["fusion_knn"]
        assert knn.shape == (k * N_CUR, 16) and knn.dtype == torch.int32
        assert torch.equal(knn // N_CUR, torch.arange(k, device=dev, dtype=torch.int32).repeat_interleave(N_CUR)
                           .view(-1, 1).expand(-1, 16))
        seen.append(k)

    aug = MultiScaleFlipAug(ds, scales=[1.0, 1.05], angles=[0.0, 0.5], flip_x=True, flip_y=False)  # 8 views
    handle = model.register_forward_pre_hook(hook)
    try:
        out = aug.predict(model, data, views_per_forward=3)
    finally:
        handle.remove()
    assert seen == [3, 3, 2] and out.shape == (N_CUR, ds.num_classes)


def test_single_sweep_image_fusion_does_not_depend_on_the_view_split(dev):
    """The per-view neighbour search serves single-sweep configs with image features too: searched with the batch, the
    stride-3 read of the [N, 6] rows made views_per_forward > 1 differ from 1 by percents of probability."""
    from oracle import params
    from openseg3d_amd import config, segformer
    from openseg3d_amd.evaluation import MultiScaleFlipAug
    cfg = config.default_cfg()
    cfg.DATASET.USE_IMAGE_FEATURE = True
    ds = config.DatasetSpec(cfg)
    model = segformer.build_segmentor(cfg, ds)
    params.fill_by_name(model, seed=0)
    model = model.to(dev).eval()
    data = frame_dict(False, dev)
    aug = MultiScaleFlipAug(ds, scales=[1.0, 1.05], angles=[0.0, 0.5], flip_x=True, flip_y=False)  # 8 views
    p1 = aug.predict(model, data, views_per_forward=1).cpu().numpy().astype(np.float64)
    p3 = aug.predict(model, data, views_per_forward=3).cpu().numpy().astype(np.float64)
    err = float(np.abs(p3 - p1).max())
    print(f"single sweep + image features, 8 views, 3 per forward against 1: max difference {err:.3e}")
    assert p1.shape == (N_CUR, ds.num_classes) and err < 1e-6


def test_spnet_reads_the_planned_rows_and_neighbours(dev):
    """MODEL.SEGMENTOR='spnet' with multi-sweep image fusion takes ``cur_rows`` and ``fusion_knn`` from the batch as
    Segformer does: the view split changes nothing beyond the project's 1e-6."""
    from oracle import params
    from openseg3d_amd import config, segformer
    from openseg3d_amd.evaluation import MultiScaleFlipAug
    cfg = config.default_cfg()
    cfg.MODEL.SEGMENTOR = "spnet"
    cfg.DATASET.USE_MULTI_SWEEPS = cfg.DATASET.USE_IMAGE_FEATURE = True
    ds = config.DatasetSpec(cfg)
    model = segformer.build_segmentor(cfg, ds)
    params.fill_by_name(model, seed=3)
    model = model.to(dev).eval()
    data = frame_dict(True, dev)
    aug = MultiScaleFlipAug(ds, scales=[1.0, 1.05], angles=[0.0, 0.5], flip_x=True, flip_y=False)  # 8 views
    p1 = aug.predict(model, data, views_per_forward=1).cpu().numpy().astype(np.float64)
    p3 = aug.predict(model, data, views_per_forward=3).cpu().numpy().astype(np.float64)
    err = float(np.abs(p3 - p1).max())
    print(f"spnet, multi-sweep + image features, 8 views, 3 per forward against 1: max difference {err:.3e}")
    assert p1.shape == (N_CUR, ds.num_classes) and err < 1e-6


def test_current_row_count_is_checked(dev, built):
    from openseg3d_amd.evaluation import MultiScaleFlipAug
    model, cfg, ds = built
    aug = MultiScaleFlipAug(ds, scales=[1.0], angles=[0.0])
    data = frame_dict(True)
    for bad in (dict(data, point_id_offset=np.array([N_CUR - 1])), dict(data, point_row_offsets=[N_CUR + 1])):
        with pytest.raises(ValueError, match="current rows"):
            aug.predict(model, bad)
    lagged = dict(data, points=data["points"].copy())
    lagged["points"][7, 4] = 0.05  # one current row with a lag: 1500 rows at lag 0
    with pytest.raises(ValueError, match="current rows"):
        aug.predict(model, lagged)
    with pytest.raises(NotImplementedError, match="point_id_offset"):
        aug.predict(model, {k: v for k, v in data.items() if k != "point_id_offset"})


# ------------------------------------------------------------------------------------------------ the fixture directory
@pytest.fixture(scope="module")
def root(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("waymo"))
    fx.write(d, int(G["fixture_seed"]))
    return d


def test_testing_mode_range_images(dev, root):
    from oracle import params
    from openseg3d_amd import evaluation, ops, segformer
    ds, index, _ = fx.make_dataset("test_ms", root, G, device=dev)
    model = segformer.build_segmentor(ds.cfg, ds)
    params.fill_by_name(model, seed=0)
    model = model.to(dev).eval()
    batch = ds.assemble([ds[index]])
    n_cur = G["test_ms_points_ri"].shape[0]
    assert batch["points"].shape[0] > n_cur and "point_labels" not in batch
    aug = evaluation.MultiScaleFlipAug(ds, scales=[1.0, 1.05], angles=[0.0], flip_x=True, flip_y=False)  # 4 views
    out = evaluation.segment_test_frame(model, batch, aug, n_classes=22, views_per_forward=3)
    pred = evaluation.segment_frame(model, {k: v for k, v in batch.items() if k != "points_ri"}, aug, views_per_forward=3)
    assert pred.shape == (n_cur,)
    want = ops.range_image_labels_host(pred.cpu().numpy(), G["test_ms_points_ri"], 22)
    assert np.array_equal(out["ri_return1"], want[0]) and np.array_equal(out["ri_return2"], want[1])
    assert out["ri_return1"].dtype == np.int32 and want[0].any() and want[1].any()
    assert out["context_name"] == "segA0001"


def _segment_a(root, mode, dev, **kw):
    """Segment A's frames in frame order: all six in testing mode, the five labelled ones in validation mode."""
    from openseg3d_amd.dataset import WaymoDataset
    file_idx, n_frames, t0 = fx.SEGMENTS[0]
    ds = WaymoDataset(fx.make_cfg(True, False, True), root, mode, device=dev, **kw)
    ds.filenames = [fx.frame_name(file_idx, i, t0) for i in range(n_frames) if mode == "testing" or (file_idx, i) != fx.UNLABELLED]
    return ds


def _same_batch(a, b):
    assert set(a) == set(b)
    for key, va in a.items():
        vb = b[key]
        if torch.is_tensor(va):
            assert va.dtype == vb.dtype and torch.equal(va, vb), key
        elif key == "point_voxel_index":
            assert torch.equal(va.ids, vb.ids), key
        else:
            assert va == vb, key


@pytest.mark.parametrize("mode,order,capacity", [("testing", "forward", 5), ("testing", "reverse", 5), ("testing", "forward", 1),
                                                 ("testing", "reverse", 1), ("validation", "forward", 5)])
def test_sweep_cache_equals_uncached_assemble(dev, root, mode, order, capacity):
    plain, cached = _segment_a(root, mode, dev), _segment_a(root, mode, dev, sweep_cache=capacity)
    assert capacity in (1, plain.cfg.DATASET.MAX_NUM_SWEEPS) and cached.filenames == plain.filenames
    reads = []
    raw_points = cached._raw_points
    cached._raw_points = lambda name: (reads.append(name), raw_points(name))[1]
    indices = list(range(len(plain)))
    if order == "reverse":
        indices = indices[::-1]
    for i in indices:
        raw = cached[i]
        assert all(s is None for s in raw["sweeps"][1:])
        if mode == "testing":  # frame i of the segment has min(i, NUM_SWEEPS - 1) history sweeps
            assert len(raw["sweeps"]) == min(i, 2) + 1
        _same_batch(cached.assemble([raw]), plain.assemble([plain[i]]))
        assert len(cached._resident_sweeps) <= capacity
    if mode == "testing" and order == "forward" and capacity == 5:
        assert sorted(reads) == sorted(plain.filenames)  # every file read once, none twice
    # a batch of two frames from the warm cache
    _same_batch(cached.assemble([cached[indices[0]], cached[indices[-1]]]),
                plain.assemble([plain[indices[0]], plain[indices[-1]]]))
