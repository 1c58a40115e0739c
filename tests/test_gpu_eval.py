"""Evaluation path on the MI355X (csrc/eval.hip, openseg3d_amd/evaluation.py): the views kernel against its host twin,
the softmax accumulation against fp64 and across view splits, argmax + confusion matrix against numpy, and
MultiScaleFlipAug.predict / segment_frame end to end against the CPU oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TTA_SCALES = [0.95, 1.0, 1.05]
TTA_ANGLES = [-0.78539816, 0, 0.78539816]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dim,n", [(6, 4096), (6, 1001), (8, 777), (8, 3), (6, 1)])
@pytest.mark.parametrize("period", [0, 6])
def test_tta_views_bit_identical_to_host_twin(dev, dim, n, period):
    from openseg3d_amd import ops, scene
    pts = scene.make_small_scene(11, max(n, 8), extent=20.0)[:n]
    if dim == 8:  # cylinder-config width (two more columns)
        pts = np.concatenate([pts, np.random.RandomState(1).randn(n, 2).astype(np.float32)], axis=1)
    t = ops.tta_table(TTA_SCALES, TTA_ANGLES, True, True, batch_period=period)
    host = ops.tta_views_host(pts, t)
    got = ops.tta_views(torch.from_numpy(pts).to(dev), t).cpu().numpy()
    assert got.shape == host.shape == (36 * n, dim + 1)
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))
    # an unaligned source (element-wise path) gives the same bits
    buf = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), pts.ravel()])).to(dev)
    got2 = ops.tta_views(buf[1:].view(n, dim), t).cpu().numpy()
    assert np.array_equal(got2.view(np.uint32), host.view(np.uint32))


def _softmax_mean_fp64(logits, k, n):
    x = logits.reshape(k, n, -1).astype(np.float64)
    e = np.exp(x - x.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).mean(axis=0)


@pytest.mark.parametrize("n,c", [(1000, 22), (333, 22), (65, 64), (1, 3)])
def test_softmax_accumulate_fp64_and_split_invariance(dev, n, c):
    from openseg3d_amd import ops
    v = 36
    rs = np.random.RandomState(n + c)
    logits = (rs.randn(v * n, c) * 4).astype(np.float32)
    logits[::7] = 3.25  # rows of equal logits
    logits[1::11, 0] = 207.0  # large logits (the headline scene reaches 207)
    logits[2::13, 1] = -250.0
    logits[3::17] *= 60.0
    lg = torch.from_numpy(logits).to(dev)
    sums = {}
    for k in (1, 4, 36, 5):
        acc = torch.full((n, c), 12345.0, device=dev)  # overwritten by the first chunk
        for k0 in range(0, v, k):
            kk = min(k, v - k0)
            ops.softmax_accumulate(lg[k0 * n:(k0 + kk) * n], acc, first=k0 == 0)
        sums[k] = acc.cpu().numpy()
    for k in (4, 36, 5):
        assert np.array_equal(sums[k].view(np.uint32), sums[1].view(np.uint32)), k
    mean = sums[1].astype(np.float64) / v
    assert np.abs(mean - _softmax_mean_fp64(logits, v, n)).max() < 1e-6
    # accumulate onto an existing sum (first = False)
    acc = torch.from_numpy(sums[1]).to(dev)
    ops.softmax_accumulate(lg[:n], acc, first=False)
    assert np.abs(acc.cpu().numpy().astype(np.float64) - (sums[1] + _softmax_mean_fp64(logits[:n], 1, n))).max() < 1e-5


@pytest.mark.parametrize("n,c", [(0, 22), (1, 22), (5000, 22), (70001, 22), (3000, 64), (100, 1)])
@pytest.mark.parametrize("label_dtype", [np.uint8, np.int64])
def test_argmax_confusion_exact(dev, n, c, label_dtype):
    from openseg3d_amd import ops
    rs = np.random.RandomState(n + c)
    scores = rs.randint(0, 4, size=(n, c)).astype(np.float32)  # many ties: the first maximum must win
    labels = rs.randint(0, c, size=n).astype(label_dtype)
    labels[rs.rand(n) < 0.1] = 255
    if label_dtype == np.int64:
        labels[rs.rand(n) < 0.02] = -1
    hist = torch.zeros(c * c, dtype=torch.int64, device=dev)
    sc = torch.from_numpy(scores).to(dev)
    lb = torch.from_numpy(labels).to(dev)
    pred = ops.argmax_confusion(sc, labels=lb, hist=hist).cpu().numpy()
    want_pred = scores.argmax(axis=1) if n else np.zeros(0, np.int64)
    assert np.array_equal(pred, want_pred)

    def numpy_hist(p, g):
        g = g.astype(np.int64)
        k = (g >= 0) & (g < c)
        return np.bincount(c * g[k] + p[k], minlength=c * c)[:c * c]

    assert np.array_equal(hist.cpu().numpy(), numpy_hist(want_pred, labels))
    ops.argmax_confusion(sc, labels=lb, hist=hist, want_pred=False)  # a second call accumulates
    ops.argmax_confusion(pred_in=torch.from_numpy(want_pred).to(dev), n_classes=c, labels=lb, hist=hist)
    assert np.array_equal(hist.cpu().numpy(), 3 * numpy_hist(want_pred, labels))


def test_argmax_nan_and_mean_division(dev):
    from openseg3d_amd import ops
    nan = float("nan")
    s = torch.tensor([[1.0, nan, 2.0, nan], [nan, 5.0, 1.0, 0.0], [3.0, 3.0, 1.0, 3.0], [-1.0, -0.5, -0.5, -2.0]],
                     device=dev)
    assert ops.argmax_confusion(s).cpu().tolist() == torch.argmax(s.cpu(), dim=1).tolist() == [1, 0, 0, 1]
    # two distinct sums that tie after the division by V: the mean's argmax is the first of them
    a = np.float32(1.5000001)
    b = np.nextafter(a, np.float32(2))
    assert a != b and np.float32(a / np.float32(3)) == np.float32(b / np.float32(3))
    s = torch.tensor([[0.5, float(a), float(b)]], device=dev)
    assert ops.argmax_confusion(s).item() == 2 and ops.argmax_confusion(s, n_views=3).item() == 1


# ------------------------------------------------------------------------------------------------ end to end
def _model(dev, cyl):
    from oracle import params
    from openseg3d_amd import config, segformer
    cfg = config.default_cfg()
    if cyl:
        cfg.DATASET.USE_CYLINDER = True
        cfg.DATASET.POINT_CLOUD_RANGE = [0, -3.1415926, -2, 75.2, 3.1415926, 5.2]
        cfg.DATASET.VOXEL_SIZE = [0.05, 0.012, 0.1]
    ds = config.DatasetSpec(cfg)
    model = segformer.build_segmentor(cfg, ds)
    params.fill_by_name(model, seed=0)
    return model.to(dev).eval(), cfg, ds


def _top2_gap(p):
    s = np.sort(p, axis=1)
    return s[:, -1] - s[:, -2]


@pytest.mark.parametrize("cyl", [False, True])
def test_predict_matches_oracle_on_representative_views(dev, cyl):
    from oracle import index_ops, model as omodel
    from openseg3d_amd import batch as B, ops, scene
    from openseg3d_amd.evaluation import MultiScaleFlipAug
    model, cfg, ds = _model(dev, cyl)
    frame = scene.make_small_scene(31, 4000, extent=10.0)
    views = [(1.0, 0.0, 0, 0), (1.0, -0.78539816, 0, 0), (1.0, 0.78539816, 0, 0), (1.0, 0.0, 1, 0), (1.05, 0.0, 0, 0)]

    class Representative(MultiScaleFlipAug):
        n_views = len(views)

        def table(self, batch_period=0):
            t = ops.tta_table([1.0], [0.0] * 5, False, False, batch_period)
            ang = torch.tensor([a for _, a, _, _ in views], dtype=torch.float32)
            for v, (s, _, fx, fy) in enumerate(views):
                t.views[v] = ops.TtaView(float(np.float32(s)), float(torch.cos(ang[v])), float(torch.sin(ang[v])), fx, fy)
            return t

    aug = Representative(ds, scales=[1.0], angles=[0.0])
    data = {"points": np.pad(frame, ((0, 0), (1, 0))), "batch_size": 1}
    prob = aug.predict(model, data, views_per_forward=2).cpu().numpy().astype(np.float64)
    # oracle: each view voxelized alone, forwarded on the CPU, softmaxed and averaged in fp64
    rows = ops.tta_views(torch.from_numpy(frame).to(dev), aug.table()).cpu()
    n = frame.shape[0]
    ocfg = {"grid_size": index_ops.grid_size_of(ds.voxel_size, ds.point_cloud_range),
            "batching_info": [{int(k): v for k, v in lvl.items()} for lvl in cfg.MODEL.BATCHING_INFO],
            "window_shape": cfg.MODEL.WINDOW_SHAPE, "depths": cfg.MODEL.DEPTHS}
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    ref = np.zeros_like(prob)
    for v in range(len(views)):
        b = B.batch_from_resident(rows[v * n:(v + 1) * n].to(dev), [n], ds.voxel_size, ds.point_cloud_range,
                                  cylinder=cyl)
        cpu = {k: (t.cpu() if torch.is_tensor(t) else t) for k, t in b.items() if k != "point_voxel_index"}
        with torch.no_grad():
            lg = omodel.segformer_forward(cpu, sd, ocfg)["point_out"].double().numpy()
        e = np.exp(lg - lg.max(axis=1, keepdims=True))
        ref += e / e.sum(axis=1, keepdims=True)
    ref /= len(views)
    assert np.abs(prob - ref).max() <= 1e-4
    sure = _top2_gap(ref) > 1e-4
    assert np.array_equal(prob.argmax(axis=1)[sure], ref.argmax(axis=1)[sure])


@pytest.mark.parametrize("cyl", [False, True])
def test_predict_view_split_36_views(dev, cyl):
    from openseg3d_amd import scene
    from openseg3d_amd.evaluation import MultiScaleFlipAug, segment_frame
    model, cfg, ds = _model(dev, cyl)
    frame = scene.make_small_scene(32, 4000, extent=10.0)
    data = {"points": np.pad(frame, ((0, 0), (1, 0))), "batch_size": 1}
    aug = MultiScaleFlipAug(ds, scales=TTA_SCALES, angles=TTA_ANGLES, flip_x=True, flip_y=True)
    p1 = aug.predict(model, data, views_per_forward=1).cpu().numpy()
    p6 = aug.predict(model, data, views_per_forward=6).cpu().numpy()
    assert np.abs(p6.astype(np.float64) - p1).max() < 1e-6
    close = _top2_gap(p1.astype(np.float64)) < 1e-5
    differ = p6.argmax(axis=1) != p1.argmax(axis=1)
    assert not (differ & ~close).any(), int((differ & ~close).sum())
    # segment_frame = argmax of the same mean (the division inside the argmax kernel)
    pred = segment_frame(model, data, aug, views_per_forward=6).cpu().numpy()
    assert np.array_equal(pred, p6.argmax(axis=1))


def test_full_size_frame_36_views_and_metric(dev):
    from openseg3d_amd import scene
    from openseg3d_amd.evaluation import IOUMetric, MultiScaleFlipAug, segment_frame
    model, cfg, ds = _model(dev, False)
    frame = scene.make_scene(0)
    n = frame.shape[0]
    rs = np.random.RandomState(0)
    labels = rs.randint(0, 22, n).astype(np.uint8)
    labels[rs.rand(n) < 0.05] = 255
    data = {"points": torch.from_numpy(np.pad(frame, ((0, 0), (1, 0)))).to(dev), "batch_size": 1,
            "point_labels": torch.from_numpy(labels).to(dev)}
    aug = MultiScaleFlipAug(ds, scales=TTA_SCALES, angles=TTA_ANGLES, flip_x=True, flip_y=True)
    names = [f"c{i}" for i in range(22)]
    metric = IOUMetric(names)
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    pred = segment_frame(model, data, aug, metric)
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev)
    assert peak < 0.5 * torch.cuda.get_device_properties(dev).total_memory, peak
    p = pred.cpu().numpy()
    assert p.shape == (n,) and p.min() >= 0 and p.max() < 22
    want = IOUMetric.fast_hist(p, labels, 22)
    assert np.array_equal(metric.confusion_matrix(), want)
    host = IOUMetric(names)
    host.add(pred.cpu(), torch.from_numpy(labels))
    assert metric.get_metric() == host.get_metric() or np.allclose(
        list(metric.get_metric()["IOU"].values()), list(host.get_metric()["IOU"].values()), equal_nan=True)
    # IOUMetric.add on device tensors: the "labels in, hist out" mode
    dev_metric = IOUMetric(names)
    dev_metric.add(pred, data["point_labels"])
    assert np.array_equal(dev_metric.confusion_matrix(), want)
