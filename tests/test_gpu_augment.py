"""GPU checks of the training augmentation (csrc/augment.hip): every device entry against its host twin bit for bit, the
whole `apply` against the reference's recorded outputs (tests/golden/augment.npz) with the tolerances of
test_augment_host.py, the properties of rng="device", and one training forward on an augmented frame."""
import numpy as np
import pytest
import torch

import aug_ref
from aug_ref import case, check_rows, make_aug, recorded_draw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [np.float64, np.float32]


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _unaligned(a):
    """The same rows at an address that is a multiple of the element size only (no 16-byte alignment)."""
    flat = torch.empty((a.size + 1,), dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
    flat[1:] = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1).to(DEV)
    out = flat[1:].view(a.shape)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def _host_stage1(c, dtype):
    from openseg3d_amd import ops
    f1 = c.points1.astype(dtype)
    if c.multi:
        return f1, None, None, None
    f2 = c.points2.astype(dtype)
    src, op, _, _ = ops.polarmix_map_host(f1, f2, c.labels2, bool(c.swap), float(c.alpha), float(c.beta),
                                          [int(v) for v in c.instance_classes], len(c.paste_angles))
    return f1, f2, src, op


# ------------------------------------------------------------------------------------------------ device == host twin
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["swap_on", "swap_off"])
def test_polarmix_map_equals_host_twin(name, dtype):
    from openseg3d_amd import ops
    c = case(name)
    f1, f2, src, op = _host_stage1(c, dtype)
    classes = [int(v) for v in c.instance_classes]
    for labels in (c.labels2, c.labels2.astype(np.int64)):
        for a, b in ((_t(f1), _t(f2)), (_unaligned(f1), _unaligned(f2))):
            dsrc, dop, base, n_inst = ops.polarmix_map(a, b, _t(labels), bool(c.swap), float(c.alpha), float(c.beta),
                                                       classes, len(c.paste_angles))
            assert np.array_equal(dsrc.cpu().numpy(), src) and np.array_equal(dop.cpu().numpy(), op)
            assert base + (1 + len(c.paste_angles)) * n_inst == len(src)


@pytest.mark.parametrize("n1,n2,d,n_paste", [(0, 0, 6, 1), (5, 0, 3, 2), (0, 9, 6, 1), (13, 11, 16, 0), (700, 1200, 5, 8)])
def test_polarmix_map_edge_shapes_equal_host_twin(n1, n2, d, n_paste):
    from openseg3d_amd import ops
    rs = np.random.RandomState(n1 + n2)
    p1, p2 = rs.uniform(-10, 10, (n1, d)), rs.uniform(-10, 10, (n2, d))
    l2 = rs.randint(0, 5, n2).astype(np.uint8)  # 1200 rows: several blocks of the class histogram
    for swap in (True, False):
        for classes in ([4, 2, 0], []):
            want = ops.polarmix_map_host(p1, p2, l2, swap, -2.0, 1.0, classes, n_paste)
            got = ops.polarmix_map(_t(p1), _t(p2), _t(l2), swap, -2.0, 1.0, classes, n_paste)
            assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
            assert got[2:] == want[2:]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", aug_ref.CASES)
def test_apply_far_near_and_gather_equal_host_twin(name, dtype):
    from openseg3d_amd import ops
    c = case(name)
    f1, f2, src, op = _host_stage1(c, dtype)
    aug = make_aug(c)
    perm = c.perm.astype(np.int32)
    idx = ops.aug_gather_host(perm, None, c.choices.astype(np.int32))
    for batch_id in (None, 2):
        p = aug._params(recorded_draw(c), batch_id)
        want = ops.aug_apply_host(f1, f2, src, op, p)
        for a, b in ((_t(f1), _t(f2)), (_unaligned(f1), None if f2 is None else _unaligned(f2))):
            got = ops.aug_apply(a, b, _t(src), _t(op), p)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    p = aug._params(recorded_draw(c), None)
    pm_only = ops.aug_params(() if c.multi else c.paste_angles)
    assert np.array_equal(ops.aug_apply(_t(f1), _t(f2), _t(src), _t(op), pm_only).cpu().numpy().view(np.uint32),
                          ops.aug_apply_host(f1, f2, src, op, pm_only).view(np.uint32))
    far, near = ops.aug_far_near(_t(f1), _t(f2), _t(src), _t(op), _t(perm), p, float(c.sample_range))
    hfar, hnear = ops.aug_far_near_host(f1, f2, src, op, perm, p, float(c.sample_range))
    assert np.array_equal(far.cpu().numpy(), hfar) and np.array_equal(near.cpu().numpy(), hnear)
    flag = ops.aug_far_near(_t(f1), _t(f2), _t(src), _t(op), None, p, float(c.sample_range), lists=False)
    assert np.array_equal(flag.cpu().numpy(), ops.aug_far_near_host(f1, f2, src, op, None, p, float(c.sample_range), lists=False))
    # the maps, labels and features through the gather (1-, 4-, 8- and 16-byte rows)
    assert np.array_equal(ops.aug_gather(_t(perm), None, _t(c.choices.astype(np.int32))).cpu().numpy(), idx)
    if c.multi:
        pos, gat = ops.aug_cur_map(_t(idx), _t(c.cur_point_indices), len(f1))
        hpos, hgat = ops.aug_cur_map_host(idx, c.cur_point_indices, len(f1))
        assert np.array_equal(pos.cpu().numpy(), hpos) and np.array_equal(gat.cpu().numpy(), hgat)
        assert np.array_equal(hpos, c.out_cur)
        rows, l2, x2 = hgat, None, None
    else:
        rows, l2, x2 = ops.aug_gather_host(src, None, idx), c.labels2, c.feats2
    for a, b in ((c.labels1, l2), (c.labels1.astype(np.int64), None if l2 is None else l2.astype(np.int64)),
                 (c.feats1, x2), (c.feats1[:, :3], None if x2 is None else x2[:, :3])):
        got = ops.aug_gather(_t(a), _t(b), _t(rows)).cpu().numpy()
        assert np.array_equal(got, ops.aug_gather_host(a, b, rows))


@pytest.mark.parametrize("d", [3, 4, 7, 8, 16])
def test_apply_every_width_equals_host_twin(d):
    from openseg3d_amd import ops
    rs = np.random.RandomState(d)
    n1, n2 = 1001, 515  # more than one workgroup of four-row threads, not a multiple of 4
    src = rs.randint(-2, n1 + n2 + 2, 1499).astype(np.int32)  # rows outside both frames read as zeros
    op = rs.randint(0, 4, 1499).astype(np.uint8)  # op 3 has no angle: taken as a copy
    p = ops.aug_params([0.4, 2.2], 0.3, 1.02, (0.4, -0.7, 0.1), True, False, batch_id=1)
    for dtype in DTYPES:
        f1, f2 = rs.uniform(-60, 60, (n1, d)).astype(dtype), rs.uniform(-60, 60, (n2, d)).astype(dtype)
        got = ops.aug_apply(_t(f1), _t(f2), _t(src), _t(op), p).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ops.aug_apply_host(f1, f2, src, op, p).view(np.uint32))
        got = ops.aug_apply(_t(f1), None, None, None, p).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ops.aug_apply_host(f1, None, None, None, p).view(np.uint32))


@pytest.mark.parametrize("n,m,n_far", [(1501, 900, 1000), (1370, 1301, 160), (5000, 4750, 0), (3, 2, 1)])
def test_device_sampler_equals_host_twin(n, m, n_far):
    from openseg3d_amd import ops
    flag = np.zeros(n, np.uint8)
    flag[np.random.RandomState(n).permutation(n)[:n_far]] = 1
    got = ops.aug_sample_device(_t(flag), n, m, 99).cpu().numpy()
    assert np.array_equal(got, ops.aug_sample_host(flag, n, m, 99))
    assert np.array_equal(ops.aug_sample_device(None, n, m, 5, device=DEV).cpu().numpy(), ops.aug_sample_host(None, n, m, 5))


# ------------------------------------------------------------------------------------------------ against the reference
def _apply(c, aug, dtype=np.float64, **kw):
    f2 = {} if c.multi else dict(frame2=_t(c.points2.astype(dtype)), labels2=_t(c.labels2), image_features2=_t(c.feats2))
    cur = dict(cur_point_indices=_t(c.cur_point_indices)) if c.multi else {}
    return aug.apply(_t(c.points1.astype(dtype)), _t(c.labels1), _t(c.feats1), **f2, **cur, **kw)


@pytest.mark.parametrize("how", ["recorded", "seed"])
@pytest.mark.parametrize("name", aug_ref.CASES)
def test_apply_numpy_mode_matches_reference(name, how):
    c = case(name)
    kw = dict(params=recorded_draw(c)) if how == "recorded" else dict(seed=int(c.seed))
    out = _apply(c, make_aug(c), **kw)
    assert all(out[k].is_cuda for k in ("points", "point_labels", "point_image_features"))
    check_rows(out["points"].cpu().numpy(), c.out_points, 2, f"{name}: whole chain on the device ({how})")
    assert np.array_equal(out["point_labels"].cpu().numpy(), c.out_labels)
    assert np.array_equal(out["point_image_features"].cpu().numpy(), c.out_feats)
    if c.multi:
        assert np.array_equal(out["cur_point_indices"].cpu().numpy(), c.out_cur)
    else:
        assert out["cur_point_indices"] is None
    if how == "seed":
        assert np.array_equal(out["draw"].choices, c.choices)


# ------------------------------------------------------------------------------------------------ rng="device"
@pytest.mark.parametrize("name", aug_ref.CASES)
def test_device_mode_properties(name):
    c = case(name)
    aug = make_aug(c, rng="device")
    out, again = _apply(c, aug, seed=21), _apply(c, aug, seed=21)
    d = out["draw"]  # the scalars drawn from the seed; replayed below with another seed for shuffle / sample alone
    other = _apply(c, aug, params=d, seed=22)
    from openseg3d_amd import ops
    f1, f2, src, op = c.points1, None, None, None
    if not c.multi:
        f2 = c.points2
        src, op, _, _ = ops.polarmix_map_host(f1, f2, c.labels2, d.swap, d.alpha, d.beta,
                                              [int(v) for v in c.instance_classes], len(c.paste_angles))
    rows = out["source_rows"].cpu().numpy()
    n = len(f1) if src is None else len(src)  # rows after PolarMix
    m = min(int(n * float(c.sample_ratio)), n)
    assert len(rows) == m == out["points"].shape[0] and out["points"].dtype == torch.float32
    for k in ("points", "point_labels", "point_image_features", "source_rows"):
        assert torch.equal(out[k], again[k]), k
    assert len(other["source_rows"]) == m and not np.array_equal(rows, other["source_rows"].cpu().numpy())
    # a permutation prefix without duplicates; far rows are kept first
    p = aug._params(d, None)
    flag = ops.aug_far_near_host(f1, f2, src, op, None, p, float(c.sample_range), lists=False).astype(bool)
    idx = ops.aug_sample_host(flag.astype(np.uint8), n, m, 21)
    assert len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < n
    assert np.array_equal(rows, idx if src is None else src[idx])
    if flag.sum() <= m:
        assert flag[idx].sum() == flag.sum()  # every far row is kept
    else:
        assert flag[idx].all()
    assert not np.array_equal(np.sort(idx), idx)
    # rows, labels and features follow the map
    if c.multi:
        cur = out["cur_point_indices"].cpu().numpy()
        is_cur = np.isin(rows, c.cur_point_indices)
        assert np.array_equal(cur, np.where(is_cur)[0])
        assert np.array_equal(out["point_labels"].cpu().numpy(), c.labels1[rows[is_cur]])
        assert np.array_equal(out["point_image_features"].cpu().numpy(), c.feats1[rows[is_cur]])
        hist = out["points"].cpu().numpy()[:, 3:]
        assert np.array_equal(hist, c.points1[rows, 3:].astype(np.float32))
    else:
        assert np.array_equal(out["point_labels"].cpu().numpy(), np.concatenate([c.labels1, c.labels2])[rows])
        assert np.array_equal(out["point_image_features"].cpu().numpy(), np.concatenate([c.feats1, c.feats2])[rows])


# ------------------------------------------------------------------------------------------------ into a training step
def test_augmented_frame_trains():
    from openseg3d_amd import batch as B, config, losses, ops, segformer
    c = case("swap_on")
    cfg = config.default_cfg()
    ds = config.DatasetSpec(cfg)
    torch.manual_seed(0)
    model = segformer.build_segmentor(cfg, ds).to(DEV).train()
    crit = losses.build_criterion(cfg, ds)
    out = _apply(c, make_aug(c, rng="device"), seed=4, batch_id=0)
    n = out["points"].shape[0]
    b = B.batch_from_resident(out["points"], [n], ds.voxel_size, ds.point_cloud_range)
    b["point_labels"] = out["point_labels"].long()
    n_vox = b["voxel_coords"].shape[0]
    b["voxel_labels"] = ops.prepare_voxel_labels(b["point_voxel_ids"], out["point_labels"], n_vox).long()
    # a numpy vote over the augmented rows (waymo_dataset.py:213-246)
    ids, lab = b["point_voxel_ids"].cpu().numpy(), out["point_labels"].cpu().numpy()
    votes = np.zeros((n_vox, 256), np.int64)
    np.add.at(votes, (ids[ids >= 0], lab[ids >= 0]), 1)
    want = np.where(votes.sum(1) > 0, votes.argmax(1), 255)
    assert np.array_equal(b["voxel_labels"].cpu().numpy(), want) and (want != 255).any()
    res = model(b)
    loss = losses.compute_loss(res, b, crit, cfg)
    loss.backward()
    assert res["point_out"].shape[0] == n and torch.isfinite(loss)
