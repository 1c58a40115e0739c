"""CPU checks of the training augmentation (openseg3d_amd/augment.py, the host entries of csrc/augment.hip) against the
reference's PolarMix and transforms as recorded in tests/golden/augment.npz (tests/golden/make_golden_aug.py).

Tolerances.  Row selection, row order, labels, features, shuffle / sample indices and every column but x, y are compared
for equality.  x, y after the global rotation are allowed 2 float32 ulp of the output row's planar magnitude: one ulp is
what the test-time-augmentation tests already grant the reference's float32 torch.matmul (its BLAS may fuse the two
products), the second covers a last-bit difference of the float64 paste rotation (np.dot, BLAS again) flipping the
float32 rounding in front of a norm-preserving rotation.  Before the global rotation, copied rows are bit-exact and
pasted rows get that second ulp alone."""
import numpy as np
import pytest

import aug_ref
from aug_ref import case, check_rows, make_aug, np_polarmix_rows, recorded_draw

from openseg3d_amd import augment, ops  # noqa: E402
from openseg3d_amd._lib import Seg3dError  # noqa: E402

MIX_CASES = ("swap_on", "swap_off")


def _cat(c):
    return np.concatenate([c.points1, c.points2])


# ------------------------------------------------------------------------------------------------ stage 1: PolarMix
@pytest.mark.parametrize("name", MIX_CASES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_polarmix_map_row_selection_and_order(name, dtype):
    c = case(name)
    pm = make_aug(c).polar_mix
    p1, p2 = c.points1.astype(dtype), c.points2.astype(dtype)
    if dtype == np.float32 and bool(c.swap):  # rounding the frames moves no yaw across a sector bound
        xy = np.concatenate([p1, p2])[:, :2].astype(np.float64)
        yaw = -np.arctan2(xy[:, 1], xy[:, 0])
        assert min(np.abs(yaw - float(c.alpha)).min(), np.abs(yaw - float(c.beta)).min()) > 1e-6
    src, op = pm.row_map(p1, p2, c.labels2, bool(c.swap), float(c.alpha), float(c.beta))
    assert src.dtype == np.int32 and op.dtype == np.uint8 and len(src) == len(c.pm_xyz)
    want_src, want_op = np_polarmix_rows(c.points1, c.points2, c.labels2, bool(c.swap), float(c.alpha), float(c.beta),
                                         c.instance_classes, len(c.paste_angles))
    assert np.array_equal(src, want_src) and np.array_equal(op, want_op)
    # against the reference itself: copied rows are the reference's rows, labels and features follow the same map
    copied = op == 0
    assert np.array_equal(_cat(c)[src[copied], :3], c.pm_xyz[copied])
    assert np.array_equal(ops.aug_gather_host(c.labels1, c.labels2, src), c.pm_labels)
    assert np.array_equal(ops.aug_gather_host(c.feats1, c.feats2, src), c.pm_feats)
    if bool(c.swap):
        assert 0 < int((src[copied] >= len(p1)).sum()) and int((src < len(p1)).sum()) < len(p1)  # the sector is in use
    assert int((op == 2).sum()) == int((op == 1).sum()) > 0


@pytest.mark.parametrize("name", MIX_CASES)
def test_polarmix_call_matches_reference(name):
    c = case(name)
    pm = make_aug(c).polar_mix
    points, feats, labels = pm(c.points1, c.feats1, c.labels1, c.points2, c.feats2, c.labels2,
                               draw=(bool(c.swap), float(c.alpha), float(c.beta)))
    assert np.array_equal(labels, c.pm_labels) and np.array_equal(feats, c.pm_feats)
    src, op = pm.row_map(c.points1, c.points2, c.labels2, bool(c.swap), float(c.alpha), float(c.beta))
    want = np.concatenate([c.pm_xyz, _cat(c)[src, 3:]], axis=1).astype(np.float32)
    copied = op == 0
    assert np.array_equal(points[copied], want[copied])  # bit for bit
    check_rows(points[~copied], want[~copied], 1, f"{name}: pasted rows before the global rotation")
    points2, labels2 = pm(c.points1, None, c.labels1, c.points2, None, c.labels2,
                          draw=(bool(c.swap), float(c.alpha), float(c.beta)))
    assert np.array_equal(points2, points) and np.array_equal(labels2, labels)


def test_polarmix_draw_order():
    pm = augment.PolarMix([0, 1], [0.5])
    for seed in range(6):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        swap, alpha, beta = pm.draw(a)
        want_swap = b.random() < 0.5
        assert swap == want_swap
        if swap:
            assert alpha == (b.random() - 1) * np.pi and beta == alpha + np.pi
        b.random()
        assert a.random() == b.random()


# ------------------------------------------------------------------------------------------------ stage 3: the recipe
def _frames(c):
    return (c.points1, None) if c.multi else (c.points1, c.points2)


def _stage1(c):
    if c.multi:
        return None, None
    return make_aug(c).polar_mix.row_map(c.points1, c.points2, c.labels2, bool(c.swap), float(c.alpha), float(c.beta))


@pytest.mark.parametrize("name", aug_ref.CASES)
def test_global_rotation_alone(name):
    c = case(name)
    f1, f2 = _frames(c)
    src, op = _stage1(c)
    paste = () if c.multi else c.paste_angles
    got = ops.aug_apply_host(f1, f2, src, op, ops.aug_params(paste, rot_angle=float(c.rot)))
    check_rows(got[:, :3], c.xyz_rot, 2, f"{name}: after RandomGlobalRotation")


@pytest.mark.parametrize("name", aug_ref.CASES)
def test_scale_translate_flip_alone_bit_exact(name):
    c = case(name)
    rows = np.ascontiguousarray(c.xyz_rot)  # the reference's own rotated rows: rotation angle 0 from here on
    p = ops.aug_params((), 0.0, 1.0, (0, 0, 0), False, False)
    assert np.array_equal(ops.aug_apply_host(rows, None, None, None, p), rows)
    p = ops.aug_params((), 0.0, float(c.scale))
    assert np.array_equal(ops.aug_apply_host(rows, None, None, None, p), c.xyz_scale)
    p = ops.aug_params((), 0.0, float(c.scale), c.offsets)
    assert np.array_equal(ops.aug_apply_host(rows, None, None, None, p), c.xyz_translate)
    p = ops.aug_params((), 0.0, float(c.scale), c.offsets, bool(c.flips[0]), bool(c.flips[1]))
    assert np.array_equal(ops.aug_apply_host(rows, None, None, None, p), c.xyz_flip)
    for fx in (False, True):
        for fy in (False, True):
            p = ops.aug_params((), 0.0, 1.0, (0, 0, 0), fx, fy)
            want = rows * np.array([-1.0 if fy else 1.0, -1.0 if fx else 1.0, 1.0], np.float32)
            assert np.array_equal(ops.aug_apply_host(rows, None, None, None, p), want)


@pytest.mark.parametrize("name", aug_ref.CASES)
def test_chain_before_shuffle(name):
    c = case(name)
    f1, f2 = _frames(c)
    src, op = _stage1(c)
    d = recorded_draw(c)
    got = ops.aug_apply_host(f1, f2, src, op, make_aug(c)._params(d, None))
    check_rows(got[:, :3], c.xyz_flip, 2, f"{name}: after RandomFlip")


# ------------------------------------------------------------------------------------------------ stage 2: the maps
@pytest.mark.parametrize("name", aug_ref.CASES)
def test_far_near_lists_and_sample_draws(name):
    c = case(name)
    aug = make_aug(c)
    f1, f2 = _frames(c)
    src, op = _stage1(c)
    d = recorded_draw(c, with_choices=False)
    perm = c.perm.astype(np.int32)
    far, near = ops.aug_far_near_host(f1, f2, src, op, perm, aug._params(d, None), float(c.sample_range))
    dist = np.linalg.norm(c.xyz_flip[c.perm][:, :2], axis=1)  # the reference's shuffled rows
    assert np.array_equal(far, np.where(dist >= float(c.sample_range))[0])
    assert np.array_equal(near, np.where(dist < float(c.sample_range))[0])
    assert len(far) == int(c.n_far) and len(far) > 0 and len(near) > 0
    if c.multi:
        assert len(far) > aug.num_samples(len(perm))  # the case that thins the far rows as well
    flag = ops.aug_far_near_host(f1, f2, src, op, perm, aug._params(d, None), float(c.sample_range), lists=False)
    assert np.array_equal(flag.astype(bool), dist >= float(c.sample_range))


@pytest.mark.parametrize("name", aug_ref.CASES)
def test_draws_consume_numpy_random_as_the_reference(name):
    c = case(name)
    aug = make_aug(c)
    rs = np.random.RandomState(int(c.seed))
    polar = None if c.multi else aug.polar_mix.draw(rs)
    if not c.multi:
        assert polar == (bool(c.swap), float(c.alpha), float(c.beta))
    n = len(c.perm)
    d = aug.draw(n, rs, polar)
    assert d.rot == float(c.rot) and d.scale == float(c.scale) and d.offsets == [float(v) for v in c.offsets]
    assert (d.flip_x, d.flip_y) == (bool(c.flips[0]), bool(c.flips[1])) and np.array_equal(d.perm, c.perm)
    f1, f2 = _frames(c)
    src, op = _stage1(c)
    far, near = ops.aug_far_near_host(f1, f2, src, op, d.perm.astype(np.int32), aug._params(d, None), float(c.sample_range))
    assert np.array_equal(aug.draw_sample(n, far, near, rs), c.choices)
    assert rs.random() == float(c.next_draw)


def test_draw_skips_a_narrow_scale_range():
    aug = augment.TrainAugmentation(aug_ref.ROT_RANGE, [1.0, 1.0005], 0.5, 0.95, 50.0, rng="numpy")
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    d = aug.draw(10, a)
    rot = b.uniform(*aug_ref.ROT_RANGE)
    off = [b.normal(0, 0.5, 1)[0] for _ in range(3)]
    assert d.rot == rot and d.scale == 1.0 and d.offsets == off


@pytest.mark.parametrize("name", aug_ref.CASES)
def test_multi_stage_maps(name):
    """src2 = src[perm][choices], and for the multi-sweep case both get_shuffled_indices loops."""
    c = case(name)
    src, op = _stage1(c)
    perm, choices = c.perm.astype(np.int32), c.choices.astype(np.int32)
    idx = ops.aug_gather_host(perm, None, choices)
    assert np.array_equal(idx, c.perm[c.choices])
    if not c.multi:
        assert np.array_equal(ops.aug_gather_host(src, None, idx), src[c.perm][c.choices])
        assert np.array_equal(ops.aug_gather_host(op, None, idx), op[c.perm][c.choices])
        labels = ops.aug_gather_host(c.labels1, c.labels2, ops.aug_gather_host(src, None, perm))
        assert np.array_equal(labels, c.shuffle_labels)
        return
    n = len(c.points1)
    pos, gat = ops.aug_cur_map_host(perm, c.cur_point_indices, n)  # after PointShuffle
    assert np.array_equal(pos, c.shuffle_cur) and np.array_equal(c.labels1[gat], c.shuffle_labels)
    pos, gat = ops.aug_cur_map_host(idx, c.cur_point_indices, n)  # after PointSample, in one step
    assert np.array_equal(pos, c.out_cur) and np.array_equal(c.labels1[gat], c.out_labels)
    assert np.array_equal(ops.aug_gather_host(c.feats1, None, gat), c.out_feats)


# ------------------------------------------------------------------------------------------------ the whole frame
def _apply(c, aug, dtype=np.float64, **kw):
    f2 = {} if c.multi else dict(frame2=c.points2.astype(dtype), labels2=c.labels2, image_features2=c.feats2)
    cur = dict(cur_point_indices=c.cur_point_indices) if c.multi else {}
    return aug.apply(c.points1.astype(dtype), c.labels1, c.feats1, **f2, **cur, **kw)


def _check_frame(c, out, what):
    check_rows(out["points"], c.out_points, 2, what)
    assert np.array_equal(out["point_labels"], c.out_labels) and out["point_labels"].dtype == c.labels1.dtype
    assert np.array_equal(out["point_image_features"], c.out_feats)
    if c.multi:
        assert np.array_equal(out["cur_point_indices"], c.out_cur)
    else:
        assert out["cur_point_indices"] is None


@pytest.mark.parametrize("name", aug_ref.CASES)
def test_apply_replays_the_recorded_draw(name):
    c = case(name)
    _check_frame(c, _apply(c, make_aug(c), params=recorded_draw(c)), f"{name}: whole chain, recorded draw")


@pytest.mark.parametrize("name", aug_ref.CASES)
def test_apply_draws_from_the_seed_as_the_reference(name):
    c = case(name)
    out = _apply(c, make_aug(c), seed=int(c.seed))
    assert np.array_equal(out["draw"].choices, c.choices)
    _check_frame(c, out, f"{name}: whole chain, drawn from the seed")


def test_apply_int64_labels_and_batch_column():
    c = case("swap_on")
    f2 = dict(frame2=c.points2, labels2=c.labels2.astype(np.int64))
    out = make_aug(c).apply(c.points1, c.labels1.astype(np.int64), **f2, params=recorded_draw(c), batch_id=3)
    assert out["point_labels"].dtype == np.int64 and np.array_equal(out["point_labels"], c.out_labels)
    assert out["point_image_features"] is None and np.all(out["points"][:, 0] == 3.0)
    check_rows(np.ascontiguousarray(out["points"][:, 1:]), c.out_points, 2, "collated rows")


def test_from_config_reads_the_aug_keys():
    from openseg3d_amd.config import default_cfg
    cfg = default_cfg()
    a, b = np.random.RandomState(2), np.random.RandomState(2)
    aug = augment.TrainAugmentation.from_config(cfg, rng_state=a)
    d = cfg.DATASET
    assert aug.rot_range == list(d.AUG_ROT_RANGE) and aug.scale_range == list(d.AUG_SCALE_RANGE)
    assert (aug.translate_std, aug.sample_ratio, aug.sample_range) == (d.AUG_TRANSLATE_STD, d.AUG_SAMPLE_RATIO,
                                                                     d.AUG_SAMPLE_RANGE)
    assert aug.dim_point == d.DIM_POINT and aug.rng == "device"
    assert aug.polar_mix.instance_classes == list(range(13))  # waymo_dataset.py:37-39
    assert aug.polar_mix.rot_angle_range == [b.random() * np.pi * 2 / 3, (b.random() + 1) * np.pi * 2 / 3]
    d.USE_MULTI_SWEEPS = True
    assert augment.TrainAugmentation.from_config(cfg).polar_mix is None  # waymo_dataset.py:307
    # DIM_POINT columns of a wider frame are used (:295)
    c = case("sweeps")
    wide = np.concatenate([c.points1, np.ones((len(c.points1), 9))], axis=1)
    aug = make_aug(c)
    aug.dim_point = 6
    out = aug.apply(wide, c.labels1, c.feats1, cur_point_indices=c.cur_point_indices, params=recorded_draw(c))
    _check_frame(c, out, "15-column frame cut to DIM_POINT")


# ------------------------------------------------------------------------------------------------ rng="device"
@pytest.mark.parametrize("n,m,n_far", [(1000, 950, 100), (1000, 600, 700), (7, 7, 0), (1, 0, 1), (0, 0, 0)])
def test_device_mode_sampler_host_twin(n, m, n_far):
    rs = np.random.RandomState(n + m)
    flag = np.zeros(n, np.uint8)
    flag[rs.permutation(n)[:n_far]] = 1
    a = ops.aug_sample_host(flag, n, m, 1234)
    assert len(a) == m and len(set(a.tolist())) == m and (m == 0 or (a.min() >= 0 and a.max() < n))
    if n_far <= m:
        assert set(np.where(flag)[0].tolist()) <= set(a.tolist())  # every far row is kept
    else:
        assert flag[a].all()  # only far rows are kept
    assert np.array_equal(a, ops.aug_sample_host(flag, n, m, 1234))
    if m > 5:
        b = ops.aug_sample_host(flag, n, m, 1235)
        assert not np.array_equal(a, b) and not np.array_equal(np.sort(a), a)
    if n:
        assert len(ops.aug_sample_host(None, n, m, 7)) == m


def test_device_mode_apply_on_the_host():
    c = case("sweeps")
    aug = make_aug(c, rng="device")
    out = _apply(c, aug, seed=11)
    again = _apply(c, aug, seed=11)
    other = _apply(c, aug, seed=12)
    m = aug.num_samples(len(c.points1))
    assert out["points"].shape == (m, 6) and np.array_equal(out["points"], again["points"])
    assert not np.array_equal(out["points"], other["points"])
    cur, rows = out["cur_point_indices"], out["source_rows"]
    assert len(set(rows.tolist())) == m  # no row twice
    is_cur = np.isin(rows, c.cur_point_indices)
    assert np.array_equal(cur, np.where(is_cur)[0])  # exactly the rows whose source is a current-sweep point
    assert np.array_equal(out["point_labels"], c.labels1[rows[is_cur]])  # cur_point_indices = arange: slot == point
    assert np.array_equal(out["point_image_features"], c.feats1[rows[is_cur]])
    # only far rows survive in this case (more far rows than samples): every kept row lies outside the range
    dist = np.linalg.norm(out["points"][:, :2], axis=1)
    assert (dist >= float(c.sample_range)).all()


# ------------------------------------------------------------------------------------------------ edge cases
def _rows(n, d, seed, dtype=np.float64):
    rs = np.random.RandomState(seed)
    return rs.uniform(-10, 10, (n, d)).astype(dtype)


@pytest.mark.parametrize("n1,n2,d,angles,swap", [
    (0, 0, 6, [0.3], True),        # no rows at all
    (5, 0, 3, [0.3, 1.0], True),   # no second frame rows, D = 3, N not a multiple of 4
    (0, 9, 6, [0.3], True),        # nothing in frame 1
    (13, 11, 16, [], True),        # R = 0, D = 16
    (13, 11, 6, [0.1] * 8, False), # R = 8, swap off
    (1003, 701, 4, [2.0], True),
])
def test_polarmix_edge_shapes(n1, n2, d, angles, swap):
    p1, p2 = _rows(n1, d, 1), _rows(n2, d, 2)
    l2 = np.random.RandomState(3).randint(0, 6, n2).astype(np.uint8)
    classes = [4, 2]
    alpha, beta = -2.0, 1.1415926
    pm = augment.PolarMix(classes, angles)
    src, op = pm.row_map(p1, p2, l2, swap, alpha, beta)
    want_src, want_op = np_polarmix_rows(p1, p2, l2, swap, alpha, beta, classes, len(angles))
    assert np.array_equal(src, want_src) and np.array_equal(op, want_op)
    got = ops.aug_apply_host(p1, p2, src, op, ops.aug_params(angles))
    cat = np.concatenate([p1, p2])[src]
    assert got.shape == (len(src), d) and np.array_equal(got[op == 0], cat[op == 0].astype(np.float32))
    assert np.array_equal(got[:, 2:], cat[:, 2:].astype(np.float32))
    for r, a in enumerate(angles):
        sel = op == r + 1
        x = cat[sel, 0] * np.cos(a) + cat[sel, 1] * (-np.sin(a))
        y = cat[sel, 0] * np.sin(a) + cat[sel, 1] * np.cos(a)
        assert np.array_equal(got[sel, 0], x.astype(np.float32)) and np.array_equal(got[sel, 1], y.astype(np.float32))


def test_polarmix_empty_sector_and_no_instances():
    p1, p2 = _rows(50, 6, 4), _rows(40, 6, 5)
    l2 = np.full(40, 255, np.uint8)
    pm = augment.PolarMix([0, 1, 2], [0.5, 1.5])
    src, op = pm.row_map(p1, p2, l2, True, 0.25, 0.25)  # an empty sector: frame 1 stays whole, nothing is pasted
    assert np.array_equal(src, np.arange(50)) and not op.any()
    src, op = pm.row_map(p1, p2, l2, True, -4.0, 4.0)  # every yaw inside: frame 2 replaces frame 1
    assert np.array_equal(src, 50 + np.arange(40))
    l2[7] = l2[3] = 1
    src, op = pm.row_map(p1, p2, l2.astype(np.int64), False, 0.0, 0.0)
    assert src.tolist() == list(range(50)) + [53, 57] * 3 and op.tolist() == [0] * 52 + [1, 1, 2, 2]
    assert len(augment.PolarMix([], [0.5]).row_map(p1, p2, l2, False, 0.0, 0.0)[0]) == 50


def test_apply_empty_frame():
    aug = augment.TrainAugmentation(aug_ref.ROT_RANGE, aug_ref.SCALE_RANGE, 0.5, 0.95, 50.0, rng="numpy")
    out = aug.apply(np.zeros((0, 6)), np.zeros(0, np.uint8), np.zeros((0, 4), np.float32), seed=1)
    assert out["points"].shape == (0, 6) and out["point_labels"].shape == (0,)
    assert out["point_image_features"].shape == (0, 4)
    aug = augment.TrainAugmentation(aug_ref.ROT_RANGE, aug_ref.SCALE_RANGE, 0.5, 0.95, 50.0,
                                    polar_mix=augment.PolarMix([1], [0.5]), rng="device")
    out = aug.apply(np.zeros((0, 6)), np.zeros(0, np.uint8), None, np.zeros((0, 6)), np.zeros(0, np.uint8), seed=1)
    assert out["points"].shape == (0, 6) and out["point_image_features"] is None


def test_bad_arguments_raise():
    p = _rows(8, 6, 1)
    lab = np.zeros(8, np.uint8)
    pm = augment.PolarMix([0], [0.5])
    with pytest.raises(Seg3dError):
        pm.row_map(p.astype(np.float16), p.astype(np.float16), lab, False, 0, 0)
    with pytest.raises(Seg3dError):
        pm.row_map(p, p.astype(np.float32), lab, False, 0, 0)  # both frames of one dtype
    with pytest.raises(Seg3dError):
        pm.row_map(p, p, lab.astype(np.int32), False, 0, 0)
    with pytest.raises(Seg3dError):
        pm.row_map(_rows(8, 17, 1), _rows(8, 17, 1), lab, False, 0, 0)
    with pytest.raises(Seg3dError):
        ops.aug_apply_host(_rows(8, 2, 1), None, None, None, ops.aug_params())
    with pytest.raises(Seg3dError):
        augment.PolarMix([0, 0], [0.5]).row_map(p, p, lab, False, 0, 0)
    with pytest.raises(Seg3dError):
        augment.PolarMix([0], [0.1] * 9)
    with pytest.raises(Seg3dError):
        make_aug(case("sweeps")).apply(_rows(8, 17, 1), lab, seed=0)
    with pytest.raises(Seg3dError):
        ops.aug_gather_host(lab, None, np.zeros(3, np.int64))
    aug = augment.TrainAugmentation(aug_ref.ROT_RANGE, aug_ref.SCALE_RANGE, 0.5, 0.95, 50.0)
    with pytest.raises(Seg3dError):
        aug.apply(p.tolist(), lab)
