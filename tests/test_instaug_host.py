"""CPU checks of the instance copy-paste augmentation (openseg3d_amd/augment.py: InstanceBank, InstanceAugmentation; the
host entry of csrc/augment_instance.hip) against the reference's InstanceAugmentation as recorded in
tests/golden/instaug.npz (tests/golden/make_golden_instaug.py) and against the numpy restatement of tests/instaug_ref.py.

Tolerances.  Decisions, row counts, labels, the feature columns of pasted rows (tanh is numpy's, applied when the bank is
packed), the image-feature zeros and the frame's own rows are compared for equality.  x, y, z of pasted rows are allowed
1e-9 m against the reference's float64: coordinates are below 64 m, where float64 spacing is 1.4e-14, and the chain is
well under 100 roundings, so honest differences (the summation order of the two means, the reference's BLAS 2 x 2
product) stay below 2e-12, while any real mistake (an axis, the sign of an angle, the z adjustment, the flip centre) is
1e-3 or more."""
import numpy as np
import pytest

import aug_ref
import instaug_ref as ir
from instaug_ref import XYZ_TOL, case, case_items, check_golden, draw_of, np_instance_paste

from openseg3d_amd import augment, ops  # noqa: E402
from openseg3d_amd._lib import Seg3dError  # noqa: E402

def make_ia(bank=None, **kw):
    return augment.InstanceAugmentation(augment.InstanceBank(ir.golden_bank() if bank is None else bank), **kw)


# ------------------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("local,flip", [(True, True), (False, True), (True, False), (False, False)])
def test_draw_order(seed, local, flip):
    ia = make_ia(local_transformation=local, random_flip=flip)
    a, b = np.random.RandomState(seed), np.random.RandomState(seed)
    d = ia.draw(a)
    want = ir.replay_draws(b, ir.golden_bank(), local=local, flip=flip)
    assert len(d) == len(want) == 5
    for i, it in enumerate(want):
        assert (d.label[i], d.index[i], d.flip_type[i]) == (it["label"], it["index"], it["flip_type"])
        assert np.array_equal(d.angles[i], it["angles"]) and len(d.angles[i]) == 20
        if local:
            assert np.array_equal(d.loc_noise[i], it["loc_noise"]) and d.rot_noise[i] == it["rot_noise"]
        else:
            assert d.loc_noise[i] is None and d.rot_noise[i] is None
    assert a.random() == b.random()  # every draw consumed, placed or not


@pytest.mark.parametrize("name", ir.CASES)
def test_draw_from_the_recorded_seed(name):
    c = case(name)
    rs = np.random.RandomState(int(c.seed))
    d = make_ia().draw(rs)
    assert d.label == c.draw_label.tolist() and d.index == c.draw_index.tolist() and d.flip_type == c.draw_flip.tolist()
    assert np.array_equal(np.array(d.loc_noise), c.draw_loc) and np.array_equal(np.array(d.rot_noise), c.draw_rot)
    assert np.array_equal(np.array(d.angles), c.draw_angles) and rs.random() == float(c.next_draw)


# ------------------------------------------------------------------------------------------------ the golden cases
@pytest.mark.parametrize("name", ir.CASES)
def test_golden_case(name):
    c = case(name)
    ia = make_ia()
    res = ia(c.points, c.feats, c.labels, draw=draw_of(case_items(c)))
    assert len(res) == (2 if c.feats is None else 3)
    points, labels = res[0], res[-1]
    assert np.array_equal(points[:len(c.points)], c.points)  # bit for bit
    check_golden(c, points, labels, ia.last_decisions, res[1] if c.feats is not None else None, what=name)
    # what the fixture was chosen for
    if name == "feats":
        assert max(ia.last_decisions) > 0 and any(f == 3 and d >= 0 for f, d in zip(c.draw_flip, ia.last_decisions))
    if name == "plain":
        assert -1 in ia.last_decisions
    # drawing from the global generator, as the reference does
    np.random.seed(int(c.seed))
    again = ia(c.points, c.feats, c.labels)
    assert np.array_equal(again[0], points) and np.array_equal(again[-1], labels)
    # int64 labels: the added labels follow the labels' width
    res64 = ia(c.points, None, c.labels.astype(np.int64), draw=draw_of(case_items(c)))
    assert res64[1].dtype == np.int64 and np.array_equal(res64[1], labels) and np.array_equal(res64[0], points)


@pytest.mark.parametrize("name", ir.CASES)
def test_ops_host_entry_against_the_restatement(name):
    """The same through ops, on the float32-rounded frame as well: decisions equal, xyz within the tolerance."""
    c = case(name)
    ia = make_ia()
    plans = ia.plans(draw_of(case_items(c)))
    for dt in (np.float64, np.float32):
        frame = c.points.astype(dt)
        add_p, add_l, dec = ops.aug_instance_paste_host(frame, c.labels, ir.GROUND_IDS, ia.bank.rows, plans)
        want_p, want_l, want_dec, _ = np_instance_paste(frame, c.labels, ir.golden_bank(), case_items(c))
        n = len(frame)
        assert dec == want_dec == c.decisions.tolist() and np.array_equal(add_l, want_l[n:]) and add_l.dtype == np.uint8
        assert add_p.dtype == np.float64 and add_p.shape == want_p[n:].shape
        assert np.abs(add_p - want_p[n:]).max() <= XYZ_TOL and np.array_equal(add_p[:, 3:], want_p[n:, 3:])


# ------------------------------------------------------------------------------------------------ by construction
@pytest.mark.parametrize("angles_from", ["recorded", "one_place"])
def test_later_instances_see_earlier_pasted_rows(angles_from):
    c = case("feats")
    items = case_items(c)
    k = int(np.argmax(c.decisions >= 0))
    it = dict(items[k], loc_noise=None, rot_noise=None, flip_type=None)
    alone = np_instance_paste(c.points, c.labels, ir.golden_bank(), [it])[2][0]
    assert alone >= 0
    if angles_from == "one_place":  # every candidate is the place the first instance takes
        it["angles"] = np.full(3, it["angles"][alone])
        alone = 0
    twice = [it, dict(it)]
    ia = make_ia()
    points, labels = ia(c.points, None, c.labels, draw=draw_of(twice))
    want_p, want_l, want_dec, info = np_instance_paste(c.points, c.labels, ir.golden_bank(), twice)
    first, second = ia.last_decisions
    assert ia.last_decisions == want_dec and first == alone
    # the second copy finds the first one's rows around the candidate centre the first took (they only moved in z)
    assert info[0]["obj"][alone] > info[0]["radius"] > 0.5 * info[0]["radius"] > info[1]["obj"][alone] and second != first
    assert (second == -1) if angles_from == "one_place" else (second > first or second == -1)
    assert points.shape == want_p.shape and np.array_equal(labels, want_l)
    assert np.abs(points - want_p).max() <= XYZ_TOL


@pytest.mark.parametrize("low_first", [True, False])
@pytest.mark.parametrize("n", [700, 1003])
def test_equal_ground_distances_keep_the_lower_row(n, low_first):
    pts, labels, bank, items, ground_z = ir.tie_case(n, low_first)
    c = np.array([10.0, 0.0, 0.0])
    d = np.linalg.norm(pts[:, :3] - c, axis=1)
    assert d[3] == d[n - 5] == np.sort(d)[0] and pts[3, 2] != pts[n - 5, 2]  # a true tie, and it matters
    ia = make_ia(bank, instance_label_ids=[4])
    points, out_labels = ia(pts, None, labels, draw=draw_of(items))
    assert ia.last_decisions == [0] and len(points) == n + 2
    want = bank[4][0]["cluster_points"][:, :3] + [0.0, 0.0, ground_z + 0.25]
    assert np.array_equal(points[n:, :3], want) and out_labels[n:].tolist() == [4, 4]
    want_p = np_instance_paste(pts, labels, bank, items)[0]
    assert np.array_equal(points[:, :3], want_p[:, :3])


# ------------------------------------------------------------------------------------------------ edge cases
def test_edge_cases():
    c = case("plain")
    ia = make_ia()
    draw = draw_of(case_items(c))
    n = len(c.points)
    ground = np.isin(c.labels, ir.GROUND_IDS)
    # no ground row: nothing can be placed
    lab = np.where(ground, 5, c.labels).astype(np.uint8)
    points, labels = ia(c.points, None, lab, draw=draw)
    assert ia.last_decisions == [-1] * 5 and np.array_equal(points, c.points) and np.array_equal(labels, lab)
    # no object row: nothing occludes
    lab = np.where(ground, c.labels, 255).astype(np.uint8)
    points, labels = ia(c.points, None, lab, draw=draw)
    want_p, want_l, want_dec, _ = np_instance_paste(c.points, lab, ir.golden_bank(), case_items(c))
    assert ia.last_decisions == want_dec and max(want_dec) >= 0 and len(points) > n
    assert np.abs(points - want_p).max() <= XYZ_TOL and np.array_equal(labels, want_l)
    # every label 255
    lab = np.full(n, 255, np.uint8)
    points, feats, labels = ia(c.points, np.ones((n, 3), np.float32), lab, draw=draw)
    assert ia.last_decisions == [-1] * 5 and np.array_equal(points, c.points) and feats.shape == (n, 3)
    # nothing to add
    none = make_ia(add_count=0)
    d = none.draw(np.random.RandomState(0))
    assert len(d) == 0
    points, labels = none(c.points.astype(np.float32), None, c.labels, draw=d)
    assert none.last_decisions == [] and points.dtype == np.float64 and np.array_equal(points, c.points.astype(np.float32))
    # an empty frame
    points, labels = ia(np.zeros((0, 6)), None, np.zeros(0, np.uint8), draw=draw)
    assert points.shape == (0, 6) and ia.last_decisions == [-1] * 5


def test_bad_arguments_raise():
    c = case("plain")
    ia = make_ia()
    with pytest.raises(Seg3dError):
        ia(c.points[:, :5], None, c.labels)  # the bank has 6 columns
    with pytest.raises(Seg3dError):
        make_ia(random_rotate=False)
    bad = ir.golden_bank()
    bad[3][1]["cluster_points"] = bad[3][1]["cluster_points"][:, :5]
    with pytest.raises(Seg3dError):
        augment.InstanceBank(bad)
    plans = ia.plans(draw_of(case_items(c)))
    need = sum(p.n_rows for p in plans)
    ops.aug_instance_paste_host(c.points, c.labels, ir.GROUND_IDS, ia.bank.rows, plans, cap_add=need)
    with pytest.raises(Seg3dError, match="SEG3D_EINVAL"):
        ops.aug_instance_paste_host(c.points, c.labels, ir.GROUND_IDS, ia.bank.rows, plans, cap_add=need - 1)
    with pytest.raises(Seg3dError):
        ops.aug_instance_paste_host(c.points, c.labels, ir.GROUND_IDS, ia.bank.rows[:, :5], plans)
    with pytest.raises(Seg3dError):
        ops.aug_instance_plan(0, 5, 3, 0.5, angles=np.zeros(21))
    with pytest.raises(Seg3dError):
        ia(c.points, None, c.labels, draw=augment.InstanceDraw(label=[3], index=[99], angles=[np.zeros(2)]))


def test_bank_from_pickle(tmp_path):
    import pickle
    path = tmp_path / "bank.pkl"
    with open(path, "wb") as f:
        pickle.dump(ir.golden_bank(), f)
    a, b = augment.InstanceAugmentation(str(path)).bank, augment.InstanceBank(ir.golden_bank())
    assert np.array_equal(a.rows, b.rows) and a.entries == b.entries and a.dim == 6
    raw = case("bank").rows
    assert not a.rows[:, 3].any() and np.array_equal(a.rows[:, 4], np.tanh(raw[:, 4])) and np.array_equal(a.rows[:, 5], raw[:, 5])


# ------------------------------------------------------------------------------------------------ TrainAugmentation
PASTE = [0.7, 2.9]
CLASSES = list(range(13))


def _train_aug(bank):
    return augment.TrainAugmentation(aug_ref.ROT_RANGE, aug_ref.SCALE_RANGE, 0.5, 1.0, 20.0,
                                     polar_mix=augment.PolarMix(CLASSES, PASTE), rng="numpy", instance_bank=bank)


def test_train_augmentation_pastes_before_polarmix():
    c, c2 = case("feats"), case("ground")
    ia = make_ia()
    idraw = draw_of(case_items(c))
    p1, f1, l1 = ia(c.points, c.feats, c.labels, draw=idraw)
    n0, n_added = len(c.points), len(p1) - len(c.points)
    assert n_added > 0
    # a sector that takes about half of the pasted rows
    yaw = -np.arctan2(p1[n0:, 1], p1[n0:, 0])
    alpha = float(np.median(yaw)) + 1e-4
    pm = augment.PolarMix(CLASSES, PASTE)
    src, _ = pm.row_map(p1, c2.points, c2.labels, True, alpha, alpha + np.pi)
    n = len(src)
    rs = np.random.RandomState(3)
    draw = augment.AugDraw(swap=True, alpha=alpha, beta=alpha + np.pi, rot=0.3, scale=1.02, offsets=[0.1, -0.2, 0.05],
                           flip_x=True, flip_y=False, perm=rs.permutation(n), choices=rs.permutation(n), instance_draw=idraw)
    out = _train_aug(ia).apply(c.points, c.labels, c.feats, c2.points, c2.labels, c2.feats, params=draw)
    # the PolarMix stage saw n1 = n0 + n_added rows: the same as running the two stages by hand
    draw.instance_draw = None
    want = _train_aug(None).apply(p1, l1, f1, c2.points, c2.labels, c2.feats, params=draw)
    for k in ("points", "point_labels", "point_image_features"):
        assert np.array_equal(out[k], want[k]), k
    assert len(out["points"]) == n and out["instance_draw"] is idraw and want["instance_draw"] is None
    # source rows: frame 1 as it came, frame 2 behind it, pasted rows as -1 - bank_row
    rows, wrows = out["source_rows"], want["source_rows"]
    pasted = (wrows >= n0) & (wrows < n0 + n_added)
    assert np.array_equal(rows[wrows < n0], wrows[wrows < n0])
    assert np.array_equal(rows[wrows >= n0 + n_added], wrows[wrows >= n0 + n_added] - n_added)
    assert np.array_equal(rows[pasted], -1 - ia.last_bank_rows[wrows[pasted] - n0]) and (rows[pasted] < 0).all()
    assert np.array_equal(out["points"][pasted, 3:], ia.bank.rows[-1 - rows[pasted], 3:].astype(np.float32))
    assert (out["point_labels"][pasted] == np.array(idraw.label)[:, None]).any(axis=0).all()
    assert not out["point_image_features"][pasted].any()
    # pasted rows inside the swap sector are dropped like any other row of frame 1
    inside = (yaw > alpha) & (yaw < alpha + np.pi)
    assert 0 < inside.sum() < n_added and np.array_equal(np.sort(wrows[pasted] - n0), np.where(~inside)[0])
    # drawn from a seed: the instance draws come first
    out = _train_aug(ia).apply(c.points, c.labels, c.feats, c2.points, c2.labels, c2.feats, seed=5)
    first = ia.draw(np.random.RandomState(5))
    assert out["instance_draw"].label == first.label and np.array_equal(out["instance_draw"].angles, first.angles)
    assert out["draw"].instance_draw is out["instance_draw"]


@pytest.mark.parametrize("name", aug_ref.CASES)
def test_train_augmentation_without_a_bank_is_unchanged(name):
    """apply() without a bank against the stages composed by hand from the entries it has always used."""
    c = aug_ref.case(name)
    aug = aug_ref.make_aug(c)
    assert aug.instance_aug is None
    d = aug_ref.recorded_draw(c)
    f2 = {} if c.multi else dict(frame2=c.points2, labels2=c.labels2, image_features2=c.feats2)
    cur = dict(cur_point_indices=c.cur_point_indices) if c.multi else {}
    out = aug.apply(c.points1, c.labels1, c.feats1, **f2, **cur, params=d)
    assert out["instance_draw"] is None
    perm, choices = c.perm.astype(np.int32), c.choices.astype(np.int32)
    idx = ops.aug_gather_host(perm, None, choices)
    if c.multi:
        src2, op2, p2 = idx, None, None
        pos, gat = ops.aug_cur_map_host(src2, c.cur_point_indices.astype(np.int32), len(c.points1))
        assert np.array_equal(out["cur_point_indices"], pos)
        want_l, want_f = ops.aug_gather_host(c.labels1, None, gat), ops.aug_gather_host(c.feats1, None, gat)
    else:
        src, op = aug.polar_mix.row_map(c.points1, c.points2, c.labels2, bool(c.swap), float(c.alpha), float(c.beta))
        src2, op2, p2 = ops.aug_gather_host(src, None, idx), ops.aug_gather_host(op, None, idx), c.points2
        want_l, want_f = ops.aug_gather_host(c.labels1, c.labels2, src2), ops.aug_gather_host(c.feats1, c.feats2, src2)
    want_p = ops.aug_apply_host(c.points1, p2, src2, op2, aug._params(d, None))
    assert np.array_equal(out["points"], want_p) and np.array_equal(out["point_labels"], want_l)
    assert np.array_equal(out["point_image_features"], want_f) and np.array_equal(out["source_rows"], src2)
