"""GPU checks of the instance copy-paste augmentation (csrc/augment_instance.hip): the device entry against its host
twin bit for bit and against the reference's recorded outputs (tests/golden/instaug.npz) with the tolerance of
test_instaug_host.py, the sequential dependence and the tie-break across workgroups, a frame large enough that every
thread strides more than once, and InstanceAugmentation / TrainAugmentation on CUDA tensors.

float32 frames: only ground_z is read from the frame, so x, y keep the 1e-9 m bound and z gets the rounding of one
float32 below 2 m on top of it (half a spacing, 2^-24 m); the fixture's generator asserts that the rounding changes no
decision."""
import numpy as np
import pytest
import torch

import instaug_ref as ir
from instaug_ref import XYZ_TOL, case, case_items, check_golden, draw_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [np.float64, np.float32]


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ia(bank=None, **kw):
    from openseg3d_amd import augment
    return augment.InstanceAugmentation(augment.InstanceBank(ir.golden_bank() if bank is None else bank), **kw)


def _both(points, labels, ia, items, ground_ids=ir.GROUND_IDS):
    """(device result as numpy, host result) of the two ops entries on the same inputs; asserts they are identical."""
    from openseg3d_amd import ops
    plans = ia.plans(draw_of(items))
    want = ops.aug_instance_paste_host(points, labels, ground_ids, ia.bank.rows, plans)
    got = ops.aug_instance_paste(_t(points), _t(labels), ground_ids, ia.bank.rows_on(DEV), plans)
    assert got[0].is_cuda and got[0].dtype == torch.float64 and got[1].is_cuda
    got = (got[0].cpu().numpy(), got[1].cpu().numpy(), got[2])
    assert got[2] == want[2], (got[2], want[2])
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])  # bit for bit
    assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1])
    return got, want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ir.CASES)
def test_device_equals_host_twin_and_the_reference(name, dtype):
    c = case(name)
    frame = c.points.astype(dtype)
    (add_p, add_l, dec), _ = _both(frame, c.labels, _ia(), case_items(c))
    z_tol = XYZ_TOL if dtype == np.float64 else XYZ_TOL + 2.0 ** -24
    check_golden(c, np.concatenate([c.points, add_p]), np.concatenate([c.labels, add_l]), dec, z_tol=z_tol,
                 what=f"{name} {np.dtype(dtype).name}")
    _both(frame, c.labels.astype(np.int64), _ia(), case_items(c))


@pytest.mark.parametrize("angles_from", ["recorded", "one_place"])
def test_later_instances_see_earlier_pasted_rows(angles_from):
    c = case("feats")
    items = case_items(c)
    it = dict(items[int(np.argmax(c.decisions >= 0))], loc_noise=None, rot_noise=None, flip_type=None)
    alone = ir.np_instance_paste(c.points, c.labels, ir.golden_bank(), [it])[2][0]
    if angles_from == "one_place":
        it["angles"] = np.full(3, it["angles"][alone])
        alone = 0
    (add_p, _, dec), _ = _both(c.points, c.labels, _ia(), [it, dict(it)])
    want_p, _, want_dec, _ = ir.np_instance_paste(c.points, c.labels, ir.golden_bank(), [it, dict(it)])
    assert dec == want_dec and dec[0] == alone and dec[1] != alone
    assert (dec[1] == -1) if angles_from == "one_place" else (dec[1] > alone or dec[1] == -1)
    assert np.abs(add_p - want_p[len(c.points):]).max() <= XYZ_TOL


@pytest.mark.parametrize("low_first", [True, False])
def test_equal_ground_distances_keep_the_lower_row_across_workgroups(low_first):
    n = 1003  # four workgroups of 256 rows: row 3 in the first, row n - 5 in the last; no multiple of 64
    pts, labels, bank, items, ground_z = ir.tie_case(n, low_first)
    for dtype in DTYPES:
        frame = pts.astype(dtype)
        assert frame[3, 1] == -frame[n - 5, 1] and frame[3, 2] == -frame[n - 5, 2]  # still mirrored after rounding
        (add_p, add_l, dec), _ = _both(frame, labels, _ia(bank, instance_label_ids=[4]), items)
        assert dec == [0] and add_l.tolist() == [4, 4]
        want = bank[4][0]["cluster_points"][:, :3] + [0.0, 0.0, float(dtype(ground_z)) + 0.25]
        assert np.array_equal(add_p[:, :3], want)


@pytest.mark.parametrize("rows,n_angles", [(1, 20), (256, 20), (257, 7), (700, 20)])
def test_cluster_sizes_around_the_workgroup(rows, n_angles):
    """Clusters of fewer, exactly and more rows than the 256 threads of the one-workgroup steps (prepare and paste
    stride then), and fewer candidates than the kernels unroll for; against the host twin and the restatement."""
    c = case("plain")
    rs = np.random.RandomState(rows)
    base = ir.golden_bank()[4][0]["cluster_points"]
    pts = base[rs.randint(0, len(base), rows)] + rs.randn(rows, 6) * ([0.05] * 3 + [0.0] * 3) * (rows > 1)
    bank = {4: [{"cluster_points": pts, "cluster_height": 0.6}]}
    items = [{"label": 4, "index": 0, "loc_noise": np.array([0.2, -0.1, 0.05]), "rot_noise": 0.1, "flip_type": 3,
              "angles": rs.random(n_angles) * np.pi * 2} for _ in range(2)]
    (add_p, _, dec), _ = _both(c.points, c.labels, _ia(bank, instance_label_ids=[4]), items)
    want_p, _, want_dec, _ = ir.np_instance_paste(c.points, c.labels, bank, items)
    assert dec == want_dec and (rows == 1 or max(dec) >= 0)  # a single point has radius 0: never on the ground
    assert np.abs(add_p - want_p[len(c.points):]).max() <= XYZ_TOL if len(add_p) else want_p.shape[0] == len(c.points)


def test_large_frame_every_thread_strides():
    """65 537 rows: more than the capped grid's 65 536 threads, so the partial-record list is full and threads stride.
    The small scene tiled on a 70 m grid (the tiles do not touch); checked against the host twin."""
    c = case("ground")
    n, m = 65537, len(c.points)
    reps = -(-n // m)
    tiles, labels = [], []
    for i in range(reps):
        p = c.points.copy()
        p[:, 0] += 70.0 * (i % 7)
        p[:, 1] += 70.0 * (i // 7)
        tiles.append(p)
        labels.append(c.labels)
    frame, labels = np.concatenate(tiles)[:n], np.concatenate(labels)[:n]
    for dtype in DTYPES:
        (add_p, _, dec), _ = _both(frame.astype(dtype), labels, _ia(), case_items(c))
        assert max(dec) >= 0 and len(add_p) > 0
    assert dec == c.decisions.tolist()  # tile 0 is the recorded scene, the others are out of reach


@pytest.mark.parametrize("label_dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("with_feats", [True, False])
def test_call_on_cuda_tensors_equals_the_numpy_path(label_dtype, with_feats):
    c = case("feats")
    ia = _ia()
    draw = draw_of(case_items(c))
    feats = c.feats if with_feats else None
    labels = c.labels.astype(label_dtype)
    want = ia(c.points, feats, labels, draw=draw)
    want_dec = ia.last_decisions
    got = ia(_t(c.points), _t(feats), _t(labels), draw=draw)
    again = ia(_t(c.points), _t(feats), _t(labels), draw=draw)
    assert len(got) == len(want) == (3 if with_feats else 2) and ia.last_decisions == want_dec
    for g, a, w in zip(got, again, want):
        assert g.is_cuda and g.cpu().numpy().dtype == w.dtype
        assert np.array_equal(g.cpu().numpy(), w) and torch.equal(g, a)  # the numpy path's bits, twice


def test_train_augmentation_on_the_device_equals_the_host():
    from openseg3d_amd import augment
    import aug_ref
    c, c2 = case("feats"), case("ground")
    ia = _ia()
    aug = augment.TrainAugmentation(aug_ref.ROT_RANGE, aug_ref.SCALE_RANGE, 0.5, 0.95, 20.0,
                                    polar_mix=augment.PolarMix(list(range(13)), [0.7, 2.9]), rng="device", instance_bank=ia)
    for dtype in DTYPES:
        f1, f2 = c.points.astype(dtype), c2.points.astype(dtype)
        want = aug.apply(f1, c.labels, c.feats, f2, c2.labels, c2.feats, seed=9)
        got = aug.apply(_t(f1), _t(c.labels), _t(c.feats), _t(f2), _t(c2.labels), _t(c2.feats), seed=9)
        for k in ("points", "point_labels", "point_image_features", "source_rows"):
            assert got[k].is_cuda and np.array_equal(got[k].cpu().numpy(), want[k]), k
        assert (want["source_rows"] < 0).any() and got["instance_draw"].label == want["instance_draw"].label
