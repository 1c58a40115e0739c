"""CPU checks of the instance bank extraction (csrc/instance_extract.hip, host twin; augment.InstanceBankBuilder):
the host entry against the numpy restatement of tools/extract_instances.py:46-76 (tests/instbank_ref.py) and against
sklearn's recorded ``labels_`` and the reference's recorded radii (tests/golden/instbank.npz) on the fixture clouds, the
restatement against sklearn itself where sklearn is installed, argument validation, and the builder's round trip through
the reference's pickle into ``InstanceAugmentation``.

Every fixture is on the 1/64 lattice with eps = 0.25, so cluster ids, rows and counts are compared exactly.  Doubles are
compared within 1e-9: both sides work in double on fewer than 2 000 rows at |coord| <= 100, whose summation error is
below 1e-11; only the summation order differs."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import instbank_ref as ir
from instbank_ref import CASES, DTYPES, LABEL_DTYPES, TOL, bank_frames, check_against_ref, check_builder_instances, host, ref_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instbank.npz")


@pytest.mark.parametrize("label_dtype", LABEL_DTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_restatement(name, dtype, label_dtype):
    check_against_ref(host(CASES[name], dtype, label_dtype), ref_of(name))


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_sklearn_and_the_reference_radius_as_recorded(name):
    g = np.load(GOLDEN)
    c = CASES[name]
    assert np.array_equal(g[f"{name}_check"], [len(c["points"]), (c["points"] * np.arange(1, len(c["points"]) + 1)[:, None]).sum()])
    pc, _, table, _ = host(c)
    first = 0
    for t, mp in zip(c["target_ids"], c["min_points"]):
        rows = np.nonzero(c["labels"] == t)[0]
        mine = [h for h in table if h["label"] == t]
        if f"{name}_{t}_ids" not in g.files:
            assert len(rows) < mp and not mine and (pc[rows] == -1).all()
            continue
        ids = g[f"{name}_{t}_ids"].astype(np.int64)
        assert np.array_equal(np.where(pc[rows] >= 0, pc[rows] - first, -1), ids)
        assert len(mine) == ids.max() + 1 == len(g[f"{name}_{t}_radius"])
        for h, center, radius in zip(mine, g[f"{name}_{t}_center"], g[f"{name}_{t}_radius"]):
            assert np.abs(h["center"] - center).max() <= TOL and abs(h["radius"] - radius) <= TOL
        first += len(mine)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_sklearn(name):
    cluster = pytest.importorskip("sklearn.cluster")
    c = CASES[name]
    for t, mp in zip(c["target_ids"], c["min_points"]):
        xy = c["points"][c["labels"] == t][:, :2]
        if len(xy) < mp:
            continue
        for dtype in DTYPES:
            want = cluster.DBSCAN(eps=c["eps"], min_samples=mp).fit(xy.astype(dtype)).labels_
            assert np.array_equal(ir.dbscan_ref(xy, c["eps"], mp), want), (t, dtype)


def test_what_the_fixtures_are_for():
    """The properties the clouds were built to show, read off the restatement (which sklearn confirms above)."""
    for name in ("empty_no_target", "empty_below_min", "empty_one_row"):
        assert ref_of(name)[3][:3] == [0, 0, 0] and (ref_of(name)[0] == -1).all()
    assert ref_of("empty_no_ground")[3] == [1, 0, 10, 10]
    pc, _, table, counts = ref_of("threshold")
    lab = CASES["threshold"]["labels"]
    assert sorted(len(c["rows"]) for c in table if c["label"] == 3) == [5] and (pc[lab == 3] == -1).sum() == 4
    assert sum(c["label"] == 4 for c in table) == 3 and (pc[lab == 4] >= 0).all()  # min_points 1: (9, 9.25) joined, two alone
    pc = ref_of("boundary")[0]  # per base: joined, apart, joined, apart
    assert (pc[:24].reshape(3, 4, 2) >= 0).all(2).tolist() == [[True, False, True, False]] * 3
    assert (pc[:24].reshape(12, 2)[::2, 0] == pc[:24].reshape(12, 2)[::2, 1]).all()
    for name, owner in (("contested_a_first", 0), ("contested_b_first", 0)):
        pc, _, table, _ = ref_of(name)
        x = CASES[name]["x_row"]
        assert pc[x] == owner == pc[0] and len(table) == 2 and len(table[0]["rows"]) == 9
    # the same cloud: X sits with blob A (one core neighbour, farther) when A is numbered first, with B otherwise
    assert np.array_equal(CASES["contested_a_first"]["points"][8, :3], CASES["contested_b_first"]["points"][8, :3])
    pc, _, table, counts = ref_of("snake")
    assert counts[0] == 3 and max(len(c["rows"]) for c in table) == 673
    order = [c["rows"].min() for c in table]
    assert order == sorted(order)  # numbered by the lowest row: every row of these clusters is a core
    side = ir.EPS
    cells = {tuple(v) for v in np.floor(CASES["snake"]["points"][table[np.argmax([len(c["rows"]) for c in table])]["rows"], :2]
                                        / side).astype(int).tolist()}
    assert len(cells) >= 300
    pc, _, table, counts = ref_of("labels")
    assert [c["label"] for c in table] == [4, 4, 10, 3] and counts[3] == 27
    assert sorted(len(c["rows"]) for c in ref_of("sizes")[2]) == [63, 64, 65, 255, 256, 257, 1025]
    table = ref_of("ground")[2]
    assert [c["kept"] for c in table] == [1, 0, 1] and [c["height"] for c in table] == [0.25, 0.0, -0.125]
    r = np.sqrt(3) / 8
    assert 1.2 * r - 0.25 >= 1e-3 and 17 / 64 - 1.2 * r >= 1e-3


def test_cap_smaller_than_the_clusters_found():
    from openseg3d_amd import _lib, ops
    c = CASES["sizes"]
    full = host(c)
    cap, guard = 3, 5
    pts, lab = np.ascontiguousarray(c["points"]), c["labels"].astype(np.uint8)
    n = len(pts)
    pc = np.full(n + guard, -77, np.int32)
    cr = np.full(n + guard, -77, np.int32)
    table = np.full((cap + guard) * 7, -1.5)
    counts = np.full(4 + guard, -77, np.int32)
    tids, mins, gids = (ctypes.c_uint8 * 3)(*c["target_ids"]), (ctypes.c_int32 * 3)(*c["min_points"]), (ctypes.c_uint8 * 5)(*c["ground_ids"])
    _lib.call("seg3d_instance_extract_host", pts.ctypes.data, n, 6, 8, lab.ctypes.data, 1, tids, mins, 3, gids, 5, 0.25, cap,
              pc.ctypes.data, cr.ctypes.data, table.ctypes.data, counts.ctypes.data)
    assert (pc[n:] == -77).all() and (cr[n:] == -77).all() and (counts[4:] == -77).all() and (table[cap * 7:] == -1.5).all()
    assert counts[0] == full[3][0] == 7 and counts[2] == full[3][2] and counts[3] == full[3][3]
    assert counts[1] == sum(int(k) for k in full[2]["kept"][:cap])
    assert np.array_equal(pc[:n], full[0]) and np.array_equal(cr[:n], full[1])
    assert table[:cap * 7].tobytes() == full[2][:cap].tobytes()
    assert ops.instance_extract_host(pts, lab, c["target_ids"], c["min_points"], c["ground_ids"], cap_clusters=cap)[2].tobytes() \
        == full[2][:cap].tobytes()
    old = ops.INSTANCE_EXTRACT_CAP
    try:  # the wrapper's own guess too small: one more run with the true number
        ops.INSTANCE_EXTRACT_CAP = 2
        again = host(c)
    finally:
        ops.INSTANCE_EXTRACT_CAP = old
    assert again[3] == full[3] and again[2].tobytes() == full[2].tobytes()


def test_argument_validation():
    from openseg3d_amd import _lib, ops
    lib = _lib.load()
    pts, lab = np.zeros((4, 6)), np.zeros(4, np.uint8)
    pc, cr, counts = np.zeros(4, np.int32), np.zeros(4, np.int32), np.full(4, -7, np.int32)
    table = np.zeros(8 * 7)

    def call(n=4, dim=6, pb=8, lb=1, tids=(3,), mins=(2,), gids=(17,), eps=0.25, cap=8, k=None, g=None, points=pts, cnt=counts):
        return lib.seg3d_instance_extract_host(points.ctypes.data if points is not None else None, n, dim, pb, lab.ctypes.data, lb,
                                               (ctypes.c_uint8 * 16)(*tids), (ctypes.c_int32 * 16)(*mins),
                                               len(tids) if k is None else k, (ctypes.c_uint8 * 16)(*gids),
                                               len(gids) if g is None else g, eps, cap, pc.ctypes.data, cr.ctypes.data,
                                               table.ctypes.data, cnt.ctypes.data if cnt is not None else None)

    assert call() == 0 and counts.tolist() == [0, 0, 0, 0]
    counts[:] = -7
    for kw in (dict(n=-1), dict(dim=2), dict(dim=17), dict(pb=2), dict(lb=4), dict(k=0), dict(k=9), dict(g=0), dict(g=9),
               dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(mins=(0,)), dict(tids=(3, 3), mins=(2, 2)),
               dict(cap=-1), dict(points=None), dict(cnt=None), dict(n=2 ** 31 - 1)):
        assert call(**kw) == _lib.EINVAL, kw
    assert counts.tolist() == [-7] * 4  # a refused call writes nothing
    assert _lib.query("seg3d_instance_extract_workspace_bytes", -1, 8) == 0
    assert _lib.query("seg3d_instance_extract_workspace_bytes", 1000, 8) >= 1000 * 4 * (8 + 4)
    # the device entry refuses the same arguments, and a missing or short workspace, before anything is enqueued
    fake = ctypes.c_void_p(256)
    dev = lib.seg3d_instance_extract
    ids, one = (ctypes.c_uint8 * 1)(3), (ctypes.c_int32 * 1)(2)
    need = _lib.query("seg3d_instance_extract_workspace_bytes", 100, 8)
    assert dev(fake, 100, 6, 4, fake, 1, ids, one, 1, ids, 1, 0.25, 8, fake, fake, fake, fake, None, need, None) == _lib.EINVAL
    assert dev(fake, 100, 6, 4, fake, 1, ids, one, 1, ids, 1, 0.25, 8, fake, fake, fake, fake, fake, need - 1, None) == _lib.EWORKSPACE
    assert dev(fake, 100, 2, 4, fake, 1, ids, one, 1, ids, 1, 0.25, 8, fake, fake, fake, fake, fake, need, None) == _lib.EINVAL
    with pytest.raises(_lib.Seg3dError):
        ops.instance_extract_host(np.zeros((4, 6), np.int32), lab, [3], [2], [17])
    with pytest.raises(_lib.Seg3dError):
        ops.instance_extract_host(pts, np.zeros(3, np.uint8), [3], [2], [17])
    with pytest.raises(_lib.Seg3dError):
        ops.instance_extract_host(pts, lab, [3, 4], [2], [17])
    with pytest.raises(_lib.Seg3dError):
        ops.instance_extract(torch.zeros(4, 6), torch.zeros(4, dtype=torch.uint8), [3], [2], [17])  # no device, no fallback


@pytest.mark.parametrize("dtype", DTYPES)
def test_builder_round_trip(dtype, tmp_path):
    from openseg3d_amd import augment
    b = augment.InstanceBankBuilder(label_ids=[3, 4, 10], min_points={3: 6, 4: 6, 10: 6}, eps=0.25)
    added = [b.add(c["points"].astype(dtype), c["labels"].astype(np.uint8)) for c in bank_frames()]
    assert added == [2, 3] and b.frames == 2  # the dropped cluster of the ground fixture is skipped, its neighbours stay
    check_builder_instances(b.instances, dtype)
    path = str(tmp_path / "bank.pkl")
    b.save(path)
    with open(path, "rb") as f:
        loaded = pickle.load(f)
    assert type(loaded) is dict
    check_builder_instances(loaded, dtype)  # the reference indexes instances[label_id][idx]['cluster_points' / 'cluster_height']
    bank = b.bank()
    assert [len(bank.entries[k]) for k in (3, 4, 10)] == [5, 0, 0] and bank.dim == 6
    # this package's InstanceAugmentation pastes from the saved file
    ia = augment.InstanceAugmentation(path, instance_label_ids=[3], add_count=2)
    assert np.array_equal(ia.bank.rows, bank.rows)
    scene = CASES["sizes"]
    points, labels = ia(scene["points"], None, scene["labels"].astype(np.uint8), draw=ia.draw(np.random.RandomState(3)))
    assert len(ia.last_decisions) == 2 and len(points) == len(labels) >= len(scene["points"])
    assert np.array_equal(points[:len(scene["points"])], scene["points"])
    for label, min_points in ((3, {3: 5}), (4, [7])):  # min_points as a dict or in label order; a missing label is refused
        assert augment.InstanceBankBuilder([label], min_points).min_points == [5 if label == 3 else 7]
    with pytest.raises(augment.Seg3dError):
        augment.InstanceBankBuilder([3, 4], {3: 5})
