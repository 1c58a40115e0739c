"""Shared by test_instaug_host.py, test_gpu_instaug.py and tests/golden/make_golden_instaug.py: the fixture
tests/golden/instaug.npz (the reference's InstanceAugmentation on a synthetic scene and bank), a vectorised numpy
restatement of instance_augmentation.py:25-186 that takes the draws as arguments, the replay of the reference's draw
order on a RandomState, and small builders for hand-made frames."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "instaug.npz")
CASES = ("feats", "plain", "ground")
INSTANCE_IDS = [3, 4, 10]
GROUND_IDS = [17, 18, 19, 20, 21]
PER_LABEL = 4  # clusters per label in the fixture's bank
XYZ_TOL = 1e-9  # metres, pasted xyz against the reference's float64 (derived in test_instaug_host.py)
_cache = {}


class Case:
    def __init__(self, name, arrays):
        self.name = name
        self._a = arrays

    def __getattr__(self, key):
        return self._a.get(key)


def case(name):
    if not _cache:
        g = np.load(GOLDEN)
        for c in CASES:
            _cache[c] = Case(c, {k[len(c) + 1:]: g[k] for k in g.files if k.startswith(c + "_")})
        _cache["bank"] = Case("bank", {k[5:]: g[k] for k in g.files if k.startswith("bank_")})
    return _cache[name]


def bank_dict(rows, offsets, heights, labels):
    """The reference's dict from the packed arrays the fixture stores (arrays only)."""
    inst = {}
    for i, lab in enumerate(labels):
        inst.setdefault(int(lab), []).append({"cluster_points": rows[offsets[i]:offsets[i + 1]].copy(),
                                              "cluster_height": float(heights[i])})
    return inst


def golden_bank():
    b = case("bank")
    return bank_dict(b.rows, b.offsets, b.heights, b.labels)


def replay_draws(rs, bank, instance_ids=INSTANCE_IDS, add_count=5, local=True, flip=True):
    """instance_augmentation.py:26-30 and, per instance, :169, :171, :66, :77 on the RandomState ``rs``."""
    items = []
    label_choice = rs.choice(instance_ids, add_count, replace=True)
    uni_label, uni_count = np.unique(label_choice, return_counts=True)
    for label_id, count in zip(uni_label, uni_count):
        for idx in rs.choice(len(bank[label_id]), count):
            it = {"label": int(label_id), "index": int(idx), "loc_noise": None, "rot_noise": None, "flip_type": None}
            if local:
                it["loc_noise"] = rs.normal(scale=0.25, size=(1, 3))[0]
                it["rot_noise"] = rs.uniform(-np.pi / 20, np.pi / 20)
            if flip:
                it["flip_type"] = int(rs.choice(5, 1)[0])
            it["angles"] = rs.random(20) * np.pi * 2
            items.append(it)
    return items


def draw_of(items):
    from openseg3d_amd.augment import InstanceDraw
    return InstanceDraw(label=[it["label"] for it in items], index=[it["index"] for it in items],
                        loc_noise=[it["loc_noise"] for it in items], rot_noise=[it["rot_noise"] for it in items],
                        flip_type=[it["flip_type"] for it in items], angles=[it["angles"] for it in items])


def case_items(c):
    """The recorded draws of a fixture case as the list ``replay_draws`` returns."""
    return [{"label": int(c.draw_label[i]), "index": int(c.draw_index[i]), "loc_noise": c.draw_loc[i],
             "rot_noise": float(c.draw_rot[i]), "flip_type": int(c.draw_flip[i]), "angles": c.draw_angles[i]}
            for i in range(len(c.draw_label))]


def _rot(xyz, r):
    out = xyz.copy()
    out[:, 0] = xyz[:, 0] * np.cos(r) + xyz[:, 1] * np.sin(r)
    out[:, 1] = -xyz[:, 0] * np.sin(r) + xyz[:, 1] * np.cos(r)
    return out


def np_instance_paste(points, labels, bank, items, ground_ids=GROUND_IDS):
    """The reference's loop with the draws given.  Returns (points float64, labels, decisions, info): info holds, per
    instance, the radius and, per EVALUATED candidate, the nearest object distance, the two smallest ground distances."""
    points = np.asarray(points, dtype=np.float64)
    labels = np.asarray(labels)
    decisions, info = [], []
    for it in items:
        keep = labels != 255
        ground = keep & np.isin(labels, ground_ids)
        gp, op = points[ground, :3], points[keep & ~ground, :3]
        inst = bank[it["label"]][it["index"]]
        pts = np.array(inst["cluster_points"])
        pts[:, 3] = 0
        pts[:, 4] = np.tanh(pts[:, 4])
        pts = pts.astype(np.float64)
        xyz, feat = pts[:, :3].copy(), pts[:, 3:]
        c0 = np.mean(xyz, axis=0)
        if it["loc_noise"] is not None:
            xyz = _rot(xyz - c0, it["rot_noise"]) + np.asarray(it["loc_noise"])[None, :] + c0
        if it["flip_type"] == 3:
            long_axis = np.array([c0[0], c0[1]]) / (c0[0] ** 2 + c0[1] ** 2) ** 0.5
            a, b = -long_axis[1], long_axis[0]
            m = np.array([[b ** 2 - a ** 2, -2 * a * b], [-2 * a * b, a ** 2 - b ** 2]])
            xyz[:, :2] = (xyz[:, :2] - c0[:2]) @ m.T + c0[:2]
        center = np.mean(xyz, axis=0)
        radius = np.max(np.linalg.norm(xyz - center, axis=1))
        rec = {"radius": radius, "obj": [], "g0": [], "g1": []}
        choice = -1
        for ci, r in enumerate(it["angles"]):
            c = _rot(center[None, :], r)[0]
            od = np.linalg.norm(op - c, axis=1) if len(op) else np.zeros(0)
            gd = np.linalg.norm(gp - c, axis=1) if len(gp) else np.zeros(0)
            gs = np.sort(gd)
            rec["obj"].append(od.min() if len(od) else np.inf)
            rec["g0"].append(gs[0] if len(gs) else np.inf)
            rec["g1"].append(gs[1] if len(gs) > 1 else np.inf)
            if (len(od) == 0 or np.all(od > radius)) and len(gd) and np.any(gd < 1.2 * radius):
                choice = ci
                xyz[:, 2] += (gp[np.argmin(gd), 2] + inst["cluster_height"]) - c[2]
                xyz = _rot(xyz, r)
                break
        decisions.append(choice)
        info.append(rec)
        if choice >= 0:
            points = np.concatenate((points, np.concatenate((xyz, feat), axis=1)), axis=0)
            labels = np.concatenate((labels, np.ones(len(xyz), dtype=labels.dtype) * it["label"]))
    return points, labels, decisions, info


def make_scene(seed, n_ground=1000, n_clusters=25, n_ignored=100, dim=6):
    """A noisy ground disc of radius 30 m at z ~ -1.8 (labels 17-21), object clusters at 5-27 m (labels 0-16), rows of
    label 255, permuted; float64 [~1500, dim], uint8 labels."""
    rs = np.random.RandomState(seed)
    rad, ang = 30.0 * np.sqrt(rs.rand(n_ground)), rs.rand(n_ground) * 2 * np.pi
    ground = np.stack([rad * np.cos(ang), rad * np.sin(ang), -1.8 + 0.03 * rs.randn(n_ground)], axis=1)
    rows, labs = [ground], [rs.randint(17, 22, n_ground)]
    for _ in range(n_clusters):
        m = rs.randint(8, 25)
        d, a = rs.uniform(5, 27), rs.rand() * 2 * np.pi
        ctr = np.array([d * np.cos(a), d * np.sin(a), -1.8 + rs.uniform(0.4, 1.0)])
        rows.append(ctr + rs.randn(m, 3) * [0.5, 0.5, 0.3])
        labs.append(np.full(m, rs.randint(0, 17)))
    rows.append(np.concatenate([rs.uniform(-30, 30, (n_ignored, 2)), rs.uniform(-2, 2, (n_ignored, 1))], axis=1))
    labs.append(np.full(n_ignored, 255))
    xyz = np.concatenate(rows)
    pts = np.concatenate([xyz, rs.rand(len(xyz), dim - 3)], axis=1)
    perm = rs.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), np.concatenate(labs).astype(np.uint8)[perm]


def make_bank(seed, labels=INSTANCE_IDS, per_label=PER_LABEL, dim=6):
    """labels x per_label clusters of 20-60 points at 6-24 m from the origin, tall / thin and low / wide ones mixed."""
    rs = np.random.RandomState(seed)
    bank = {}
    for lab in labels:
        bank[lab] = []
        for _ in range(per_label):
            m = rs.randint(20, 61)
            d, a = rs.uniform(6, 24), rs.rand() * 2 * np.pi
            h, s = rs.uniform(0.8, 1.8), rs.uniform(0.2, 0.6)
            xyz = np.stack([d * np.cos(a) + s * rs.randn(m), d * np.sin(a) + s * rs.randn(m), -1.8 + h * rs.rand(m)], axis=1)
            pts = np.concatenate([xyz, rs.randn(m, dim - 3)], axis=1)
            bank[lab].append({"cluster_points": pts, "cluster_height": float(xyz[:, 2].mean() + 1.8)})
    return bank


def tie_case(n, low_first, dim=6):
    """A frame with two ground rows at bit-identical distance 0.5 from the only candidate centre (10, 0, 0) -- mirrored
    in y and in z, so their z differ -- one at row 3, one at row n - 5; every other row is ground farther away or an
    object far off.  The bank is one two-point cluster whose mean is exactly (10, 0, 0), radius 0.5, height 0.25.
    Returns (points, labels, bank, items, ground_z the lower row holds)."""
    rs = np.random.RandomState(n)
    pts = np.zeros((n, dim))
    ang = rs.rand(n) * 2 * np.pi
    pts[:, 0], pts[:, 1], pts[:, 2] = 10 + 3 * np.cos(ang), 3 * np.sin(ang), -0.4  # ground, 3 m from the centre
    labels = np.full(n, 17, np.uint8)
    obj = rs.rand(n) < 0.3
    pts[obj, 0] -= 40.0
    labels[obj] = 5
    z = (-0.4, 0.4) if low_first else (0.4, -0.4)
    pts[3, :3], pts[n - 5, :3] = (10.0, 0.3, z[0]), (10.0, -0.3, z[1])
    labels[3] = labels[n - 5] = 19
    cluster = np.zeros((2, dim))
    cluster[:, :3] = [[10.0, 0.0, 0.5], [10.0, 0.0, -0.5]]
    cluster[:, 3:] = [[0.5, 0.25, 7.0][:dim - 3], [0.5, -0.5, 8.0][:dim - 3]]
    bank = {4: [{"cluster_points": cluster, "cluster_height": 0.25}]}
    items = [{"label": 4, "index": 0, "loc_noise": None, "rot_noise": None, "flip_type": None, "angles": np.zeros(1)}]
    return pts, labels, bank, items, z[0]


def check_golden(c, points, labels, decisions, feats=None, xyz_tol=XYZ_TOL, z_tol=XYZ_TOL, what=""):
    n = len(c.points)
    assert list(decisions) == c.decisions.tolist(), (what, decisions)
    assert points.dtype == np.float64 and points.shape == (n + len(c.add_points), 6)
    assert np.array_equal(labels[n:], c.add_labels) and np.array_equal(labels[:n], c.labels) and labels.dtype == c.labels.dtype
    assert np.array_equal(points[n:, 3:], c.add_points[:, 3:])  # bit for bit
    err = np.abs(points[n:, :3] - c.add_points[:, :3]).max(axis=0)
    print(f"{what}: worst |x|, |y|, |z| error of pasted rows {err} m (bounds {xyz_tol}, {xyz_tol}, {z_tol})")
    assert err[0] <= xyz_tol and err[1] <= xyz_tol and err[2] <= z_tol, (what, err)
    if c.feats is not None and feats is not None:
        assert feats.dtype == c.feats.dtype and np.array_equal(feats[:n], c.feats) and feats.shape == (len(points), 4)
        assert not feats[n:].any()
