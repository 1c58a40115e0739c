"""Shared by test_augment_host.py and test_gpu_augment.py: the fixture tests/golden/augment.npz (written by
tests/golden/make_golden_aug.py from the reference's PolarMix and transforms), a plain numpy restatement of the PolarMix
row order for inputs the fixture does not hold, and the comparison the two files use."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "augment.npz")
ROT_RANGE = [-0.78539816, 0.78539816]
SCALE_RANGE = [0.95, 1.05]
TRANSLATE_STD = 0.5
CASES = ("swap_on", "swap_off", "sweeps")
_cache = {}


class Case:
    """One case of the fixture; array ``<case>_<name>`` is attribute ``name`` (None when the case has no such array)."""

    def __init__(self, name, arrays):
        self.name = name
        self._a = arrays

    def __getattr__(self, key):
        return self._a.get(key)

    @property
    def multi(self):
        return self.name == "sweeps"


def case(name):
    if not _cache:
        g = np.load(GOLDEN)
        for c in CASES:
            _cache[c] = Case(c, {k[len(c) + 1:]: g[k] for k in g.files if k.startswith(c + "_")})
    return _cache[name]


def make_aug(c, rng="numpy"):
    from openseg3d_amd.augment import PolarMix, TrainAugmentation
    pm = None if c.multi else PolarMix([int(v) for v in c.instance_classes], [float(a) for a in c.paste_angles])
    return TrainAugmentation(ROT_RANGE, SCALE_RANGE, TRANSLATE_STD, float(c.sample_ratio), float(c.sample_range),
                             polar_mix=pm, rng=rng)


def recorded_draw(c, with_choices=True):
    from openseg3d_amd.augment import AugDraw
    swap, alpha, beta = (False, 0.0, 0.0) if c.multi else (bool(c.swap), float(c.alpha), float(c.beta))
    return AugDraw(swap=swap, alpha=alpha, beta=beta, rot=float(c.rot), scale=float(c.scale),
                   offsets=[float(v) for v in c.offsets], flip_x=bool(c.flips[0]), flip_y=bool(c.flips[1]),
                   perm=c.perm.copy(), choices=c.choices.copy() if with_choices else None)


def np_polarmix_rows(p1, p2, l2, swap, alpha, beta, classes, n_angles):
    """(src, op) of polarmix.py:4-111 restated: rows of [p1; p2] and the paste angle of each."""
    def inside(p):
        yaw = -np.arctan2(p[:, 1].astype(np.float64), p[:, 0].astype(np.float64))
        return (yaw > alpha) & (yaw < beta) if swap else np.zeros(len(p), bool)
    n1 = len(p1)
    src = [np.where(~inside(p1))[0], n1 + np.where(inside(p2))[0]]
    inst = np.concatenate([np.where(l2 == c)[0] for c in classes] + [np.zeros(0, np.int64)]).astype(np.int64)
    op = [np.zeros(len(src[0]) + len(src[1]), np.uint8)]
    for r in range(1 + n_angles):
        src.append(n1 + inst)
        op.append(np.full(len(inst), r, np.uint8))
    return np.concatenate(src).astype(np.int32), np.concatenate(op)


def check_rows(got, want, ulps, what=""):
    """x, y within `ulps` float32 ulp of the row's planar magnitude sqrt(x^2 + y^2); z and every other column bit-exact."""
    assert got.shape == want.shape and got.dtype == np.float32, (got.shape, want.shape, got.dtype)
    if got.shape[0] == 0:
        return
    w = want.astype(np.float64)
    mag = np.sqrt(w[:, 0] ** 2 + w[:, 1] ** 2).astype(np.float32)
    ulp = np.spacing(mag).astype(np.float64)
    err = np.abs(got[:, :2].astype(np.float64) - w[:, :2]).max(axis=1) / ulp
    print(f"{what}: worst x/y error {err.max():.3f} ulp of the planar magnitude (bound {ulps}); "
          f"{int((err > 0).sum())} of {len(err)} rows differ")
    assert err.max() <= ulps, (what, float(err.max()))
    assert np.array_equal(got[:, 2:], want[:, 2:]), what
