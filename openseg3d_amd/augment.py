"""Training augmentation: PolarMix, the global transforms, PointShuffle and PointSample (csrc/augment.hip).

The reference runs these once per training frame on the host, between the disk and the voxelizer
(seg3d/datasets/transforms/polarmix.py, transforms.py, transform_utils.py; composed at
seg3d/datasets/waymo_dataset.py:44-50, called at :262-263 and :307-323).  Here every stage that selects or reorders rows
composes an int32 source map and one kernel gathers and transforms the rows; labels and image features go through the
same map.  numpy arrays in give numpy arrays out through the library's host entries (no HIP call: DataLoader workers);
CUDA tensors in stay on the device.  Neither is a fallback for the other.

Random numbers.  ``rng="numpy"`` reproduces the reference draw for draw from ``numpy.random``: the host draws the
PointShuffle permutation and the PointSample choices, and because the far / near lists it draws from come back from the
device this mode has ONE MORE host sync than the other.  ``rng="device"`` draws only the scalars on the host; shuffle
and sample are sorts of hashed keys on the device: the reference's distribution, not its draws.

Out of scope: ``InstanceAugmentation`` (it needs a pickled instance bank that is not part of this repository) and
``RandomDropPointsColor`` (no config composes it)."""
import numpy as np
import torch

from . import ops
from ._lib import Seg3dError


class _Host:
    polarmix_map = staticmethod(ops.polarmix_map_host)
    far_near = staticmethod(ops.aug_far_near_host)
    sample = staticmethod(lambda flag, n, m, seed, like: ops.aug_sample_host(flag, n, m, seed))
    cur_map = staticmethod(ops.aug_cur_map_host)
    apply = staticmethod(ops.aug_apply_host)
    gather = staticmethod(ops.aug_gather_host)

    @staticmethod
    def index(a, like):
        return np.ascontiguousarray(a, dtype=np.int32)


class _Device:
    polarmix_map = staticmethod(ops.polarmix_map)
    far_near = staticmethod(ops.aug_far_near)
    sample = staticmethod(lambda flag, n, m, seed, like: ops.aug_sample_device(flag, n, m, seed, device=like.device))
    cur_map = staticmethod(ops.aug_cur_map)
    apply = staticmethod(ops.aug_apply)
    gather = staticmethod(ops.aug_gather)

    @staticmethod
    def index(a, like):
        if isinstance(a, torch.Tensor):
            return a.to(device=like.device, dtype=torch.int32)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(like.device)


def _backend(x):
    if isinstance(x, np.ndarray):
        return _Host
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return _Device
    raise Seg3dError("augmentation takes numpy arrays (host entries) or CUDA tensors (device entries)")


class AugDraw:
    """The parameter record of one frame: every number the reference draws from ``numpy.random`` for it."""
    __slots__ = ("swap", "alpha", "beta", "rot", "scale", "offsets", "flip_x", "flip_y", "perm", "choices")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class PolarMix:
    """``seg3d.datasets.transforms.polarmix.PolarMix``: same constructor, same ``__call__`` signature and row order
    (polarmix.py:67-111).  The returned points are float32 -- the rounding ``transform_utils.py:7`` applies to them next;
    the paste rotation itself is done in float64 as the reference's ``np.dot`` does."""

    def __init__(self, instance_classes, rot_angle_range):
        self.instance_classes = list(instance_classes)
        self.rot_angle_range = list(rot_angle_range)
        if len(self.rot_angle_range) > ops.AUG_MAX_PASTE:
            raise Seg3dError(f"at most {ops.AUG_MAX_PASTE} paste angles")

    def draw(self, rng_state=np.random):
        """polarmix.py:80-91: random() for the swap, random() for alpha when swapping, random() for the paste."""
        swap = rng_state.random() < 0.5
        alpha = beta = 0.0
        if swap:
            alpha = (rng_state.random() - 1) * np.pi
            beta = alpha + np.pi
        rng_state.random()  # `if np.random.random() < 1.0`: always taken, the draw is still consumed
        return swap, alpha, beta

    def row_map(self, points1, points2, labels2, swap, alpha, beta):
        """(src, op): the rows of the result as rows of [points1; points2] and the paste angle of each (0 = copy)."""
        src, op, _, _ = _backend(points1).polarmix_map(points1, points2, labels2, swap, alpha, beta,
                                                      self.instance_classes, len(self.rot_angle_range))
        return src, op

    def __call__(self, points1, point_image_features1, labels1, points2, point_image_features2, labels2, draw=None):
        be = _backend(points1)
        swap, alpha, beta = self.draw() if draw is None else draw
        src, op = self.row_map(points1, points2, labels2, swap, alpha, beta)
        points = be.apply(points1, points2, src, op, ops.aug_params(self.rot_angle_range))
        labels = be.gather(labels1, labels2, src)
        if point_image_features1 is not None and point_image_features2 is not None:
            return points, be.gather(point_image_features1, point_image_features2, src), labels
        return points, labels


class TrainAugmentation:
    """The training pipeline of WaymoDataset (waymo_dataset.py:44-50 after :307-323) on one frame."""

    def __init__(self, rot_range, scale_range, translate_std, sample_ratio, sample_range, polar_mix=None, rng="device"):
        if rng not in ("device", "numpy"):
            raise ValueError("rng is 'device' or 'numpy'")
        self.rot_range = [float(v) for v in rot_range]
        self.scale_range = [float(v) for v in scale_range]
        self.translate_std = float(translate_std)
        self.sample_ratio = float(sample_ratio)
        self.sample_range = None if sample_range is None else float(sample_range)
        self.polar_mix = polar_mix
        self.rng = rng
        self.dim_point = None

    @classmethod
    def from_config(cls, cfg, rng="device", rng_state=np.random):
        """DATASET.AUG_* of a config.  PolarMix is built as waymo_dataset.py:37-39 builds it (two ``random()`` draws for
        the paste angles) unless DATASET.USE_MULTI_SWEEPS is set (:307); DIM_POINT columns of a frame are used (:295)."""
        d = cfg.DATASET
        pm = None
        if not d.USE_MULTI_SWEEPS:
            pm = PolarMix(instance_classes=list(range(13)),
                          rot_angle_range=[rng_state.random() * np.pi * 2 / 3, (rng_state.random() + 1) * np.pi * 2 / 3])
        aug = cls(d.AUG_ROT_RANGE, d.AUG_SCALE_RANGE, d.AUG_TRANSLATE_STD, d.AUG_SAMPLE_RATIO, d.AUG_SAMPLE_RANGE,
                  polar_mix=pm, rng=rng)
        aug.dim_point = int(d.DIM_POINT)
        return aug

    # ---------------------------------------------------------------------------------------- draws
    def draw(self, n, rng_state=np.random, polar=None):
        """The draws of the composed transforms for a frame of n rows, in the reference's call order: uniform (rotation,
        transforms.py:99); uniform (scale, :86; skipped when the range is narrower than 1e-3, :84); normal(0, std, 1)
        three times (transform_utils.py:68, :80, :92); choice([False, True], replace=False, p=[.5, .5]) twice (:41, :54);
        shuffle of arange(n) (transforms.py:143-144) -- left out with rng="device".  ``polar``: the (swap, alpha, beta)
        PolarMix drew before them (``PolarMix.draw``; n is only known after its row map).  The PointSample draws need
        the far / near lists of the shuffled frame and follow in ``draw_sample``."""
        swap, alpha, beta = polar if polar is not None else (False, 0.0, 0.0)
        rot = rng_state.uniform(self.rot_range[0], self.rot_range[1])
        scale = 1.0
        if not self.scale_range[1] - self.scale_range[0] < 1e-3:
            scale = rng_state.uniform(self.scale_range[0], self.scale_range[1])
        offsets = [float(rng_state.normal(0, self.translate_std, 1)[0]) for _ in range(3)]
        flip_x = bool(rng_state.choice([False, True], replace=False, p=[0.5, 0.5]))
        flip_y = bool(rng_state.choice([False, True], replace=False, p=[0.5, 0.5]))
        perm = None
        if self.rng == "numpy":
            perm = np.array(range(n))
            rng_state.shuffle(perm)
        return AugDraw(swap=swap, alpha=alpha, beta=beta, rot=rot, scale=scale, offsets=offsets, flip_x=flip_x,
                       flip_y=flip_y, perm=perm)

    def num_samples(self, n):
        return min(int(n * self.sample_ratio), n)  # transforms.py:212, transform_utils.py:118

    def draw_sample(self, n, far_inds, near_inds, rng_state=np.random):
        """points_random_sampling (transform_utils.py:117-134) on the far / near lists of the shuffled frame."""
        num_samples = self.num_samples(n)
        if self.sample_range is None:
            return rng_state.choice(range(n), num_samples, replace=False)
        far_inds, near_inds = np.asarray(far_inds, dtype=np.int64), np.asarray(near_inds, dtype=np.int64)
        if len(far_inds) > num_samples:
            far_inds = rng_state.choice(far_inds, num_samples, replace=False)
        num_samples -= len(far_inds)
        choices = rng_state.choice(near_inds, num_samples, replace=False)
        choices = np.concatenate((far_inds, choices))
        rng_state.shuffle(choices)
        return choices

    def _params(self, d, batch_id):
        paste = self.polar_mix.rot_angle_range if self.polar_mix is not None else ()
        return ops.aug_params(paste, d.rot, d.scale, d.offsets, d.flip_x, d.flip_y, batch_id=batch_id)

    # ---------------------------------------------------------------------------------------- the frame
    def apply(self, frame, labels, image_features=None, frame2=None, labels2=None, image_features2=None,
              cur_point_indices=None, params=None, seed=None, batch_id=None):
        """One training frame through PolarMix (single-sweep frames with a second frame, waymo_dataset.py:307-323) and
        the composed transforms.  frame [N, D] float32 / float64, labels uint8 / int64, image_features [., F];
        cur_point_indices: the current-sweep rows of a multi-sweep frame, to which labels and features are sized.
        ``params``: an ``AugDraw`` to replay (with rng="numpy" its perm and choices are used); otherwise the scalars
        are drawn from ``numpy.random.RandomState(seed)`` (``numpy.random`` itself when seed is None) and, with
        rng="device", shuffle and sample are a pure function of ``seed`` on the device.  Returns a dict of ``points``
        float32 [n_out, D] ([n_out, 1 + D] with ``batch_id``), ``point_labels``, ``point_image_features`` (None without
        features) and ``cur_point_indices`` (None for single-sweep frames), ready for ``batch.batch_from_resident``; the
        cylinder conversion stays where it is, after augmentation.  Also returned: ``draw`` (the ``AugDraw`` used) and
        ``source_rows`` (the row of [frame; frame2] behind every output row)."""
        be = _backend(frame)
        if self.dim_point is not None and frame.shape[1] > self.dim_point:
            frame = frame[:, :self.dim_point]
            frame2 = None if frame2 is None else frame2[:, :self.dim_point]
        if frame.ndim != 2 or frame.shape[1] > 16:
            raise Seg3dError(f"frames are [N, D] with D <= 16; got {tuple(frame.shape)}")
        rs = np.random if seed is None else np.random.RandomState(int(seed) & 0xFFFFFFFF)
        multi = cur_point_indices is not None
        mix = self.polar_mix is not None and frame2 is not None and not multi
        n0 = int(frame.shape[0])

        # stage 1: the PolarMix row map (one host read of its counts)
        src = op = None
        polar = None
        f2 = None
        if mix:
            polar = (params.swap, params.alpha, params.beta) if params is not None else self.polar_mix.draw(rs)
            src, op = self.polar_mix.row_map(frame, frame2, labels2, *polar)
            f2 = frame2
        n = n0 if src is None else int(src.shape[0])
        d = params if params is not None else self.draw(n, rs, polar)
        p = self._params(d, batch_id)

        # stage 2: shuffle + sample as one index list into the rows of stage 1
        m = self.num_samples(n)
        if self.rng == "numpy":
            perm = be.index(d.perm, frame)
            choices = d.choices
            if choices is None:
                if self.sample_range is None:
                    choices = self.draw_sample(n, None, None, rs)
                else:  # the extra host sync of this mode: the two lists come back for the draws
                    far, near = be.far_near(frame, f2, src, op, perm, p, self.sample_range, lists=True)
                    far, near = (far.cpu().numpy(), near.cpu().numpy()) if be is _Device else (far, near)
                    choices = self.draw_sample(n, far, near, rs)
                d.choices = choices
            idx = be.gather(perm, None, be.index(choices, frame))
        else:
            flag = None
            if self.sample_range is not None:
                flag = be.far_near(frame, f2, src, op, None, p, self.sample_range, lists=False)
            dev_seed = int(seed) if seed is not None else int(rs.randint(0, 2 ** 31 - 1))
            idx = be.sample(flag, n, m, dev_seed, frame)
        src2 = idx if src is None else be.gather(src, None, idx)
        op2 = None if op is None else be.gather(op, None, idx)

        # stage 3: the rows, once
        out = {"points": be.apply(frame, f2, src2, op2, p), "point_image_features": None, "cur_point_indices": None}
        if multi:
            cur_pos, cur_gather = be.cur_map(src2, be.index(cur_point_indices, frame), n0)
            out["cur_point_indices"] = cur_pos
            lab_idx, lab2, feat2 = cur_gather, None, None
        else:
            lab_idx, lab2, feat2 = src2, (labels2 if mix else None), (image_features2 if mix else None)
        out["point_labels"] = be.gather(labels, lab2, lab_idx)
        if image_features is not None and (not mix or image_features2 is not None):
            out["point_image_features"] = be.gather(image_features, feat2, lab_idx)
        out["draw"], out["source_rows"] = d, src2
        return out
