"""Training augmentation: InstanceAugmentation (csrc/augment_instance.hip), PolarMix, the global transforms, PointShuffle
and PointSample (csrc/augment.hip).

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

``InstanceAugmentation`` (seg3d/datasets/transforms/instance_augmentation.py, called at waymo_dataset.py:314-315, :321)
pastes up to ``add_count`` objects of an instance bank into frame 1 before PolarMix.  All of its random numbers are
independent of the data, so ``draw`` takes them up front, in the reference's call order, and the placement search -- one
pass over the frame for all candidate rotations of an instance at once -- runs in the library, in double on both paths.
The bank is the reference's pickled dict; ``InstanceBank`` packs it once.

Out of scope: ``RandomDropPointsColor`` (no config composes it)."""
import pickle

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
    __slots__ = ("swap", "alpha", "beta", "rot", "scale", "offsets", "flip_x", "flip_y", "perm", "choices",
                 "instance_draw")

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


class InstanceBank:
    """The reference's instance bank, packed once: ``instances`` is its pickled dict ``label_id -> list of
    {'cluster_points': [m, D], 'cluster_height': float}`` (tools/extract_instances.py:65-76).  ``rows`` float64 [R, D]:
    every cluster's rows, with feature column 0 zeroed and feature column 1 replaced by its ``np.tanh`` as
    instance_augmentation.py:52-53 does on every call (in the cluster's own dtype, then converted exactly);
    ``entries[label]``: (first row, rows, height) per cluster."""

    def __init__(self, instances):
        self.entries = {}
        blocks, begin, dim = [], 0, None
        for label in sorted(instances):
            self.entries[int(label)] = []
            for inst in instances[label]:
                pts = np.array(inst["cluster_points"])  # a copy, as :48
                if pts.ndim != 2 or pts.shape[0] < 1 or pts.shape[1] < 3 or (dim is not None and pts.shape[1] != dim):
                    raise Seg3dError("every cluster of an instance bank is [m >= 1, D >= 3] with one D")
                dim = pts.shape[1]
                if dim > 3:
                    pts[:, 3] = 0
                if dim > 4:
                    pts[:, 4] = np.tanh(pts[:, 4])
                blocks.append(pts.astype(np.float64))
                self.entries[int(label)].append((begin, pts.shape[0], float(inst["cluster_height"])))
                begin += pts.shape[0]
        self.dim = dim
        self.rows = np.concatenate(blocks) if blocks else np.zeros((0, 3))
        self._device_rows = {}

    @classmethod
    def from_pickle(cls, path):
        with open(path, "rb") as f:
            return cls(pickle.load(f))

    def to(self, device):
        """Upload the rows once per device; returns the bank itself."""
        device = torch.device(device)
        if device not in self._device_rows:
            self._device_rows[device] = torch.from_numpy(self.rows).to(device)
        return self

    def rows_on(self, device):
        return self.to(device)._device_rows[torch.device(device)]


class InstanceBankBuilder:
    """The reference's ``tools/extract_instances.py`` as a class, for all target labels at once (the script is edited and
    run once per label): ``add`` a training frame after ``load_points`` / ``load_label``, read ``instances``.  Per frame
    and label, DBSCAN over the xy of the label's rows (``eps``, ``min_points[label]``: the script's TARGET_MIN_POINT_NUM),
    and every cluster with a ground row within 1.2 radii of its centre becomes ``{'cluster_points': the cluster's raw rows
    in the frame's dtype and row order, 'cluster_height': float}`` (:56-76) -- in the library
    (csrc/instance_extract.hip): numpy frames through the host entry, CUDA tensors through the device entry, the same
    clusters and the same heights bit for bit.  The device path reads back the counts and the cluster table in one copy
    per frame, then the kept rows in a second one.  Centre, radius and height are computed in double whatever the
    frame's dtype (numpy's ``np.mean`` of a float32 file runs in float32)."""

    def __init__(self, label_ids=[3, 4, 10], min_points={3: 120, 4: 30, 10: 30}, ground_label_ids=[17, 18, 19, 20, 21],
                 eps=0.25):
        self.label_ids = [int(v) for v in label_ids]
        if isinstance(min_points, dict):
            missing = [v for v in self.label_ids if v not in min_points]
            if missing:
                raise Seg3dError(f"no min_points for labels {missing}")
            self.min_points = [int(min_points[v]) for v in self.label_ids]
        else:
            self.min_points = [int(v) for v in min_points]
        self.ground_label_ids = [int(v) for v in ground_label_ids]
        self.eps = float(eps)
        self.instances = {v: [] for v in self.label_ids}
        self.frames = 0
        self.last_counts = None

    def add(self, points, labels):
        """One frame; returns how many instances it contributed."""
        be = _backend(points)
        if be is _Host:
            _, rows, table, counts = ops.instance_extract_host(points, labels, self.label_ids, self.min_points,
                                                               self.ground_label_ids, self.eps)
            points = np.asarray(points)
        else:
            _, rows, table, counts = ops.instance_extract(points, labels, self.label_ids, self.min_points,
                                                          self.ground_label_ids, self.eps)
        self.frames += 1
        self.last_counts = counts
        kept = [c for c in table if c["kept"]]
        if not kept:
            return 0
        if be is _Host:
            picked = points[rows[:counts[2]]]
        else:
            picked = points[rows[:counts[2]].long()].cpu().numpy()
        for c in kept:
            self.instances[int(c["label"])].append({"cluster_height": float(c["height"]),
                                                    "cluster_points": picked[c["begin"]:c["begin"] + c["rows"]].copy()})
        return len(kept)

    def bank(self):
        return InstanceBank(self.instances)

    def save(self, path):
        """The pickle the reference's ``InstanceAugmentation(instance_path)`` loads (instance_augmentation.py:21-23)."""
        with open(path, "wb") as f:
            pickle.dump(self.instances, f)


class InstanceDraw:
    """Every number ``InstanceAugmentation`` draws for one frame: per instance, in processing order, ``label``,
    ``index`` (into the bank's list of that label), ``loc_noise`` [3] and ``rot_noise`` (None without the local
    transform), ``flip_type`` (None without the flip) and the candidate ``angles``."""
    __slots__ = ("label", "index", "loc_noise", "rot_noise", "flip_type", "angles")

    def __init__(self, label=(), index=(), loc_noise=None, rot_noise=None, flip_type=None, angles=()):
        k = len(label)
        self.label, self.index = [int(v) for v in label], [int(v) for v in index]
        self.loc_noise = [None] * k if loc_noise is None else list(loc_noise)
        self.rot_noise = [None] * k if rot_noise is None else list(rot_noise)
        self.flip_type = [None] * k if flip_type is None else list(flip_type)
        self.angles = list(angles)

    def __len__(self):
        return len(self.label)


class InstanceAugmentation:
    """``seg3d.datasets.transforms.instance_augmentation.InstanceAugmentation``: the reference's constructor (a path to
    the pickled bank, or an ``InstanceBank``) and ``__call__`` signature.  The result points are float64 [n + n_added, D]
    (the reference's dtype whenever it pastes): the frame's rows unchanged, then the accepted instances.  Where the
    reference raises, this is defined: without a ground point nothing is placed, without an object point nothing
    occludes; ``random_rotate=False`` (a branch that reads an unset variable there, :90) is refused."""

    def __init__(self, instance_path, instance_label_ids=[3, 4, 10], ground_label_ids=[17, 18, 19, 20, 21], add_count=5,
                 random_rotate=True, local_transformation=True, random_flip=True):
        if not random_rotate:
            raise Seg3dError("random_rotate=False is not supported: that branch of the reference cannot run")
        self.bank = instance_path if isinstance(instance_path, InstanceBank) else InstanceBank.from_pickle(instance_path)
        self.instance_label_ids = list(instance_label_ids)
        self.ground_label_ids = list(ground_label_ids)
        self.add_count = int(add_count)
        self.random_rotate = True
        self.local_transformation = bool(local_transformation)
        self.random_flip = bool(random_flip)
        self.last_decisions = None
        self.last_bank_rows = None

    def draw(self, rng_state=np.random):
        """instance_augmentation.py:26-30, then per instance :169, :171, :66, :77, whether or not it is placed."""
        d = InstanceDraw()
        label_choice = rng_state.choice(self.instance_label_ids, self.add_count, replace=True)
        uni_label, uni_count = np.unique(label_choice, return_counts=True)
        for label_id, count in zip(uni_label, uni_count):
            if int(label_id) not in self.bank.entries or not self.bank.entries[int(label_id)]:
                raise Seg3dError(f"the instance bank has no cluster of label {int(label_id)}")
            for idx in rng_state.choice(len(self.bank.entries[int(label_id)]), count):
                d.label.append(int(label_id))
                d.index.append(int(idx))
                loc = rot = flip = None
                if self.local_transformation:
                    loc = rng_state.normal(scale=0.25, size=(1, 3))[0]
                    rot = rng_state.uniform(-np.pi / 20, np.pi / 20)
                if self.random_flip:
                    flip = int(rng_state.choice(5, 1)[0])
                d.loc_noise.append(loc)
                d.rot_noise.append(rot)
                d.flip_type.append(flip)
                d.angles.append(rng_state.random(20) * np.pi * 2)
        return d

    def plans(self, draw):
        out = []
        for i in range(len(draw)):
            entries = self.bank.entries.get(draw.label[i], [])
            if not 0 <= draw.index[i] < len(entries):
                raise Seg3dError(f"no cluster {draw.index[i]} of label {draw.label[i]} in the instance bank")
            begin, rows, height = entries[draw.index[i]]
            out.append(ops.aug_instance_plan(begin, rows, draw.label[i], height, draw.loc_noise[i], draw.rot_noise[i],
                                             draw.flip_type[i] == 3, draw.angles[i]))
        return out

    def __call__(self, points, point_image_features, labels, draw=None):
        be = _backend(points)
        if points.ndim != 2 or self.bank.dim is None or points.shape[1] != self.bank.dim:
            raise Seg3dError(f"the instance bank has {self.bank.dim} columns, the frame {tuple(points.shape)}")
        draw = self.draw() if draw is None else draw
        plans = self.plans(draw)
        if be is _Host:
            add_p, add_l, decisions = ops.aug_instance_paste_host(points, labels, self.ground_label_ids, self.bank.rows, plans)
            cat, f64 = np.concatenate, (lambda a: np.asarray(a, dtype=np.float64))
            zeros = lambda m, like: np.zeros((m,) + tuple(like.shape[1:]), dtype=like.dtype)  # noqa: E731
        else:
            add_p, add_l, decisions = ops.aug_instance_paste(points, labels, self.ground_label_ids,
                                                             self.bank.rows_on(points.device), plans)
            cat, f64 = torch.cat, (lambda a: a.to(torch.float64))
            zeros = lambda m, like: torch.zeros((m,) + tuple(like.shape[1:]), dtype=like.dtype, device=like.device)  # noqa: E731
        self.last_decisions = decisions
        rows = [np.arange(p.row_begin, p.row_begin + p.n_rows) for p, c in zip(plans, decisions) if c >= 0]
        self.last_bank_rows = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int64)
        points = cat((f64(points), add_p))
        labels = cat((labels, add_l))
        if point_image_features is not None:  # :95-102: pasted rows have no image features
            m = int(add_p.shape[0])
            return points, cat((point_image_features, zeros(m, point_image_features))), labels
        return points, labels


class TrainAugmentation:
    """The training pipeline of WaymoDataset (waymo_dataset.py:44-50 after :307-323) on one frame."""

    def __init__(self, rot_range, scale_range, translate_std, sample_ratio, sample_range, polar_mix=None, rng="device",
                 instance_bank=None):
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
        if instance_bank is not None and not isinstance(instance_bank, InstanceAugmentation):
            instance_bank = InstanceAugmentation(instance_bank)  # an InstanceBank or a path, the reference's defaults
        self.instance_aug = instance_bank

    @classmethod
    def from_config(cls, cfg, rng="device", rng_state=np.random, instance_bank=None):
        """DATASET.AUG_* of a config.  PolarMix is built as waymo_dataset.py:37-39 builds it (two ``random()`` draws for
        the paste angles) unless DATASET.USE_MULTI_SWEEPS is set (:307); DIM_POINT columns of a frame are used (:295).
        ``instance_bank``: an ``InstanceAugmentation`` (or an ``InstanceBank`` / a path for one with the reference's
        defaults, :41-42); its constructor draws nothing."""
        d = cfg.DATASET
        pm = None
        if not d.USE_MULTI_SWEEPS:
            pm = PolarMix(instance_classes=list(range(13)),
                          rot_angle_range=[rng_state.random() * np.pi * 2 / 3, (rng_state.random() + 1) * np.pi * 2 / 3])
        aug = cls(d.AUG_ROT_RANGE, d.AUG_SCALE_RANGE, d.AUG_TRANSLATE_STD, d.AUG_SAMPLE_RATIO, d.AUG_SAMPLE_RANGE,
                  polar_mix=pm, rng=rng, instance_bank=instance_bank)
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
        ``source_rows`` (the row of [frame; frame2] behind every output row).  With an instance bank (and PolarMix
        running) ``InstanceAugmentation`` pastes into frame 1 first (waymo_dataset.py:313-315, :321), its draws before
        PolarMix's: ``instance_draw`` is the ``InstanceDraw`` used (replayed from ``params.instance_draw`` when that is
        set) and a pasted row's ``source_rows`` entry is ``-1 - bank_row``."""
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

        # stage 0: instance copy-paste into frame 1 (one host read of its counts)
        inst_draw = None
        n_added = 0
        if mix and self.instance_aug is not None:
            inst_draw = params.instance_draw if params is not None and params.instance_draw is not None else \
                self.instance_aug.draw(rs)
            res = self.instance_aug(frame, image_features, labels, draw=inst_draw)
            frame, labels = res[0], res[-1]
            image_features = res[1] if image_features is not None else None
            if frame2.dtype != frame.dtype:  # the pasted frame is float64; both frames go through one kernel
                frame2 = frame2.astype(np.float64) if be is _Host else frame2.to(torch.float64)
            n_added = int(frame.shape[0]) - n0

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
        if n_added:  # rows of the pasted frame-1 -> rows of [frame; frame2] as the caller passed them
            bank_rows = be.index(-1 - self.instance_aug.last_bank_rows, frame)
            xp = np if be is _Host else torch
            pasted = (src2 >= n0) & (src2 < n0 + n_added)
            clamped = xp.where(pasted, src2 - n0, xp.zeros_like(src2))
            src2 = xp.where(pasted, bank_rows[clamped.astype(np.int64) if be is _Host else clamped.long()],
                            xp.where(src2 >= n0 + n_added, src2 - n_added, src2))
        d.instance_draw = inst_draw
        out["draw"], out["source_rows"], out["instance_draw"] = d, src2, inst_draw
        return out
