"""``WaymoDataset``: the reference's dataset class (seg3d/datasets/waymo_dataset.py) on this library.

Two ways to run it, neither a fallback for the other:

``device=None`` is the reference's behaviour -- numpy in, numpy out, usable in forked DataLoader workers.
``__getitem__`` returns the reference's dict (same keys, dtypes and row order), computed by the library's HOST entries:
``seg3d_frame_assemble_host`` for load_points / load_points_from_sweeps (:145-202), ``seg3d_voxelize_host_*`` for the
voxel generator, ``TrainAugmentation`` / ``InstanceAugmentation`` on numpy arrays with ``rng="numpy"``, and a vectorised
restatement of the voxel-label vote (:213-246).  Every draw from ``numpy.random`` comes in the reference's order: the
history choice (:182-183), ``randint`` for the second frame (:308), InstanceAugmentation, PolarMix, the transforms.

``device="cuda"`` splits the work where the file system ends.  ``load_raw(index)`` (= ``__getitem__``) does the
``np.load`` / ``np.loadtxt`` calls and returns a picklable dict of raw arrays -- what a DataLoader worker hands over, with
``collate_raw`` as the ``collate_fn``.  ``assemble(list_of_raw)`` uploads each sweep once and does everything else on the
device: ``seg3d_frame_assemble`` (one launch per frame for all sweeps), the label remap, the image-feature scatter,
``TrainAugmentation.apply``, ``cart2polar``, the voxelizer, ``prepare_voxel_labels`` and the collation.  It returns the
``batch_dict`` of ``batch.batch_from_resident`` plus ``point_labels``, ``voxel_labels``, ``voxel_id_offset``,
``filename`` and (testing) ``points_ri``.  Voxelization runs in the dtype the reference voxelizes in (the file's own
dtype without augmentation, float32 after it), per frame, so the voxel ids are the reference's; the float32 cast for the
model comes after.

``sweep_cache=n`` (validation / testing on the device) keeps the last ``n`` uploaded sweeps in HBM.  ``load_raw`` then
reads the current sweep only and names the history sweeps (``sweeps[s] is None``, ``sweep_names``); ``assemble`` takes
them from the cache, reads and uploads a missing one itself, and puts the current sweep in afterwards.  Frames taken in
order then read and upload every lidar file once instead of ``NUM_SWEEPS`` times; the batch is the same bit
for bit in any order.
"""
import glob
import os
from collections import OrderedDict, defaultdict

import numpy as np
import torch
from torch.utils.data import Dataset

from . import augment, image_features, ops, scene
from ._lib import Seg3dError
from .batch import VoxelGenerator


class WaymoDataset(Dataset):
    def __init__(self, cfg, data_root, mode='training', device=None, rng="device", instance_bank=None, sweep_cache=None):
        assert mode in ['training', 'validation', 'testing']
        self.cfg = cfg
        self.data_root = data_root
        self.mode = mode
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise Seg3dError("device is None (the host entries) or a CUDA device")
        # sweep_cache = n: the last n uploaded sweeps stay on the device, keyed by file name, and ``assemble`` takes a
        # frame's history sweeps from there (frames evaluated in order share all but one sweep with their predecessor)
        if sweep_cache is not None:
            if self.device is None:
                raise ValueError("sweep_cache keeps uploaded sweeps on the device: it needs device='cuda'")
            if mode == 'training':
                raise ValueError("sweep_cache is for frames read in order: training draws its history sweeps at random "
                                 "and shuffles frames")
            if int(sweep_cache) < 1:
                raise ValueError(f"sweep_cache={sweep_cache}: the number of sweeps kept, at least 1")
        self.sweep_cache = None if sweep_cache is None else int(sweep_cache)
        self._resident_sweeps = OrderedDict()  # file name -> uploaded [N, DIM_POINT] rows, least recently used first

        all_filenames = self.get_dir_filenames('lidar')
        self.file_idx_to_name = self.build_file_idx_to_name(all_filenames)
        if self.mode == 'testing':
            self.filenames = self.get_testing_filenames(all_filenames)
        else:
            self.filenames = self.get_dir_filenames('label')

        self.voxel_generator = VoxelGenerator(voxel_size=cfg.DATASET.VOXEL_SIZE,
                                              point_cloud_range=cfg.DATASET.POINT_CLOUD_RANGE)
        self.grid_size = self.voxel_generator.grid_size
        self.voxel_size = self.voxel_generator.voxel_size
        self.point_cloud_range = self.voxel_generator.point_cloud_range

        # :37-39 draws PolarMix's two paste angles whatever the config says; from_config draws them for single-sweep
        # configs, so the other configs consume the same two numbers here
        if instance_bank is None:
            bank_path = os.path.join(self.data_root, 'instances/lidar_instances_with_height.pkl')
            use_bank = mode == 'training' and cfg.DATASET.AUG_DATA and not cfg.DATASET.USE_MULTI_SWEEPS
            instance_bank = bank_path if use_bank and os.path.exists(bank_path) else None
        # the host path replays the reference draw for draw; the device path takes the caller's choice
        self.train_aug = augment.TrainAugmentation.from_config(cfg, rng="numpy" if self.device is None else rng,
                                                               instance_bank=instance_bank)
        if cfg.DATASET.USE_MULTI_SWEEPS:
            np.random.random()
            np.random.random()
        self.polar_mix = self.train_aug.polar_mix
        self.last_draw = None
        self.instance_aug = self.train_aug.instance_aug

    # ------------------------------------------------------------------------------------------ :52-91
    @property
    def dim_point(self):
        return self.cfg.DATASET.DIM_POINT

    @property
    def use_multi_sweeps(self):
        return self.cfg.DATASET.USE_MULTI_SWEEPS

    @property
    def use_cylinder(self):
        return self.cfg.DATASET.USE_CYLINDER

    @property
    def num_classes(self):
        return self.cfg.DATASET.NUM_CLASSES

    @property
    def class_names(self):
        return self.cfg.DATASET.CLASS_NAMES

    @property
    def class_weight(self):
        return self.cfg.DATASET.CLASS_WEIGHT

    @property
    def palette(self):
        return self.cfg.DATASET.PALETTE

    @property
    def use_image_feature(self):
        return self.cfg.DATASET.USE_IMAGE_FEATURE

    @property
    def dim_image_feature(self):
        return self.cfg.DATASET.DIM_IMAGE_FEATURE

    @property
    def ignore_index(self):
        return self.cfg.DATASET.IGNORE_INDEX

    @property
    def _augments(self):
        return self.mode == 'training' and bool(self.cfg.DATASET.AUG_DATA)

    # ------------------------------------------------------------------------------------------ file names
    @staticmethod
    def parse_filename(filename):
        """'<file_idx>-<timestamp>-<frame_idx>' -> (file_idx, frame_idx, timestamp)."""
        file_idx, timestamp, frame_idx = filename.split('-')[:3]
        return file_idx, int(frame_idx), np.int64(timestamp)

    def get_dir_filenames(self, dir_name):
        paths = glob.glob(os.path.join(self.data_root, dir_name, '*.npy'))
        return [os.path.splitext(os.path.basename(p))[0] for p in paths]

    def get_testing_filenames(self, filenames):
        wanted = set()
        with open(os.path.join(self.data_root, '3d_semseg_test_set_frames.txt'), 'r') as fp:
            for line in fp.read().splitlines():
                parts = line.split(',')
                wanted.add((parts[0], np.int64(parts[1])))
        keep = []
        for filename in filenames:
            file_idx, _, timestamp = self.parse_filename(filename)
            if (file_idx, timestamp) in wanted:
                keep.append(filename)
        return keep

    def build_file_idx_to_name(self, filenames):
        table = dict()
        for filename in filenames:
            file_idx, frame_idx, _ = self.parse_filename(filename)
            table[(file_idx, frame_idx)] = filename
        return table

    # ------------------------------------------------------------------------------------------ files
    def load_pose(self, filename):
        return np.loadtxt(os.path.join(self.data_root, 'pose', filename + '.txt'))

    def _raw_points(self, filename):
        return np.load(os.path.join(self.data_root, 'lidar', filename + '.npy'))

    def _raw_image_features(self, filename):
        """(rows int32 [K], feats float32 [K, F]) of a frame.  ``image_feature/<name>.npz`` (image_features.save_packed:
        the two arrays as they are, no pickle, no loop) is read when it exists; otherwise the reference's pickled dict
        row -> feature, ``<name>.npy``, is flattened as before.  When both files exist the packed one wins."""
        packed = os.path.join(self.data_root, 'image_feature', filename + '.npz')
        if os.path.exists(packed):
            rows, feats = image_features.load_packed(packed)
            if feats.shape[1] != self.dim_image_feature:
                raise Seg3dError(f"{packed}: {feats.shape[1]} features per row, DIM_IMAGE_FEATURE is {self.dim_image_feature}")
            return rows, feats
        d = np.load(os.path.join(self.data_root, 'image_feature', filename + '.npy'), allow_pickle=True).item()
        rows = np.fromiter(d.keys(), dtype=np.int64, count=len(d)).astype(np.int32)
        feats = np.zeros((len(d), self.dim_image_feature), dtype=np.float32)
        for j, v in enumerate(d.values()):
            feats[j] = v
        return rows, feats

    def load_image_features(self, num_points, filename):
        rows, feats = self._raw_image_features(filename)
        out = np.zeros((num_points, self.dim_image_feature), dtype=np.float32)
        out[rows] = feats
        return out

    def load_points(self, filename):
        """:145-154: the file's rows with the range column zeroed and the intensity through tanh."""
        raw = self._raw_points(filename)
        return ops.frame_assemble_host(ops.sweep_table([raw]), want=("rows",))["rows"]

    def _sweep_plan(self, filename, num_sweeps, max_num_sweeps):
        """The sweeps of a frame, current first: (filenames, matrices, lags).  :165-198 without the arithmetic; draws the
        history choice from numpy.random in training mode."""
        file_idx, frame_idx, timestamp = self.parse_filename(filename)
        ts = timestamp / 1e6
        pose = self.load_pose(filename)
        history = [self.file_idx_to_name[(file_idx, frame_idx - i - 1)] for i in range(max_num_sweeps - 1)
                   if frame_idx - i - 1 >= 0]
        want = num_sweeps - 1
        if len(history) <= want:
            choices = np.arange(len(history))
        elif self.mode == 'training':
            choices = np.random.choice(len(history), want, replace=False)
        else:
            choices = np.arange(want)
        names, matrices, lags = [filename], [None], [0.0]
        inv_pose = None
        for idx in choices:
            sweep = history[idx]
            if inv_pose is None:
                inv_pose = np.linalg.inv(pose)
            # :193 computes inv() once per sweep; the same input gives the same bits
            matrices.append(inv_pose @ self.load_pose(sweep))
            lags.append(ts - self.parse_filename(sweep)[-1] / 1e6)
            names.append(sweep)
        return names, matrices, lags

    def load_points_from_sweeps(self, filename, num_sweeps=3, max_num_sweeps=5, pad_empty_sweeps=False):
        if pad_empty_sweeps:
            raise NotImplementedError("pad_empty_sweeps=True: no caller of the reference sets it")
        names, matrices, lags = self._sweep_plan(filename, num_sweeps, max_num_sweeps)
        raws = [self._raw_points(n) for n in names]
        points = ops.frame_assemble_host(ops.sweep_table(raws, matrices, lags), want=("rows",))["rows"]
        return points, np.arange(raws[0].shape[0])

    def _raw_labels(self, filename):
        return np.load(os.path.join(self.data_root, 'label', filename + '.npy'))[:, 1]

    def load_label(self, filename):
        """:204-211: the semantic column, shifted by one, unlabelled (0) -> 255."""
        labels = self._raw_labels(filename)
        labels -= 1
        labels[labels == -1] = 255
        return labels

    # ------------------------------------------------------------------------------------------ host path
    def prepare_voxel_labels(self, data_dict):
        """:213-246: per voxel the most frequent label among its (current-sweep) points, ties to the smallest label,
        ignore_index where no such point lies."""
        assert self.ignore_index == 255
        ids = data_dict.get('point_voxel_ids', None)
        labels = data_dict.get('point_labels', None)
        coords = data_dict.get('voxel_coords', None)
        assert ids is not None and labels is not None and coords is not None
        cur = data_dict.get('cur_point_indices', None)
        ids = np.asarray(ids if cur is None else ids[cur]).astype(np.int64)
        labels = np.asarray(labels).astype(np.int64)
        keep = ids != -1
        keys, counts = np.unique(ids[keep] * 256 + labels[keep], return_counts=True)
        vox, lab = keys // 256, keys % 256
        order = np.lexsort((lab, -counts, vox))
        first = np.ones(len(order), dtype=bool)
        first[1:] = vox[order][1:] != vox[order][:-1]
        voxel_labels = np.full(coords.shape[0], self.ignore_index, dtype=np.uint8)
        voxel_labels[vox[order][first]] = lab[order][first]
        data_dict['voxel_labels'] = voxel_labels

    def prepare_data(self, data_dict):
        """:248-279 for a frame whose training transforms have run (``__getitem__`` runs them with the rest of the
        augmentation): cur_point_count, the cylinder rows, the voxelizer."""
        if self.use_multi_sweeps:
            data_dict['cur_point_count'] = data_dict['cur_point_indices'].shape[0]
        else:
            data_dict['cur_point_count'] = data_dict['points'].shape[0]
        if self.use_cylinder:
            data_dict['points'] = scene.cart2polar_rows(data_dict['points'])
        coords, ids = self.voxel_generator.generate(data_dict['points'])
        data_dict['voxel_coords'] = coords
        data_dict['point_voxel_ids'] = ids
        return data_dict

    def _getitem_host(self, index):
        filename = self.filenames[index]
        d = {'filename': filename}
        multi, image = self.use_multi_sweeps, self.use_image_feature
        if multi:
            points, cur = self.load_points_from_sweeps(filename, self.cfg.DATASET.NUM_SWEEPS,
                                                       self.cfg.DATASET.MAX_NUM_SWEEPS)
            d['cur_point_indices'] = cur
        else:
            points = self.load_points(filename)
        d['points'] = points[:, :self.dim_point]
        n_cur = d['cur_point_indices'].shape[0] if multi else points.shape[0]
        if image:
            d['point_image_features'] = self.load_image_features(n_cur, filename)
        if self.mode != 'testing':
            d['point_labels'] = self.load_label(filename)

        if self._augments:
            feats = d.get('point_image_features')
            if multi:
                res = self.train_aug.apply(d['points'], d['point_labels'].astype(np.int64), feats,
                                           cur_point_indices=d['cur_point_indices'])
                d['cur_point_indices'] = res['cur_point_indices'].astype(np.int64)
                d['point_labels'] = res['point_labels'].astype(np.int32)
            else:
                filename2 = self.filenames[np.random.randint(len(self.filenames))]
                points2 = self.load_points(filename2)[:, :self.dim_point]
                labels2 = self.load_label(filename2).astype(np.int64)
                feats2 = self.load_image_features(points2.shape[0], filename2) if image else None
                res = self.train_aug.apply(d['points'], d['point_labels'].astype(np.int64), feats, frame2=points2,
                                           labels2=labels2, image_features2=feats2)
                d['point_labels'] = res['point_labels'].astype(np.int64)  # the reference's concatenations promote
            d['points'] = res['points']
            self.last_draw = res['draw']  # every number drawn for this frame; ``assemble(draws=...)`` replays it
            if image:
                d['point_image_features'] = res['point_image_features']

        if self.mode == 'testing':
            d['points_ri'] = points[:n_cur, -3:].astype(np.int32)
        d = self.prepare_data(d)
        if self.mode != 'testing':
            self.prepare_voxel_labels(d)
        return d

    def __getitem__(self, index):
        if self.device is None:
            return self._getitem_host(index)
        return self.load_raw(index)

    @staticmethod
    def collate_batch(batch_list, _unused=False):
        """:339-376: batch index in front of points / voxel_coords, voxel ids shifted by the voxels of earlier samples,
        cumulative voxel and current-point counts.  The samples are left unchanged."""
        cols = defaultdict(list)
        for sample in batch_list:
            for key, val in sample.items():
                cols[key].append(val)
        ret = {}
        for key, vals in cols.items():
            if key in ('points', 'voxel_coords'):
                ret[key] = np.concatenate([np.pad(v, ((0, 0), (1, 0)), mode='constant', constant_values=b)
                                           for b, v in enumerate(vals)], axis=0)
            elif key in ('points_ri', 'point_image_features', 'point_labels', 'voxel_labels'):
                ret[key] = np.concatenate(vals, axis=0)
            elif key == 'filename':
                ret[key] = vals
        ids, voxel_id_offset, count = [], [], 0
        for b, v in enumerate(cols['point_voxel_ids']):
            ids.append(np.where(v != -1, v + count, v).astype(v.dtype))
            count += cols['voxel_coords'][b].shape[0]
            voxel_id_offset.append(count)
        ret['point_voxel_ids'] = np.concatenate(ids, axis=0)
        ret['voxel_id_offset'] = np.array(voxel_id_offset)
        ret['point_id_offset'] = np.cumsum([int(c) for c in cols['cur_point_count']])
        ret['batch_size'] = len(batch_list)
        return ret

    def __len__(self):
        return len(self.filenames)

    # ------------------------------------------------------------------------------------------ device path
    def load_raw(self, index):
        """Everything of frame ``index`` that needs the file system, nothing else: host only, picklable."""
        filename = self.filenames[index]
        multi, dim = self.use_multi_sweeps, self.dim_point
        if multi:
            names, matrices, lags = self._sweep_plan(filename, self.cfg.DATASET.NUM_SWEEPS,
                                                    self.cfg.DATASET.MAX_NUM_SWEEPS)
        else:
            names, matrices, lags = [filename], [None], [0.0]
        if self.sweep_cache is None:
            raws = [self._raw_points(n) for n in names]
            raw = {'filename': filename, 'sweeps': [r[:, :dim] for r in raws], 'matrices': matrices, 'lags': lags}
        else:  # the history sweeps by name only: ``assemble`` has them on the device, or reads them on a miss
            raws = [self._raw_points(filename)]
            raw = {'filename': filename, 'sweeps': [raws[0][:, :dim]] + [None] * (len(names) - 1), 'matrices': matrices,
                   'lags': lags, 'sweep_names': names}
        if self.use_image_feature:
            raw['image_rows'], raw['image_feats'] = self._raw_image_features(filename)
        if self.mode != 'testing':
            raw['labels'] = self._raw_labels(filename)
        else:
            raw['points_ri'] = raws[0][:, -3:].astype(np.int32)
        if self._augments:
            if not multi:
                filename2 = self.filenames[np.random.randint(len(self.filenames))]
                raw['sweeps2'] = [self._raw_points(filename2)[:, :dim]]
                raw['labels2'] = self._raw_labels(filename2)
                if self.use_image_feature:
                    raw['image_rows2'], raw['image_feats2'] = self._raw_image_features(filename2)
            raw['seed'] = int(np.random.randint(0, 2 ** 32, dtype=np.uint64))
        return raw

    @staticmethod
    def collate_raw(raw_list):
        """The DataLoader's collate_fn on the device path: the list, untouched."""
        return raw_list

    def _upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _resident_sweep(self, name, rows=None):
        """The uploaded [N, DIM_POINT] rows of lidar file ``name`` through the LRU of ``sweep_cache`` sweeps.  rows: the
        file's rows when the caller has just read them (the current sweep), which are uploaded and replace the entry;
        otherwise a miss reads the file here, in the calling process."""
        cache = self._resident_sweeps
        if rows is None and name in cache:
            cache.move_to_end(name)
            return cache[name]
        t = self._upload(self._raw_points(name)[:, :self.dim_point] if rows is None else rows)
        cache[name] = t
        cache.move_to_end(name)
        while len(cache) > self.sweep_cache:
            cache.popitem(last=False)
        return t

    def _uploaded_sweeps(self, raw):
        """Every sweep of a ``load_raw`` result on the device, current first."""
        if self.sweep_cache is None:
            return [self._upload(s) for s in raw['sweeps']]
        names = raw.get('sweep_names', [raw['filename']])
        # history first: the current sweep enters the cache after the frame has taken what it needs from it
        history = [self._resident_sweep(n) if s is None else self._upload(s)
                   for n, s in zip(names[1:], raw['sweeps'][1:])]
        return [self._resident_sweep(names[0], raw['sweeps'][0])] + history

    def _labels_on_device(self, raw_labels):
        lab = self._upload(raw_labels).long() - 1
        lab[lab == -1] = 255
        return lab

    def _features_on_device(self, rows, feats, n):
        out = torch.zeros((n, self.dim_image_feature), dtype=torch.float32, device=self.device)
        if len(rows):
            out.index_copy_(0, self._upload(rows).long(), self._upload(feats))
        return out

    def assemble(self, raw_list, draws=None):
        """list of ``load_raw`` results -> the collated device ``batch_dict``.  draws: per sample an ``AugDraw`` to
        replay (tests); otherwise each sample's numbers come from ``RandomState(raw['seed'])``."""
        if self.device is None:
            raise Seg3dError("assemble is the device path: construct the dataset with device='cuda'")
        dev = self.device
        vs, pcr = self.voxel_size.tolist(), self.point_cloud_range.tolist()
        image, multi = self.use_image_feature, self.use_multi_sweeps
        pts, coords, ids, labels, vlabels, feats, ri = [], [], [], [], [], [], []
        row_offsets, voxel_id_offset, n_vox, n_cur_total = [], [], 0, 0
        for b, raw in enumerate(raw_list):
            table = ops.sweep_table(self._uploaded_sweeps(raw), raw['matrices'], raw['lags'], dim=self.dim_point)
            n_cur = int(raw['sweeps'][0].shape[0])
            plain = not self._augments and not self.use_cylinder
            out = ops.frame_assemble(table, want=("rows", "collated") if plain else ("rows",), batch_id=b)
            rows = out["rows"]
            lab = self._labels_on_device(raw['labels']) if 'labels' in raw else None
            f = self._features_on_device(raw['image_rows'], raw['image_feats'], n_cur) if image else None
            cur = None
            if self._augments:
                kw = {}
                if multi:
                    kw['cur_point_indices'] = torch.arange(n_cur, dtype=torch.int32, device=dev)
                else:
                    t2 = ops.sweep_table([self._upload(s) for s in raw['sweeps2']], dim=self.dim_point)
                    kw['frame2'] = ops.frame_assemble(t2, want=("rows",))["rows"]
                    kw['labels2'] = self._labels_on_device(raw['labels2'])
                    if image:
                        kw['image_features2'] = self._features_on_device(raw['image_rows2'], raw['image_feats2'],
                                                                        int(kw['frame2'].shape[0]))
                res = self.train_aug.apply(rows, lab, f, params=None if draws is None else draws[b], seed=raw['seed'],
                                           **kw)
                rows, lab, f, cur = res['points'], res['point_labels'], res['point_image_features'], res['cur_point_indices']
                if multi:
                    n_cur = int(cur.shape[0])
                else:
                    n_cur = int(rows.shape[0])
            if self.use_cylinder:
                rows = ops.cart2polar(rows)
            c, i = ops.voxelize(rows, vs, pcr)  # the frame's own dtype: the reference's voxel ids
            if lab is not None:
                vlabels.append(ops.prepare_voxel_labels(i, lab, c.shape[0], self.ignore_index,
                                                        None if not multi else (cur.long() if cur is not None else
                                                                                torch.arange(n_cur, device=dev))))
                labels.append(lab)
            if plain:
                pts.append(out["collated"])
            else:
                pts.append(torch.nn.functional.pad(rows.float(), (1, 0), value=float(b)))
            c = c.clone()
            c[:, 0] = b
            coords.append(c)
            ids.append(torch.where(i >= 0, i + n_vox, i))
            n_vox += int(c.shape[0])
            voxel_id_offset.append(n_vox)
            n_cur_total += n_cur
            row_offsets.append(n_cur_total)
            if image:
                feats.append(f)
            if 'points_ri' in raw:
                ri.append(self._upload(raw['points_ri']))
        ids32 = torch.cat(ids)
        batch = {
            "points": torch.cat(pts),
            "voxel_coords": torch.cat(coords).float(),
            "point_voxel_ids": ids32.long(),
            "point_id_offset": torch.tensor(row_offsets, dtype=torch.float32, device=dev),
            "point_row_offsets": [int(o) for o in row_offsets],
            "point_voxel_index": ops.SegmentIndex(ids32, n_vox),
            "batch_size": len(raw_list),
            "voxel_id_offset": torch.tensor(voxel_id_offset, dtype=torch.float32, device=dev),
            "filename": [raw['filename'] for raw in raw_list],
        }
        if image:
            batch["point_image_features"] = torch.cat(feats)
        if labels:
            batch["point_labels"] = torch.cat(labels)
            batch["voxel_labels"] = torch.cat(vlabels).long()
        if ri:
            batch["points_ri"] = torch.cat(ri)
        return batch
