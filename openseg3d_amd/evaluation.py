"""Evaluation: ``IOUMetric`` and ``MultiScaleFlipAug`` drop-ins, and the device path behind ``tools/eval.py --tta``.

Reference: seg3d/core/evaluation/iou_metric.py (IOUMetric), seg3d/datasets/transforms/test_time_aug.py
(MultiScaleFlipAug), tools/eval.py:35-64 (the eval loop), seg3d/utils/data_utils.py:6-15 (load_data_to_gpu).

The reference's ``--tta`` loop builds 36 views of a frame on the host (numpy / torch CPU transforms and a CPU
re-voxelization each), uploads them one by one, runs 36 batch-1 forwards, softmaxes each, stacks and averages them, and
scores the argmax with a numpy ``bincount``.  ``MultiScaleFlipAug.predict`` uploads the frame once, builds all views in
one launch (seg3d_tta_views_f32), voxelizes K views at a time on the device as one batch of K scenes, and folds every
forward's softmax into a running sum (seg3d_softmax_accumulate_f32); ``segment_frame`` takes the argmax and feeds the
confusion matrix in the same pass (seg3d_argmax_confusion).  The list form ``MultiScaleFlipAug.__call__`` stays for
the reference's loop as written.

Multi-sweep frames (configs/waymo_multi_sweeps.yaml), which the reference's views cannot carry (test_time_aug.py:23-24
copies no ``cur_point_indices``): a view transforms x, y, z of every row, current and history; the current rows are those
whose lag column is exactly 0, and the result has one row per current row, in the order of ``point_labels``,
``points_ri`` and ``point_image_features``.  Each view searches its own fusion kNN.
"""
import warnings

import numpy as np
import torch
import torch.distributed as dist

from . import batch as B
from . import ops

# views per forward of MultiScaleFlipAug.predict: measured by tools/tta_bench.py ("Evaluation")
DEFAULT_VIEWS_PER_FORWARD = 9
MAX_BATCH = 255  # batch fields of the kNN and tiled-conv kernels are 8 bits (knn.hip, spconv_tile.hip)


def load_data_to_gpu(data_dict, device="cuda"):
    """seg3d/utils/data_utils.py:6-15: numpy arrays -> device tensors, int64 for ids and labels, float32 otherwise."""
    for key, val in data_dict.items():
        if not isinstance(val, np.ndarray):
            continue
        if key in ("point_voxel_ids", "point_labels", "voxel_labels"):
            data_dict[key] = torch.from_numpy(val).long().to(device)
        else:
            data_dict[key] = torch.from_numpy(val).float().to(device)
    return data_dict


class IOUMetric:
    """seg3d.core.IOUMetric (iou_metric.py:6-85) with the same interface.  ``add`` of CUDA tensors accumulates the
    confusion matrix on the device (seg3d_argmax_confusion, labels as delivered: uint8 or int64); anything else goes
    through numpy ``bincount`` on the host.  ``get_metric`` sums both, all-reduces over the default process group when
    one is initialised (so frames sharded across ranks give the global matrix), and returns
    ``{'mIOU': float, 'IOU': {name: float}}`` -- NaN for a class whose union is empty, skipped by the nanmean."""

    def __init__(self, class_names):
        self.class_names = class_names
        self.hist_list = []
        self.device_hist = None  # int64 [C * C] on the device the CUDA frames came from

    @staticmethod
    def fast_hist(preds, labels, num_classes):
        """iou_metric.py:21-37 (np.int, gone from numpy >= 1.24, is int64 here)."""
        preds = np.asarray(preds).astype(np.int64)
        labels = np.asarray(labels).astype(np.int64)
        k = (labels >= 0) & (labels < num_classes)
        bin_count = np.bincount(num_classes * labels[k] + preds[k], minlength=num_classes ** 2)
        return bin_count[:num_classes ** 2].reshape(num_classes, num_classes)

    @staticmethod
    def per_class_iou(hist):
        """iou_metric.py:39-48."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))

    def hist_on(self, device):
        """The device confusion matrix (created on first use), flattened [C * C] int64."""
        c = len(self.class_names)
        if self.device_hist is None:
            self.device_hist = torch.zeros((c * c,), dtype=torch.int64, device=device)
        elif self.device_hist.device != torch.device(device):
            raise ValueError(f"IOUMetric holds a confusion matrix on {self.device_hist.device}, not {device}")
        return self.device_hist

    def add(self, pred_labels, gt_labels):
        if torch.is_tensor(pred_labels) and pred_labels.is_cuda:
            gt = gt_labels if torch.is_tensor(gt_labels) else torch.from_numpy(np.asarray(gt_labels))
            gt = gt.to(pred_labels.device)
            if gt.dtype not in (torch.uint8, torch.int64):
                gt = gt.long()
            ops.argmax_confusion(pred_in=pred_labels.reshape(-1), n_classes=len(self.class_names), labels=gt.reshape(-1),
                                 hist=self.hist_on(pred_labels.device), want_pred=False)
            return
        preds = pred_labels.cpu().numpy() if torch.is_tensor(pred_labels) else np.asarray(pred_labels)
        labels = gt_labels.cpu().numpy() if torch.is_tensor(gt_labels) else np.asarray(gt_labels)
        self.hist_list.append(self.fast_hist(preds.reshape(-1), labels.reshape(-1), len(self.class_names)))

    @staticmethod
    def reduce_tensor(tensor):
        rt = tensor.clone()
        dist.all_reduce(rt, op=dist.ReduceOp.SUM)
        return rt

    def confusion_matrix(self):
        """This process's confusion matrix (host + device parts), int64 numpy [C, C]."""
        c = len(self.class_names)
        hist = np.zeros((c, c), dtype=np.int64)
        for h in self.hist_list:
            hist += h
        if self.device_hist is not None:
            hist += self.device_hist.cpu().numpy().reshape(c, c)
        return hist

    def get_metric(self):
        hist = self.confusion_matrix()
        if dist.is_available() and dist.is_initialized():
            t = torch.from_numpy(hist)
            if dist.get_backend() == "nccl":  # RCCL reduces device tensors only
                t = t.to(self.device_hist.device if self.device_hist is not None else torch.device("cuda"))
            hist = self.reduce_tensor(t).cpu().numpy()
        iou = self.per_class_iou(hist)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # all classes absent: the mean of nothing is NaN
            miou = float(np.nanmean(iou))
        return {"mIOU": miou, "IOU": {self.class_names[i]: float(iou[i]) for i in range(len(self.class_names))}}


def _cartesian_rows(points, dataset):
    """Frame rows without the batch column -> cartesian [x, y, z, f..].  Cylinder configs collate polar rows
    [rho, phi, z, x, y, f..] (waymo_dataset.py:270-273); their x, y, z are recovered exactly, so the views are cartesian
    and the cylinder conversion runs after them, where prepare_data / batch_from_resident put it."""
    if getattr(dataset, "use_cylinder", False) and points.shape[1] == dataset.dim_point + 2:
        cols = [3, 4, 2] + list(range(5, points.shape[1]))
        return points[:, cols]
    return points


def _current_row_count(data_dict):
    """point_id_offset[-1] of a one-frame batch: the python ints of the device batch builders where they are there
    (no read-back), else the collated array or tensor."""
    offsets = data_dict.get("point_row_offsets")
    if offsets is None:
        offsets = data_dict["point_id_offset"]
        offsets = offsets.tolist() if torch.is_tensor(offsets) else np.asarray(offsets).reshape(-1).tolist()
    return int(offsets[-1])


class MultiScaleFlipAug:
    """test_time_aug.py:6-43, same constructor and attributes.  ``__call__`` is the reference's list form (one collated
    dict per view, built by the library's host views routine, then ``dataset.prepare_data`` / ``collate_batch``);
    ``predict`` is the device path."""

    def __init__(self, dataset, scales=None, angles=None, flip_x=False, flip_y=False):
        self.dataset = dataset
        self.scales = scales
        self.angles = angles
        self.flip_x = [True, False] if flip_x else [False]
        self.flip_y = [True, False] if flip_y else [False]

    @property
    def n_views(self):
        return len(self.scales) * len(self.angles) * len(self.flip_x) * len(self.flip_y)

    def table(self, batch_period=0):
        return ops.tta_table(self.scales, self.angles, self.flip_x, self.flip_y, batch_period)

    def __call__(self, data):
        """Call function to apply test time augment transforms on results (test_time_aug.py:15-35).  Image features
        are carried only when the frame has them (the reference indexes them unconditionally)."""
        points = np.asarray(data["points"])[:, 1:]
        frame = np.ascontiguousarray(_cartesian_rows(points, self.dataset), dtype=np.float32)
        views = ops.tta_views_host(frame, self.table())
        n = frame.shape[0]
        # multi-sweep: prepare_data reads cur_point_indices (waymo_dataset.py:266), which the reference's views lack; the
        # views keep the lag column, so the current rows of every view are the frame's
        cur = np.flatnonzero(frame[:, 3] == 0) if getattr(self.dataset, "use_multi_sweeps", False) else None
        aug_data_list = []
        for v in range(self.n_views):
            new_data = dict()
            if data.get("point_image_features") is not None:
                new_data["point_image_features"] = np.array(data["point_image_features"], copy=True)
            if cur is not None:
                new_data["cur_point_indices"] = cur.copy()
            new_data["points"] = views[v * n:(v + 1) * n, 1:].copy()
            new_data = self.dataset.prepare_data(new_data)
            new_data = self.dataset.collate_batch([new_data])
            aug_data_list.append(new_data)
        return aug_data_list

    def check_views_per_forward(self, views_per_forward, batch_size=1):
        k = DEFAULT_VIEWS_PER_FORWARD if views_per_forward is None else int(views_per_forward)
        k = min(k, self.n_views) if views_per_forward is None else k
        if not 1 <= k <= self.n_views:
            raise ValueError(f"views_per_forward={k}: 1 .. {self.n_views} (the number of views)")
        if k * batch_size > MAX_BATCH:
            raise ValueError(f"views_per_forward={k} x batch {batch_size} scenes exceeds the kernels' {MAX_BATCH}")
        return k

    @staticmethod
    def _view_current_rows(points, j, n, cur):
        """The rows of view ``j`` of a collated K-view batch that the model's point branch reads, without the batch
        column: all ``n`` of them, or the current ones of a multi-sweep frame."""
        rows = points[j * n:(j + 1) * n, 1:]
        return rows if cur is None else rows[cur]

    def accumulate(self, model, data_dict, views_per_forward=None):
        """Sum over the views of the per-view softmax, float32 [N, C] on the device, and the number of views.  For a
        multi-sweep dataset a view transforms every row, current and history, and N is the number of current rows (lag
        column exactly 0, the model's own rule), in their order in the frame."""
        if model.training:
            raise RuntimeError("MultiScaleFlipAug.predict needs model.eval(): DropPath / dropout would randomize the views")
        multi = bool(getattr(self.dataset, "use_multi_sweeps", False))
        if multi and data_dict.get("point_id_offset") is None:
            raise NotImplementedError("test-time augmentation of a multi-sweep frame needs its point_id_offset (the number "
                                      "of current-sweep rows; collate_batch, assemble and batch_from_resident all set it)")
        bs = int(data_dict.get("batch_size", 1))
        if bs != 1:
            raise ValueError(f"MultiScaleFlipAug.predict takes one frame, got batch_size={bs} (the reference's "
                             "points[:, 1:] would merge the frames)")
        k_per = self.check_views_per_forward(views_per_forward)
        pts = data_dict["points"]
        if isinstance(pts, np.ndarray):
            pts = torch.from_numpy(np.ascontiguousarray(pts))
        dev = pts.device if pts.is_cuda else torch.device("cuda", torch.cuda.current_device())
        frame = _cartesian_rows(pts[:, 1:], self.dataset).to(device=dev, dtype=torch.float32).contiguous()
        img = data_dict.get("point_image_features")
        if img is not None:
            img = (torch.from_numpy(img) if isinstance(img, np.ndarray) else img).to(device=dev, dtype=torch.float32)
        n, n_views = frame.shape[0], self.n_views
        n_out, cur, cur_rows = n, None, None
        if multi:
            # the current rows, found once per frame (nonzero reads their count back); view j of a forward has them at
            # j * N + cur, which travels with the batch so that the model does not search each forward again
            cur = torch.nonzero(frame[:, 3] == 0).view(-1)
            n_out = int(cur.shape[0])
            want = _current_row_count(data_dict)
            if n_out != want:
                raise ValueError(f"{n_out} rows of the frame have time lag 0, point_id_offset says {want} current rows")
            cur_rows = (torch.arange(k_per, device=dev).view(-1, 1) * n + cur.view(1, -1)).reshape(-1)
        views = ops.tta_views(frame, self.table(batch_period=k_per))  # all views, one launch; column 0 = v % K
        cylinder = bool(getattr(self.dataset, "use_cylinder", False))
        vs = [float(v) for v in self.dataset.voxel_size]
        pcr = [float(v) for v in self.dataset.point_cloud_range]
        # DeepFusion's neighbour search, planned here view by view.  The search strides the [N, D] rows by 3 floats, as the
        # reference's kernel does (ops.knn_query), so in a batch of K frames the segment of frame j > 0 lies over other
        # frames' rows: searched with the batch, a view's neighbours would depend on K.  Each view is searched alone, in its
        # own coordinates, exactly as its batch-1 forward searches it, and its rows are shifted to its place in the batch.
        search = getattr(getattr(model, "deep_fusion", None), "neighbours", None) if img is not None else None
        one = torch.tensor([n_out], dtype=torch.int32, device=dev)
        acc = None
        with torch.no_grad():
            for k0 in range(0, n_views, k_per):
                k = min(k_per, n_views - k0)
                b = B.batch_from_resident(views[k0 * n:(k0 + k) * n], [n_out * (j + 1) for j in range(k)], vs, pcr,
                                          None if img is None else img.repeat(k, 1), cylinder)
                if multi:
                    b["cur_rows"] = cur_rows[:k * n_out]
                if search is not None:
                    b["fusion_knn"] = torch.cat([search(self._view_current_rows(b["points"], j, n, cur), one) + j * n_out
                                                 for j in range(k)])
                logits = model(b)["point_out"]
                if acc is None:
                    acc = torch.empty((n_out, logits.shape[1]), dtype=torch.float32, device=dev)
                ops.softmax_accumulate(logits, acc, first=k0 == 0)
        return acc, n_views

    def predict(self, model, data_dict, views_per_forward=None):
        """Mean over the views of softmax(point_out), float32 [N, C] on the device (eval.py:43-52)."""
        acc, n_views = self.accumulate(model, data_dict, views_per_forward)
        return acc / n_views

    def __repr__(self):
        repr_str = self.__class__.__name__
        repr_str += f'(scales={self.scales}, '
        repr_str += f'(angles={self.angles}, '
        repr_str += f'(flip_x={self.flip_x}, '
        repr_str += f'(flip_y={self.flip_y}'
        return repr_str


def segment_frame(model, data_dict, augmentor=None, metric=None, views_per_forward=None):
    """Predicted labels, int64 [N] on the device (eval.py:41-58): the argmax of the logits, or with ``augmentor`` of
    the mean probability over its views.  When ``metric`` is given and the frame has ``point_labels``, the same launch
    adds the frame to the metric's device confusion matrix."""
    if augmentor is None:
        d = load_data_to_gpu({k: v for k, v in data_dict.items() if k != "point_labels"})
        with torch.no_grad():
            scores = model(d)["point_out"]
        n_views = 0
    else:
        scores, n_views = augmentor.accumulate(model, data_dict, views_per_forward)
    labels = data_dict.get("point_labels")
    hist = None
    if metric is not None and labels is not None:
        labels = torch.from_numpy(np.asarray(labels)) if not torch.is_tensor(labels) else labels
        labels = labels.to(scores.device).reshape(-1)
        if labels.dtype not in (torch.uint8, torch.int64):
            labels = labels.long()
        hist = metric.hist_on(scores.device)
    else:
        labels = None
    return ops.argmax_confusion(scores.float(), labels=labels, hist=hist, n_views=n_views)


def segment_test_frame(model, batch, augmentor=None, n_classes=None, views_per_forward=None):
    """``semseg_for_one_frame`` of tools/test.py:37-61 without the protobuf: the frame's predicted labels (argmax of the
    logits, or of ``MultiScaleFlipAug``'s mean probability) written into the two range images of the top lidar on the device (seg3d_range_image_labels; submission.py:27-41).  ``batch``: one frame with ``points_ri``
    and ``filename``, as ``WaymoDataset(mode='testing')`` delivers it.  Returns ``context_name``,
    ``frame_timestamp_micros`` and the int32 [64, 2650, 2] numpy images ``ri_return1`` / ``ri_return2``; packing them
    into Waymo's SegmentationFrame proto needs ``waymo_open_dataset`` and is left to the caller."""
    if int(batch.get("batch_size", 1)) != 1:
        raise ValueError("segment_test_frame takes one frame (tools/test.py reads filename[0])")
    ri = batch["points_ri"]
    name = batch["filename"][0] if isinstance(batch["filename"], (list, tuple)) else batch["filename"]
    pred = segment_frame(model, {k: v for k, v in batch.items() if k not in ("points_ri", "point_labels")}, augmentor,
                         views_per_forward=views_per_forward)
    if not torch.is_tensor(ri):
        ri = torch.from_numpy(np.ascontiguousarray(ri, dtype=np.int32))
    ri = ri.to(device=pred.device, dtype=torch.int32)
    img1, img2 = ops.range_image_labels(pred, ri, 254 if n_classes is None else int(n_classes))
    context_name, timestamp = name.split('-')[:2]
    return {"context_name": context_name, "frame_timestamp_micros": int(timestamp),
            "ri_return1": img1.cpu().numpy(), "ri_return2": img2.cpu().numpy()}


def evaluate(model, frames, class_names, augmentor=None, views_per_forward=None):
    """tools/eval.py:35-64: every frame through segment_frame, scored by IOUMetric; returns get_metric()."""
    model.eval()
    metric = IOUMetric(class_names)
    for data_dict in frames:
        segment_frame(model, data_dict, augmentor, metric, views_per_forward)
    return metric.get_metric()
