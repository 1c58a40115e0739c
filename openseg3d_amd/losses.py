"""Training criterion of the reference on device.

  seg3d/models/builder.py:26-40                          build_criterion: MODEL.LOSSES = {'ohem_ce': 1.0, 'lovasz': 1.0}
  seg3d/models/losses/ohem_cross_entropy_loss.py:5-38    OHEMCrossEntropyLoss
  seg3d/models/losses/lovasz_loss.py:215-290             LovaszLoss
  seg3d/models/losses/focal_loss.py:6-105                FocalLoss
  seg3d/models/losses/dice_loss.py:9-43, 46-127          DiceLoss (seg3d/utils/loss_utils.py:9-22, 43-73)
  tools/train.py:71-110                                  compute_loss (point, voxel and 0.4 x auxiliary terms)

Same class names, constructor arguments and ``loss_name`` properties.  The configurations build_criterion can produce
(OHEM by probability threshold, multi-class Lovasz over the whole batch) run in libseg3d_hip.so: one pass each way for
the cross-entropy terms, one device sort for all classes of the Lovasz term -- and compute_loss, given such a list, makes one
call for all heads and both terms (ops.fused_criterion, same bits).  The cross-entropy options the reference's builder
never sets -- class weights (nn.CrossEntropyLoss(weight=), OHEMCrossEntropyLoss(class_weight=)) and OHEM by keep_ratio, an
exact device-side selection of the hardest rows without a read-back -- run in the library as well on CUDA float32 inputs
(seg3d_ce_select_fwd / _bwd; build_criterion keys 'weighted_ce' and 'ohem_ce_ratio', which consume DATASET.CLASS_WEIGHT
and MODEL.OHEM_KEEP_RATIO), as terms of compute_loss's per-term loop.  Per-image / binary Lovasz are composed from torch
ops on the same device tensors.  FocalLoss and DiceLoss, which no configuration of the reference builds but its package
exports, run in the library too on CUDA float32 inputs (build_criterion keys 'focal' and 'dice', beyond the reference's
three); other inputs take a torch composition of the same formulas.
"""
import contextlib
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


class _ClassWeightCache:
    """The class weights as a float32 tensor on the logits' device, uploaded once per device instead of per call."""

    def _device_weight(self, device):
        if self.class_weight is None:
            return None
        cache = self.__dict__.setdefault("_weight_cache", {})
        if device not in cache:
            w = self.class_weight
            cache[device] = torch.as_tensor(w if torch.is_tensor(w) else np.asarray(w), dtype=torch.float32).to(device)
        return cache[device]

    def _weight_like(self, inputs):
        """For the torch compositions: the weights in the logits' dtype, on their device."""
        w = self.class_weight
        if w is None:
            return None
        return w.to(inputs) if torch.is_tensor(w) else inputs.new_tensor(np.asarray(w))


class CrossEntropyLoss(nn.Module, _ClassWeightCache):
    """nn.CrossEntropyLoss(ignore_index=...) (builder.py:29-30) through seg3d_cross_entropy_fwd/bwd.  ``class_weight`` (a
    list, or the path of an .npy file): nn.CrossEntropyLoss(weight=..., ignore_index=...), the mean weighted by the
    targets' class weights, through seg3d_ce_select_fwd/bwd on CUDA float32 inputs and F.cross_entropy elsewhere."""

    def __init__(self, ignore_index=255, class_weight=None, loss_name="loss_cross_entropy"):
        super().__init__()
        self.ignore_index = ignore_index
        self.class_weight = get_class_weight(class_weight)
        self._loss_name = loss_name

    def forward(self, inputs, targets):
        if self.class_weight is None:
            return ops.cross_entropy(inputs, targets, ignore_index=self.ignore_index)
        if ops._loss_args_ok(inputs, targets, 4096):
            return ops.cross_entropy_select(inputs, targets, ignore_index=self.ignore_index,
                                            class_weight=self._device_weight(inputs.device), weighted_mean=True)
        return F.cross_entropy(inputs, targets, weight=self._weight_like(inputs), ignore_index=self.ignore_index)

    @property
    def loss_name(self):
        return self._loss_name


class OHEMCrossEntropyLoss(nn.Module, _ClassWeightCache):
    """ohem_cross_entropy_loss.py:5-38.  keep_ratio wins over keep_thresh (the reference's if / elif).  Without class
    weights and without keep_ratio: seg3d_cross_entropy_fwd/bwd.  With either, CUDA float32 inputs run in
    seg3d_ce_select_fwd/bwd (keep_ratio: an exact device-side selection of the int(n_valid * keep_ratio) largest losses,
    no read-back); other inputs (CPU, float64) take the torch composition of the reference's lines.  Equal losses at the
    keep_ratio cut are taken in row order on both paths (a stable sort; the reference's own sort leaves it open, the
    value does not depend on it).  The mean over nothing is 0 on the kernel paths (NaN in torch)."""

    def __init__(self, keep_ratio=None, keep_thresh=None, ignore_index=255, class_weight=None,
                 loss_name="loss_ohem_cross_entropy"):
        super().__init__()
        self.keep_ratio, self.keep_thresh = keep_ratio, keep_thresh
        self.ignore_index, self.class_weight = ignore_index, get_class_weight(class_weight)
        self._loss_name = loss_name

    def forward(self, inputs, targets):
        if self.class_weight is None and not self.keep_ratio:
            # keep_thresh (what build_criterion passes) or plain CE: fused kernel, no [n, C] softmax materialised
            return ops.cross_entropy(inputs, targets, ignore_index=self.ignore_index, keep_thresh=self.keep_thresh)
        if ops._loss_args_ok(inputs, targets, 4096):
            return ops.cross_entropy_select(inputs, targets, ignore_index=self.ignore_index,
                                            class_weight=self._device_weight(inputs.device), keep_ratio=self.keep_ratio,
                                            keep_thresh=self.keep_thresh)
        mask = targets != self.ignore_index
        losses = F.cross_entropy(inputs, targets, weight=self._weight_like(inputs), ignore_index=self.ignore_index,
                                 reduction="none")[mask]
        if self.keep_ratio:  # ohem_cross_entropy_loss.py:27-30: the hardest keep_ratio of the valid rows
            kept = int(losses.shape[0] * self.keep_ratio)
            losses = losses[torch.sort(losses, descending=True, stable=True)[1][:kept]]
        elif self.keep_thresh:
            probs = F.softmax(inputs, dim=1)[mask].gather(1, targets[mask].unsqueeze(1)).squeeze(1)
            losses = losses[probs < self.keep_thresh]
        return losses.mean()

    @property
    def loss_name(self):
        return self._loss_name


def _lovasz_grad(gt_sorted):
    """lovasz_loss.py:13-26 (used by the torch-composed variants only)."""
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.float().cumsum(0)
    union = gts + (1 - gt_sorted).float().cumsum(0)
    jaccard = 1.0 - intersection / union
    if gt_sorted.shape[0] > 1:
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
    return jaccard


def _lovasz_hinge_flat(logits, labels):
    """lovasz_loss.py:56-76."""
    if labels.numel() == 0:
        return logits.sum() * 0.0
    signs = 2.0 * labels.float() - 1.0
    errors_sorted, perm = torch.sort(1.0 - logits * signs, dim=0, descending=True)
    return torch.dot(F.relu(errors_sorted), _lovasz_grad(labels[perm]))


class LovaszLoss(nn.Module):
    def __init__(self, loss_type="multi_class", classes="present", per_image=False, reduction="none", class_weight=None,
                 loss_weight=1.0, ignore_index=255, loss_name="loss_lovasz"):
        super().__init__()
        assert loss_type in ("binary", "multi_class")
        if not per_image:
            assert reduction == "none", "reduction should be 'none' when per_image is False."
        self.loss_type, self.classes, self.per_image, self.reduction = loss_type, classes, per_image, reduction
        self.class_weight, self.loss_weight, self.ignore_index = class_weight, loss_weight, ignore_index
        self._loss_name = loss_name

    def forward(self, cls_score, label, avg_factor=None, reduction_override=None):
        """cls_score [n, C] logits, label [n].  The reference feeds the rows as a [n, C, 1, 1] image batch, so
        per_image=True means one loss per ROW (lovasz_loss.py:278-287)."""
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        if self.loss_type == "multi_class" and not self.per_image:
            return self.loss_weight * ops.lovasz_softmax(cls_score, label, self.ignore_index, self.classes, self.class_weight)
        if self.loss_type == "binary" and not self.per_image:
            valid = label.view(-1) != self.ignore_index
            return self.loss_weight * _lovasz_hinge_flat(cls_score.view(-1)[valid], label.view(-1)[valid])
        raise NotImplementedError("LovaszLoss(per_image=True) on [n, C] rows degenerates to one loss per row; "
                                  "no configuration of the reference uses it")

    @property
    def loss_name(self):
        return self._loss_name


def get_class_weight(class_weight):
    """loss_utils.py:9-22: a list is taken as given, a str is the path of an .npy file."""
    if isinstance(class_weight, str):
        if not class_weight.endswith(".npy"):
            raise ValueError("unsupported class weight file format")
        class_weight = np.load(class_weight)
    return class_weight


def _on_device_path(inputs, targets):
    return (inputs.is_cuda and inputs.dtype == torch.float32 and inputs.dim() == 2 and inputs.shape[1] <= 64
            and targets.dtype == torch.int64 and targets.dim() == 1)


class FocalLoss(nn.Module, _ClassWeightCache):
    """focal_loss.py:6-105.  CUDA float32 [n, C <= 64] logits with reduction 'mean' / 'sum' run in seg3d_focal_loss_fwd /
    _bwd; anything else (CPU, float64, reduction 'none' with its [n_valid, C] result) is composed from torch ops.
    Deviations: num_classes = -1 means "C of the logits" (the reference hands -1 to one_hot, which then infers the
    width from the largest label present); on the kernel path a label outside [0, C) that is not ignore_index is
    skipped, where one_hot raises; 'mean' over no valid row is 0 on the kernel path (NaN in torch); the composed one-hot
    target takes the logits' dtype (focal_loss.py:77 casts it to float32, which under float64 logits leaves a float32
    BCE term: binary_cross_entropy_with_logits returns the target's dtype)."""

    def __init__(self, gamma=2.0, alpha=0.5, num_classes=-1, ignore_index=255, class_weight=None, reduction="mean",
                 loss_name="loss_focal"):
        super().__init__()
        assert reduction in ("none", "mean", "sum"), "AssertionError: reduction should be 'none', 'mean' or 'sum'"
        assert isinstance(alpha, (float, list)), "AssertionError: alpha should be of type float"
        assert isinstance(gamma, float), "AssertionError: gamma should be of type float"
        assert isinstance(loss_name, str), "AssertionError: loss_name should be of type str"
        if isinstance(alpha, list):  # focal_loss.py:82 compares self.alpha >= 0: a list cannot run there either
            raise NotImplementedError("FocalLoss: a list alpha passes the reference's assertion but not its forward")
        self.gamma, self.alpha, self.num_classes, self.ignore_index = gamma, alpha, num_classes, ignore_index
        self.class_weight, self.reduction = get_class_weight(class_weight), reduction
        self._loss_name = loss_name

    def forward(self, inputs, targets):
        num_classes = inputs.size(1) if self.num_classes < 0 else self.num_classes
        if (self.reduction != "none" and self.gamma >= 0 and num_classes == inputs.size(1)
                and _on_device_path(inputs, targets)):
            return ops.focal_loss(inputs, targets, gamma=self.gamma, alpha=self.alpha, ignore_index=self.ignore_index,
                                  class_weight=self._device_weight(inputs.device), reduction=self.reduction)
        final_weight = torch.ones(1, inputs.size(1)).type_as(inputs)
        if self.class_weight is not None:
            final_weight = final_weight * inputs.new_tensor(np.asarray(self.class_weight))
        valid_mask = targets != self.ignore_index
        inputs, targets = inputs[valid_mask], targets[valid_mask]
        p = torch.sigmoid(inputs)
        targets = F.one_hot(targets, num_classes).to(inputs.dtype)
        ce_loss = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
        p_t = p * targets + (1 - p) * (1 - targets)
        loss = ce_loss * ((1 - p_t) ** self.gamma)
        if self.alpha >= 0:
            loss = (self.alpha * targets + (1 - self.alpha) * (1 - targets)) * loss
        loss = loss * final_weight
        if self.reduction == "mean":
            loss = loss.mean()
        elif self.reduction == "sum":
            loss = loss.sum()
        return loss

    @property
    def loss_name(self):
        return self._loss_name


class DiceLoss(nn.Module, _ClassWeightCache):
    """dice_loss.py:46-127.  On [n, C] rows the reference's per-class binary dice (dice_loss.py:9-43) is a mean over all n
    rows of 1 - (2 p t v + smooth) / (p^e + t^e + smooth) with the valid mask v in the numerator only, so ``reduction``
    acts on a scalar: a no-op, except that an ``avg_factor`` divides by avg_factor + eps under 'mean' and raises under
    'sum' (loss_utils.py:43-73).  CUDA float32 [n, C <= 64] logits run in seg3d_dice_loss_fwd / _bwd, anything else is
    composed from torch ops.  An empty input gives 0 on the kernel path (NaN in torch)."""

    def __init__(self, smooth=1, exponent=2, reduction="mean", class_weight=None, loss_weight=1.0, ignore_index=255,
                 loss_name="loss_dice"):
        super().__init__()
        self.smooth, self.exponent, self.reduction = smooth, exponent, reduction
        self.class_weight = get_class_weight(class_weight)
        self.loss_weight, self.ignore_index = loss_weight, ignore_index
        self._loss_name = loss_name

    def forward(self, pred, target, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        if avg_factor is not None and reduction not in ("mean", "none"):
            raise ValueError('avg_factor can not be used with reduction="sum"')
        divide = avg_factor is not None and reduction == "mean"
        ignore_index = -(1 << 62) if self.ignore_index is None else self.ignore_index  # None: nothing is left out
        if _on_device_path(pred, target) and not (divide and avg_factor < 0):
            return ops.dice_loss(pred, target, smooth=self.smooth, exponent=self.exponent, ignore_index=ignore_index,
                                 class_weight=self._device_weight(pred.device), loss_weight=self.loss_weight,
                                 avg_factor=avg_factor if divide else None)
        p = F.softmax(pred, dim=1)
        num_classes = p.shape[1]
        one_hot = F.one_hot(torch.clamp(target.long(), 0, num_classes - 1), num_classes=num_classes)
        valid = (target != ignore_index).long().view(-1, 1)
        num = p * one_hot * valid * 2 + self.smooth
        den = p.pow(self.exponent) + one_hot.pow(self.exponent) + self.smooth
        per_class = (1 - num / den).mean(dim=0)
        if self.class_weight is not None:
            per_class = per_class * p.new_tensor(np.asarray(self.class_weight))
        keep = torch.arange(num_classes, device=p.device) != ignore_index
        loss = self.loss_weight * (per_class * keep).sum() / num_classes
        if divide:
            loss = loss / (avg_factor + torch.finfo(torch.float32).eps)
        return loss

    @property
    def loss_name(self):
        return self._loss_name


def build_criterion(cfg, dataset):
    """seg3d/models/builder.py:26-40: list of (criterion, weight) in MODEL.LOSSES order.  'focal' and 'dice' go beyond the
    reference's three keys: its package exports the two classes, its builder has no key for them.  So do 'weighted_ce'
    (CrossEntropyLoss with DATASET.CLASS_WEIGHT) and 'ohem_ce_ratio' (OHEM by MODEL.OHEM_KEEP_RATIO): two configuration
    keys the reference ships and nothing of it reads."""
    losses = []
    for name in cfg.MODEL.LOSSES:
        if name == "ce":
            criterion = CrossEntropyLoss(ignore_index=dataset.ignore_index)
        elif name == "ohem_ce":
            criterion = OHEMCrossEntropyLoss(keep_thresh=cfg.MODEL.OHEM_KEEP_THRESH, ignore_index=dataset.ignore_index)
        elif name == "weighted_ce":  # DATASET.CLASS_WEIGHT finds a consumer; an empty list means no weights
            criterion = CrossEntropyLoss(ignore_index=dataset.ignore_index,
                                         class_weight=list(cfg.DATASET.CLASS_WEIGHT) or None)
        elif name == "ohem_ce_ratio":
            criterion = OHEMCrossEntropyLoss(keep_ratio=cfg.MODEL.OHEM_KEEP_RATIO, ignore_index=dataset.ignore_index)
        elif name == "lovasz":
            criterion = LovaszLoss(ignore_index=dataset.ignore_index)
        elif name == "focal":
            criterion = FocalLoss(num_classes=dataset.num_classes, ignore_index=dataset.ignore_index)
        elif name == "dice":
            criterion = DiceLoss(ignore_index=dataset.ignore_index)
        else:
            raise NotImplementedError(name)
        losses.append((criterion, cfg.MODEL.LOSSES[name]))
    return losses


AUX_OVERLAP = os.environ.get("SEG3D_AUX_OVERLAP", "1") != "0"
# all heads and both terms in one native call (ops.fused_criterion) where the criterion list allows it; 0 = the loop below
FUSED_CRITERION = os.environ.get("SEG3D_CRITERION_FUSED", "1") != "0"


def _fused_terms(criterion):
    """(ignore_index, keep_thresh, ce weight, lovasz weight) when the list is what build_criterion makes from one of 'ce' /
    'ohem_ce' (by keep_thresh), then 'lovasz' (multi-class, whole batch, classes 'present', no class weights), or one of
    the two alone; None for any other list (focal, dice, class weights, OHEM by ratio, another order)."""
    ce = lov = None
    for fn, w in criterion:
        if lov is None and ce is None and type(fn) is CrossEntropyLoss and fn.class_weight is None:
            ce = (fn.ignore_index, None, w)
        elif (lov is None and ce is None and type(fn) is OHEMCrossEntropyLoss and fn.class_weight is None
              and not fn.keep_ratio):
            ce = (fn.ignore_index, fn.keep_thresh, w)
        elif (lov is None and type(fn) is LovaszLoss and fn.loss_type == "multi_class" and not fn.per_image
              and fn.classes == "present" and fn.class_weight is None and fn.loss_weight == 1.0):
            lov = (fn.ignore_index, w)
        else:
            return None
    if ce is None and lov is None:
        return None
    if ce is not None and lov is not None and ce[0] != lov[0]:
        return None
    weights = [t[-1] for t in (ce, lov) if t is not None]
    if not all(isinstance(w, (int, float)) for w in weights):
        return None
    return (ce[0] if ce is not None else lov[0], ce[1] if ce is not None else None,
            ce[2] if ce is not None else None, lov[1] if lov is not None else None)


def compute_loss(pred_result, data_dict, criterion, cfg):
    """tools/train.py:71-110: criterion on the point logits, the voxel logits and (x MODEL.AUX_LOSS_WEIGHT) the
    stride-8 auxiliary logits, whose ground truth is looked up by nearest fine voxel centre (ops.aux_voxel_labels)."""
    # The auxiliary labels (a kNN lookup: no gradient, independent of the other two heads) come from the planned index
    # of the batch (Segmentor.prepare_batch, both segmentors) where there is one: a gather.  Otherwise they are looked up on the second
    # stream while this one computes the point and voxel losses; the streams meet in front of the auxiliary loss.
    aux_gt = side = None
    if "aux_voxel_out" in pred_result:
        dev = pred_result["aux_voxel_out"].device
        planned = (pred_result.get("index_plan") or {}).get("aux_label_index")  # either segmentor's forward of a planned batch
        overlap = AUX_OVERLAP and dev.type == "cuda" and planned is None
        if overlap:
            main, side = torch.cuda.current_stream(dev), ops.side_stream(dev)
            side.wait_stream(main)
        with torch.no_grad(), torch.cuda.stream(side) if overlap else contextlib.nullcontext():
            aux_gt = ops.aux_voxel_labels(pred_result["voxel_coords"], pred_result["aux_voxel_coords"],
                                          data_dict["voxel_labels"], data_dict["batch_size"], cfg.DATASET.VOXEL_SIZE,
                                          cfg.DATASET.POINT_CLOUD_RANGE, index=planned)
    heads = [(pred_result["point_out"], data_dict["point_labels"], 1.0)]
    if "voxel_out" in pred_result:
        heads.append((pred_result["voxel_out"], data_dict["voxel_labels"], 1.0))
    if aux_gt is not None:
        heads.append((pred_result["aux_voxel_out"], aux_gt, cfg.MODEL.AUX_LOSS_WEIGHT))
    terms = _fused_terms(criterion) if FUSED_CRITERION else None
    if (terms is not None and all(ops._loss_args_ok(x, y, 64) and x.shape[1] == heads[0][0].shape[1] for x, y, _ in heads)
            and sum(x.numel() for x, _, _ in heads) < 1 << 31):
        def fused(hs):
            return ops.fused_criterion([h[0] for h in hs], [h[1] for h in hs], [h[2] for h in hs], ignore_index=terms[0],
                                       keep_thresh=terms[1], ce_weight=terms[2], lovasz_weight=terms[3])

        if side is None:
            return fused(heads)
        # no planned index: the lookup is under way on the second stream.  The heads in front go through one fused call
        # beside it; the auxiliary head follows through the per-term entries once the streams have met -- the same
        # sequence of float32 additions as one call over all heads (a call returns the running sum from 0)
        loss = fused(heads[:-1])
        main.wait_stream(side)
        for fn, w in criterion:
            loss = loss + cfg.MODEL.AUX_LOSS_WEIGHT * fn(pred_result["aux_voxel_out"], aux_gt) * w
        return loss
    loss = 0
    for fn, w in criterion:
        loss = loss + fn(pred_result["point_out"], data_dict["point_labels"]) * w
    if "voxel_out" in pred_result:
        voxel_gt = data_dict["voxel_labels"]
        for fn, w in criterion:
            loss = loss + fn(pred_result["voxel_out"], voxel_gt) * w
    if aux_gt is not None:
        if side is not None:
            main.wait_stream(side)
        for fn, w in criterion:
            loss = loss + cfg.MODEL.AUX_LOSS_WEIGHT * fn(pred_result["aux_voxel_out"], aux_gt) * w
    return loss
