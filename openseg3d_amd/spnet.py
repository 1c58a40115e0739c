"""SPNet: the reference's second segmentor on the same kernels.

  seg3d/models/segmentors/spnet.py:12-148         SPNet (point MLPs + SparseUnet + fusion head)
  seg3d/models/backbones/spconv_unet.py:12-233    SparseBasicBlock (optional SE), UpBlock, SparseUnet
  seg3d/models/layers/ocr.py:10-116               SpatialGatherModule, ObjectAttentionBlock, OCRLayer

Same constructor arguments, ``forward(batch_dict) -> OrderedDict`` contract and state_dict keys / shapes as the
reference (tests/golden/spnet_keys.json).  This file holds what only SPNet has: the object-context layers and the
SparseUnet backbone.  SparseBasicBlock, UpBlock and everything around the backbone (segformer.Segmentor: construction,
prepare_batch, forward) are Segformer's own objects, so every sparse convolution, BatchNorm(+ReLU) pass, voxel reduce
and voxel->point gather runs in libseg3d_hip.so exactly as there; the object-context attention works on
[voxels of the stride-8 level] x [22 class proxies] matrices and stays on torch.
"""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from . import spconv
from .segformer import (ConvBnAct, FusedMLP, RowLinear, SALayer, Segmentor, SparseBasicBlock, UpBlock,  # SALayer: re-exported
                        conv_module)


class SpatialGatherModule(nn.Module):
    """Class proxies of one sample: softmax of the coarse class scores over the sample's voxels, times the features
    (ocr.py:10-36)."""

    def __init__(self, scale):
        super().__init__()
        self.scale = scale

    def forward(self, feats, probs, batch_size, batch_indices, offsets=None):
        if offsets is not None and feats.is_cuda and ops.class_context_fits(probs.shape[1], feats.shape[1]):
            # samples are row spans: one segmented softmax-matmul for the whole batch (seg3d_class_context_fwd / _bwd)
            return ops.class_context(feats, probs, offsets[:batch_size], self.scale)
        out = []
        for i in range(batch_size):
            sel = slice(offsets[i - 1] if i else 0, offsets[i]) if offsets is not None else batch_indices == i
            prob = F.softmax(self.scale * probs[sel].t(), dim=1)  # [classes, n_i]
            out.append(prob @ feats[sel])
        return torch.stack(out)  # [batch, classes, C]


class ObjectAttentionBlock(nn.Module):
    """Voxel-to-proxy attention (ocr.py:39-82); the BatchNorms see one sample at a time, as in the reference."""

    def __init__(self, in_channels, key_channels):
        super().__init__()
        self.key_channels = key_channels

        def proj(cin, cout):
            return FusedMLP(nn.Linear(cin, cout, bias=False), nn.BatchNorm1d(cout), nn.ReLU(inplace=True))

        self.query_project = proj(in_channels, key_channels)
        self.key_project = proj(in_channels, key_channels)
        self.value_project = proj(in_channels, key_channels)
        self.bottleneck = proj(key_channels, in_channels)

    def forward(self, x, proxy):
        query = self.query_project(x)
        key = self.key_project(proxy)
        value = self.value_project(proxy)
        sim = F.softmax((self.key_channels ** -0.5) * (query @ key.t()), dim=-1)
        return self.bottleneck(sim @ value)


class OCRLayer(nn.Module):
    """Object-contextual representation on the stride-8 level (ocr.py:85-116)."""

    def __init__(self, in_channels, mid_channels, key_channels, scale=1.0, drop=0.05):
        super().__init__()
        self.scale = scale
        self.transform_input = ConvBnAct(spconv.SubMConv3d(in_channels, mid_channels, 3, padding=1, bias=False),
                                         nn.BatchNorm1d(mid_channels), nn.ReLU(inplace=True))
        self.spatial_gather_module = SpatialGatherModule(self.scale)
        self.object_context_block = ObjectAttentionBlock(mid_channels, key_channels)
        self.bottleneck = FusedMLP(nn.Linear(mid_channels * 2, in_channels, bias=False), nn.BatchNorm1d(in_channels),
                                   nn.ReLU(inplace=True), nn.Dropout(drop))

    def forward(self, inputs, probs, batch_size):
        inputs = self.transform_input(inputs)
        feats = inputs.features
        batch_indices = inputs.indices[:, 0]
        offsets = inputs.level.sample_offsets()  # contiguous samples: slices instead of masks and scatters
        context = self.spatial_gather_module(feats, probs, batch_size, batch_indices, offsets)
        pieces, rows = [], []
        for i in range(batch_size):
            if offsets is not None:
                sel = slice(offsets[i - 1] if i else 0, offsets[i])
            else:
                sel = torch.nonzero(batch_indices == i).view(-1)
                rows.append(sel)
            pieces.append(self.object_context_block(feats[sel], context[i]))
        out = torch.cat(pieces) if batch_size > 1 else pieces[0]
        if rows:
            out = torch.empty_like(feats).index_copy(0, torch.cat(rows), out)
        feats = self.bottleneck(torch.cat([out, feats], dim=1))
        return inputs.replace_feature(feats)


class SparseUnet(nn.Module):
    """spconv_unet.py:115-233: 4-level sparse U-Net, channels 32/64/128/256, OCR on the coarsest level."""

    def __init__(self, input_channels, output_channels, grid_size, voxel_size, point_cloud_range, num_classes,
                 use_ocr=True):
        super().__init__()
        self.sparse_shape = grid_size[::-1]
        self.voxel_size, self.point_cloud_range, self.use_ocr = voxel_size, point_cloud_range, use_ocr
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        act_fn = nn.ReLU(inplace=True)
        block = partial(SparseBasicBlock, norm_fn=norm_fn, act_fn=act_fn)
        self.conv_input = conv_module(input_channels, 32, norm_fn, act_fn, "subm", "subm1")
        self.conv1 = spconv.SparseSequential(block(32, 32, indice_key="subm1"), block(32, 32, indice_key="subm1"))
        self.conv2 = spconv.SparseSequential(
            conv_module(32, 64, norm_fn, act_fn, "spconv", "spconv2"), block(64, 64, indice_key="subm2"),
            block(64, 64, indice_key="subm2"), block(64, 64, indice_key="subm2"))
        self.conv3 = spconv.SparseSequential(
            conv_module(64, 128, norm_fn, act_fn, "spconv", "spconv3"), block(128, 128, indice_key="subm3"),
            block(128, 128, indice_key="subm3"), block(128, 128, with_se=True, indice_key="subm3"))
        self.conv4 = spconv.SparseSequential(
            conv_module(128, 256, norm_fn, act_fn, "spconv", "spconv4"), block(256, 256, indice_key="subm4"),
            block(256, 256, indice_key="subm4"), block(256, 256, with_se=True, indice_key="subm4"))

        def up(inplanes, planes, conv_type, layer_id):
            # The lateral transform's conv weights are drawn a second time, behind the block's other convs: the order in which
            # this backbone has always consumed the torch generator (it used to build each transform twice).  It keeps the
            # weights a seed gives, the benchmark's and the tests' among them, what they were.
            blk = UpBlock(inplanes, planes, norm_fn, act_fn, conv_type, layer_id)
            blk.transform.conv1.reset_parameters()
            blk.transform.conv2.reset_parameters()
            return blk

        self.up4 = up(256, 128, conv_type="inverseconv", layer_id=4)
        self.up3 = up(128, 64, conv_type="inverseconv", layer_id=3)
        self.up2 = up(64, 32, conv_type="inverseconv", layer_id=2)
        self.up1 = up(32, output_channels, conv_type="subm", layer_id=1)
        if self.use_ocr:
            self.ocr = OCRLayer(256, 128, 64)
        self.aux_voxel_classifier = nn.Sequential(RowLinear(256, num_classes, bias=False))
        self.voxel_classifier = nn.Sequential(RowLinear(output_channels, num_classes, bias=False))

    def prepare(self, batch_dict):
        """All site levels, rulebooks, row orders and per-sample row offsets before the first feature kernel: the three
        host read-backs (strided level sizes) happen while only index kernels are in flight (see
        segformer.PointTransformer.prepare)."""
        level = spconv.SiteLevel(batch_dict["voxel_coords"].int(), self.sparse_shape, batch_dict["batch_size"])
        batch_dict["site_level"] = level
        # per-sample row offsets of levels 2 and 3: squeeze-excite of conv3 / conv4, OCR
        level.plan_chain(3, lambda k, level: level.sample_offsets() if k >= 2 else None)
        return batch_dict

    def forward(self, batch_dict):
        coords = batch_dict["voxel_coords"]
        x = spconv.SparseConvTensor(batch_dict["voxel_features"], coords.int(), self.sparse_shape, batch_dict["batch_size"],
                                    _level=batch_dict.get("site_level"))
        x = self.conv_input(x)
        x1 = self.conv1(x)
        x2 = self.conv2(x1)
        x3 = self.conv3(x2)
        x4 = self.conv4(x3)
        aux = self.aux_voxel_classifier(x4.features)
        batch_dict["aux_voxel_out"], batch_dict["aux_voxel_coords"] = aux, x4.indices
        if self.use_ocr:
            x4 = self.ocr(x4, aux, batch_dict["batch_size"])
        y = self.up4(x4, x4)
        y = self.up3(y, x3)
        y = self.up2(y, x2)
        y = self.up1(y, x1)
        batch_dict["voxel_features"], batch_dict["voxel_coords"] = y.features, y.indices
        batch_dict["voxel_out"] = self.voxel_classifier(y.features)
        return batch_dict


class SPNet(Segmentor):
    backbone_name, voxel_feature_channel = "voxel_encoder", 64

    def build_backbone(self, dataset):
        return SparseUnet(self.vfe.voxel_feature_channel, self.voxel_feature_channel, dataset.grid_size,
                          dataset.voxel_size, dataset.point_cloud_range, dataset.num_classes)
