#!/usr/bin/env python3
"""Test-time-augmentation evaluation, ms per frame: the reference's eval loop on this stack against the device path.

    python tools/tta_bench.py [--frames F] [--warmup W] [--ks 1,2,4,6,9,12,18,36] [--out FILE]
    python tools/tta_bench.py --profile [--k K]     # the device path only, for rocprofv3 --kernel-trace --stats
    python tools/tta_bench.py --workload multi_sweeps [--ks 1,3,6,9] [--out FILE]

--workload multi_sweeps: configs/waymo_multi_sweeps.yaml with image features at 3 and 5 sweeps on the seeded multi-sweep
scene; (a) is the list-form loop below (which the reference itself cannot run on this config), (b) segment_frame at each
K.  The result goes under the key "multi_sweeps" of FILE, whose other keys stay.

Scenes: the seeded Waymo-shaped scene (scene.make_scene, ~175 k points, configs/waymo_one_sweep.yaml) and the same
scene under the cylinder config; MultiScaleFlipAug with tools/eval.py's 36 views, Segformer with seeded weights.

(a) reference_loop: tools/eval.py:41-58 as written on this package -- MultiScaleFlipAug.__call__ (host views, host
    voxelizer through prepare_data, collate_batch), per-view load_data_to_gpu, batch-1 forward, F.softmax, then
    torch.stack + mean, argmax .cpu(), IOUMetric.fast_hist (numpy bincount);
(b) device: segment_frame(model, frame, augmentor, metric) with views_per_forward = K (the frame uploaded once, one
    views launch, K views per forward, softmax accumulation, argmax + confusion matrix on the device), with
    torch.cuda.max_memory_allocated for each K.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time
from collections import defaultdict

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd import batch as B, config, scene, segformer  # noqa: E402
from openseg3d_amd import evaluation as E  # noqa: E402

SCALES = [0.95, 1.0, 1.05]
ANGLES = [-0.78539816, 0, 0.78539816]


class HostDataset:
    """Validation-mode WaymoDataset.prepare_data / collate_batch (waymo_dataset.py:248-279, 338-376) on the library's
    host voxelizer, cylinder rows through scene.cart2polar_rows (numpy, as pointops_utils.cart2polar)."""

    def __init__(self, ds):
        self.spec = ds
        self.use_cylinder, self.use_multi_sweeps, self.dim_point = ds.use_cylinder, ds.use_multi_sweeps, ds.dim_point
        self.voxel_size, self.point_cloud_range = ds.voxel_size, ds.point_cloud_range
        self.voxel_generator = B.VoxelGenerator(ds.voxel_size, ds.point_cloud_range)

    def prepare_data(self, d):
        d["cur_point_count"] = d["cur_point_indices" if self.use_multi_sweeps else "points"].shape[0]
        if self.use_cylinder:
            d["points"] = scene.cart2polar_rows(d["points"])
        d["voxel_coords"], d["point_voxel_ids"] = self.voxel_generator.generate(d["points"])
        return d

    @staticmethod
    def collate_batch(batch_list):
        data = defaultdict(list)
        for cur in batch_list:
            for k, v in cur.items():
                data[k].append(v)
        ret = {k: np.concatenate([np.pad(c, ((0, 0), (1, 0)), constant_values=i) for i, c in enumerate(data[k])])
               for k in ("points", "voxel_coords")}
        if "point_image_features" in data:
            ret["point_image_features"] = np.concatenate(data["point_image_features"])
        ids, count, off = [], 0, []
        for i, pv in enumerate(data["point_voxel_ids"]):
            ids.append(np.where(pv != -1, pv + count, -1))
            count += data["voxel_coords"][i].shape[0]
            off.append(count)
        ret["point_voxel_ids"] = np.concatenate(ids)
        ret["voxel_id_offset"] = np.array(off)
        ret["point_id_offset"] = np.cumsum(data["cur_point_count"])
        ret["batch_size"] = len(batch_list)
        return ret


def setup(cyl, dev):
    cfg = config.default_cfg()
    if cyl:  # configs/waymo_one_sweep_cylinder.yaml:2-4
        cfg.DATASET.USE_CYLINDER = True
        cfg.DATASET.POINT_CLOUD_RANGE = [0, -3.1415926, -2, 75.2, 3.1415926, 5.2]
        cfg.DATASET.VOXEL_SIZE = [0.05, 0.012, 0.1]
    ds = config.DatasetSpec(cfg)
    torch.manual_seed(0)
    model = segformer.build_segmentor(cfg, ds).to(dev).eval()
    frame = scene.make_scene(0)
    rs = np.random.RandomState(0)
    labels = rs.randint(0, ds.num_classes, frame.shape[0]).astype(np.uint8)
    data = {"points": np.pad(frame, ((0, 0), (1, 0))), "point_labels": labels, "batch_size": 1}
    return model, HostDataset(ds), data


def setup_multi(n_sweeps, dev):
    """configs/waymo_multi_sweeps.yaml with image features at ``n_sweeps`` sweeps: the seeded multi-sweep scene
    (scene.make_multi_sweep_scene: the 175 k-point current sweep plus re-posed history sweeps of ~105 k points)."""
    cfg = config.default_cfg()
    cfg.DATASET.USE_MULTI_SWEEPS = cfg.DATASET.USE_IMAGE_FEATURE = True
    cfg.DATASET.NUM_SWEEPS = n_sweeps
    ds = config.DatasetSpec(cfg)
    torch.manual_seed(0)
    model = segformer.build_segmentor(cfg, ds).to(dev).eval()
    rows, n_cur = scene.make_multi_sweep_scene(0, n_sweeps)
    rs = np.random.RandomState(0)
    labels = rs.randint(0, ds.num_classes, n_cur).astype(np.uint8)
    data = {"points": np.pad(rows, ((0, 0), (1, 0))), "point_labels": labels, "batch_size": 1,
            "point_image_features": scene.make_image_features(0, n_cur, ds.dim_image_feature),
            "point_id_offset": np.array([n_cur])}
    return model, HostDataset(ds), data


def multi_sweeps(args, dev):
    """--workload multi_sweeps: (a) the list-form loop, which the reference itself cannot run on this config
    (test_time_aug.py:23-24 drops cur_point_indices), against (b) segment_frame at K views per forward."""
    out = {"views": 36, "image_features": True, "default_views_per_forward": E.DEFAULT_VIEWS_PER_FORWARD,
           "device_name": torch.cuda.get_device_name(dev),
           "device_memory_gib": torch.cuda.get_device_properties(dev).total_memory / 2**30}
    for n_sweeps in (3, 5):
        model, hds, data = setup_multi(n_sweeps, dev)
        aug = E.MultiScaleFlipAug(hds, scales=SCALES, angles=ANGLES, flip_x=True, flip_y=True)
        n_classes = hds.spec.num_classes
        names = [f"c{i}" for i in range(n_classes)]
        resident = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in data.items()}
        r = {"n_rows": int(data["points"].shape[0]), "n_current": int(data["point_id_offset"][-1])}
        hist_a = reference_loop(model, aug, data, n_classes)
        r["list_form_loop_ms"] = timed(lambda: reference_loop(model, aug, data, n_classes), args.frames, args.warmup, dev)
        r["device"] = {}
        for k in [int(x) for x in args.ks.split(",")]:
            metric = E.IOUMetric(names)
            torch.cuda.synchronize(dev)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            E.segment_frame(model, resident, aug, metric, k)
            torch.cuda.synchronize(dev)
            peak = torch.cuda.max_memory_allocated(dev)
            ms = timed(lambda: E.segment_frame(model, resident, aug, metric, k), args.frames, args.warmup, dev)
            m1 = E.IOUMetric(names)
            E.segment_frame(model, data, aug, m1, k)
            r["device"][str(k)] = {"ms": ms, "peak_mib": peak / 2**20,
                                   "hist_points_differing_from_loop": int(np.abs(m1.confusion_matrix() - hist_a).sum() // 2)}
        best = min(r["device"], key=lambda k: r["device"][k]["ms"])
        r["best_k"] = int(best)
        r["speedup_best_vs_list_form_loop"] = r["list_form_loop_ms"] / r["device"][best]["ms"]
        out[f"sweeps{n_sweeps}"] = r
        del model
        torch.cuda.empty_cache()
    return out


def reference_loop(model, aug, data_dict, n_classes):
    """tools/eval.py:41-58, the --tta branch."""
    point_out_list = []
    aug_data_list = aug(data_dict)
    for aug_data in aug_data_list:
        E.load_data_to_gpu(aug_data)
        with torch.no_grad():
            result = model(aug_data)
        point_out_list.append(F.softmax(result["point_out"], dim=1))
    point_out = torch.mean(torch.stack(point_out_list, dim=0), dim=0)
    pred = torch.argmax(point_out, dim=1).cpu()
    return E.IOUMetric.fast_hist(pred.numpy(), data_dict["point_labels"], n_classes)


def timed(fn, frames, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(frames):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ks", default=None, help="default 1,2,4,6,9,12,18,36; multi_sweeps: 1,3,6,9")
    ap.add_argument("--workload", default="single_sweep", choices=["single_sweep", "multi_sweeps"])
    ap.add_argument("--scenes", default="one_sweep,cylinder")
    ap.add_argument("--profile", action="store_true", help="device path only (rocprofv3 run)")
    ap.add_argument("--k", type=int, default=None, help="--profile: views per forward (default: the package default)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.workload == "multi_sweeps":
        args.ks = args.ks or "1,3,6,9"
        res = {"tool": "tta_bench"}
        if args.out and os.path.exists(args.out):  # the other workload's keys stay
            with open(args.out) as f:
                res = json.loads(f.read())
        res["multi_sweeps"] = multi_sweeps(args, dev)
        line = json.dumps(res)
        print(json.dumps({"tool": "tta_bench", "multi_sweeps": res["multi_sweeps"]}))
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    args.ks = args.ks or "1,2,4,6,9,12,18,36"
    res = {"tool": "tta_bench", "views": 36, "default_views_per_forward": E.DEFAULT_VIEWS_PER_FORWARD,
           "device_name": torch.cuda.get_device_name(dev), "scenes": {}}
    for name in args.scenes.split(","):
        model, hds, data = setup(name == "cylinder", dev)
        aug = E.MultiScaleFlipAug(hds, scales=SCALES, angles=ANGLES, flip_x=True, flip_y=True)
        n_classes = hds.spec.num_classes
        names = [f"c{i}" for i in range(n_classes)]
        resident = {"points": torch.from_numpy(data["points"]).to(dev), "batch_size": 1,
                    "point_labels": torch.from_numpy(data["point_labels"]).to(dev)}
        r = {"n_points": int(data["points"].shape[0])}
        if args.profile:
            metric = E.IOUMetric(names)
            r["device_ms"] = timed(lambda: E.segment_frame(model, resident, aug, metric, args.k), args.frames,
                                   args.warmup, dev)
            res["scenes"][name] = r
            continue
        hist_a = reference_loop(model, aug, data, n_classes)
        r["reference_loop_ms"] = timed(lambda: reference_loop(model, aug, data, n_classes), args.frames, args.warmup, dev)
        r["device"] = {}
        for k in [int(x) for x in args.ks.split(",")]:
            try:
                metric = E.IOUMetric(names)
                torch.cuda.synchronize(dev)
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats(dev)
                E.segment_frame(model, resident, aug, metric, k)
                torch.cuda.synchronize(dev)
                peak = torch.cuda.max_memory_allocated(dev)
                ms = timed(lambda: E.segment_frame(model, resident, aug, metric, k), args.frames, args.warmup, dev)
                m1 = E.IOUMetric(names)  # the numpy frame, as the loader hands it over
                E.segment_frame(model, data, aug, m1, k)
                entry = {"ms": ms, "peak_mib": peak / 2**20,
                         "hist_equals_reference_loop": bool(np.array_equal(m1.confusion_matrix(), hist_a)),
                         "hist_points_differing": int(np.abs(m1.confusion_matrix() - hist_a).sum() // 2)}
            except torch.cuda.OutOfMemoryError:
                entry = {"oom": True}
                torch.cuda.empty_cache()
            r["device"][str(k)] = entry
        ok = {k: v["ms"] for k, v in r["device"].items() if "ms" in v}
        if ok:
            best = min(ok, key=ok.get)
            r["best_k"] = int(best)
            r["speedup_best_vs_reference_loop"] = r["reference_loop_ms"] / ok[best]
        res["scenes"][name] = r
        del model
        torch.cuda.empty_cache()
    if args.out and os.path.exists(args.out):  # the other workload's key stays
        with open(args.out) as f:
            old = json.loads(f.read())
        if "multi_sweeps" in old:
            res["multi_sweeps"] = old["multi_sweeps"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
