#!/usr/bin/env python3
"""Per-point image features for a split: the query half of the reference's tools/extract_image_feature.py, with the
per-row Python loop (:84-100) replaced by the library (csrc/image_features.hip).

    python tools/extract_image_feature.py DATA_DIR WORK_DIR SPLIT PATHNAMES_FILE --maps DIR [--packed] [--device cuda|cpu]

The four positional arguments, the directory layout (``DATA_DIR/SPLIT/lidar``, ``.../image_feature``) and the frame list
(``get_image_list``: the lines of PATHNAMES_FILE, for the testing split only those named in
``3d_semseg_test_set_frames.txt``) are the reference's.  The image model is not part of this stack, so the feature maps
come from ``--maps DIR``: ``DIR/<camera_id>/<name>.npy`` holds the (C, H, W) float32 / float16 map of camera 0..4 for
frame <name>, dumped by whatever image model the user runs (the reference: ``inference_segmentor(model, img)[0]``).  A
missing file means that camera is absent for the frame, as a failed image read is in the reference (:19-21).  WORK_DIR
(the reference's model directory) is accepted and not read.

Per frame it writes ``image_feature/<name>.npy``, the reference's pickled dict, or with ``--packed``
``image_feature/<name>.npz`` (rows, feats), which ``WaymoDataset`` reads without unpickling.  ``--device cpu`` uses the
library's host entry; both give the same files.  A row that projects outside its camera's map stops the run, as the
reference's IndexError does."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd import image_features, ops  # noqa: E402

NUM_CAMERAS = 5


def get_image_list(data_dir, split, pathnames_file):
    """The frames to process: every line of ``pathnames_file``; in the testing split only the frames whose
    (context, timestamp) pair is listed in ``<data_dir>/<split>/3d_semseg_test_set_frames.txt``."""
    with open(pathnames_file, "r") as fp:
        pathnames = fp.read().splitlines()
    if split != "testing":
        return pathnames
    wanted = set()
    with open(os.path.join(data_dir, split, "3d_semseg_test_set_frames.txt"), "r") as fp:
        for line in fp.read().splitlines():
            parts = line.split(",")
            wanted.add((parts[0], parts[1]))
    if not wanted:
        return pathnames
    keep = [p for p in pathnames if tuple(os.path.basename(p).split("-")[:2]) in wanted]
    print("Total %d frames, %d image frames" % (len(wanted), len(keep)))
    return keep


def load_feature_maps(maps_dir, filename):
    """dict camera id -> (C, H, W) array of the cameras whose map file exists."""
    maps = dict()
    for camera_id in range(NUM_CAMERAS):
        path = os.path.join(maps_dir, str(camera_id), filename + ".npy")
        if not os.path.exists(path):
            print("no feature map: %s" % path)
            continue
        maps[camera_id] = np.load(path, allow_pickle=False)
    return maps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("data_dir")
    ap.add_argument("work_dir")
    ap.add_argument("split")
    ap.add_argument("pathnames_file")
    ap.add_argument("--maps", required=True, help="DIR/<camera_id>/<name>.npy, (C, H, W) per camera and frame")
    ap.add_argument("--packed", action="store_true", help="write <name>.npz (rows, feats) instead of the pickled dict")
    ap.add_argument("--device", choices=["cuda", "cpu"], default="cuda")
    ap.add_argument("--channels", type=int, default=None, help="C, needed only for frames without any camera")
    args = ap.parse_args()
    lidar_dir = os.path.join(args.data_dir, args.split, "lidar")
    feature_dir = os.path.join(args.data_dir, args.split, "image_feature")
    os.makedirs(feature_dir, exist_ok=True)
    if args.device == "cuda":
        import torch
    pathnames = get_image_list(args.data_dir, args.split, args.pathnames_file)
    for k, pathname in enumerate(pathnames):
        filename = os.path.basename(pathname).replace(".npy", "")
        maps = load_feature_maps(args.maps, filename)
        lidar = np.load(os.path.join(lidar_dir, filename + ".npy"))
        if not maps:  # every row misses: the reference stores an empty dict
            if args.packed and args.channels is None:
                raise SystemExit(f"{filename}: no camera has a feature map; the packed file needs --channels C for its width")
            dense = np.zeros((lidar.shape[0], args.channels or 0), np.float32)
            camera = np.full((lidar.shape[0],), -1, np.int32)
        elif args.device == "cuda":
            dev_maps = {c: torch.from_numpy(m).cuda() for c, m in maps.items()}
            dense, camera = ops.point_image_features(torch.from_numpy(lidar).cuda(), dev_maps, channels=args.channels)
        else:
            dense, camera = ops.point_image_features_host(lidar, maps, channels=args.channels)
        save = image_features.save_packed if args.packed else image_features.save_dict
        save(os.path.join(feature_dir, filename), dense, camera)
        if (k + 1) % 100 == 0 or k + 1 == len(pathnames):
            print(f"{k + 1} / {len(pathnames)} frames", flush=True)


if __name__ == "__main__":
    main()
