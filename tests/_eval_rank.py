"""One rank of tests/test_eval_host.py::test_distributed_hist_gloo_world_2 (CPU, gloo): the rank adds its own shard of
the frames to an IOUMetric; get_metric() all-reduces the confusion matrix over the default group, so every rank prints
the matrix and mIoU of the union of the shards."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openseg3d_amd.evaluation import IOUMetric  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    g = np.load(os.path.join(ROOT, "tests", "golden", "tta_views.npz"))
    cut = int(g["iou22_split"][0])
    shard = slice(0, cut) if rank == 0 else slice(cut, None)
    m = IOUMetric([f"c{i}" for i in range(22)])
    m.add(g["iou22_preds"][shard], g["iou22_labels"][shard])
    local = m.confusion_matrix()
    r = m.get_metric()
    c = len(m.class_names)
    # the union's matrix, reduced the way get_metric reduces it: the test compares both against the whole set
    hist = m.reduce_tensor(torch.from_numpy(local)).numpy().reshape(c, c)
    out = {"rank": rank, "hist": hist.tolist(), "local_total": int(local.sum()), "mIOU": r["mIOU"]}
    sys.stdout.write("EVALRANK " + json.dumps(out) + "\n")
    sys.stdout.flush()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
