"""Stand-alone timing of the window-attention core per stage of the headline scene (forward, optionally backward):
python tools/attn_bench.py [--bwd] [--iters 20] [--workload one_sweep|dense2m] [--drop 0.1]
                           [--mode shared|perhead|dot|torch-cosine|torch-dot] [--json FILE]
--mode: shared = one tau (seg3d_window_attn_fwd / _bwd), perhead = tau [1, H, 1, 1] and dot = no tau (the _modes entries);
torch-cosine / torch-dot = the composition a user had before the kernels took a mode: windows padded to [W, T, C] by gathers,
bmm, softmax under a key-padding mask, bmm (what flat2window + nn.MultiheadAttention do), dropout on the probabilities."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openseg3d_amd import batch as B, config, ops, scene, spconv, swformer  # noqa: E402


def torch_composition(qk, v, tau, heads, wi, drop_p):
    """Padded-window attention in plain torch.  Windows are grouped by padded length (powers of two from 32) as the
    reference's batching levels do, so a 5-token window is not padded to the longest one."""
    m, c = v.shape
    dh = c // heads
    tok = wi.tok[:m].long()
    starts, counts = wi.win_start[: wi.n_windows].long(), wi.win_count[: wi.n_windows].long()
    out = torch.zeros_like(v)
    cap = 32
    done = torch.zeros_like(counts, dtype=torch.bool)
    while not bool(done.all()):
        sel = (~done) & (counts <= cap)
        done |= sel
        if bool(sel.any()):
            s, n = starts[sel], counts[sel]
            slot = torch.arange(cap, device=v.device)[None, :]
            valid = slot < n[:, None]                                 # [W, T]
            rows = tok[(s[:, None] + slot).clamp(max=m - 1)]          # [W, T] flat rows (padding: any row, masked)
            w = rows.shape[0]
            q, k = (qk[rows][..., i * c:(i + 1) * c].reshape(w, cap, heads, dh).transpose(1, 2) for i in (0, 1))
            vv = v[rows].reshape(w, cap, heads, dh).transpose(1, 2)
            if tau is None:
                att = (q / dh ** 0.5) @ k.transpose(-1, -2)
            else:
                att = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-1, -2) / tau.reshape(1, -1, 1, 1).clamp(min=0.01)
            att = att.masked_fill(~valid[:, None, None, :], float("-inf")).softmax(dim=-1)
            if drop_p > 0:
                att = F.dropout(att, drop_p)
            o = (att @ vv).transpose(1, 2).reshape(w, cap, c)
            out = out.index_put((rows[valid],), o[valid])
        cap *= 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bwd", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--workload", default="one_sweep")
    ap.add_argument("--drop", type=float, default=0.0)
    ap.add_argument("--stages", default="0,1,2,3")
    ap.add_argument("--tau", type=float, default=1.0, help="value of the learnable temperature (tau_min = 0.01 clamps below)")
    ap.add_argument("--mode", default="shared", choices=["shared", "perhead", "dot", "torch-cosine", "torch-dot"])
    ap.add_argument("--json", default=None, help="append one result record to this file")
    args = ap.parse_args()
    per_stage = []
    dev = torch.device("cuda:0")
    cfg = config.default_cfg()
    if args.workload == "dense2m":
        cfg.DATASET.POINT_CLOUD_RANGE, cfg.DATASET.VOXEL_SIZE = list(scene.DENSE_RANGE), list(scene.DENSE_VOXEL)
        pts = scene.make_dense_scene(0)
    else:
        pts = scene.make_scene(0)
    ds = config.DatasetSpec(cfg)
    b = B.make_batch([pts], ds.voxel_size, ds.point_cloud_range)
    level = spconv.SiteLevel(b["voxel_coords"].int(), [int(g) for g in ds.grid_size][::-1], 1)
    info = [{int(k): v for k, v in lvl.items()} for lvl in cfg.MODEL.BATCHING_INFO]
    tot_ms, tot_fl = 0.0, 0.0
    depth_split = {0: (1, 2), 1: (2, 2), 2: (4, 4), 3: (1, 2)}  # layers on shift 0 / shift 1 (depths 3, 4, 8, 3)
    for stage, c in enumerate((48, 96, 192, 384)):
        if str(stage) in args.stages.split(","):
            part = swformer.SparseWindowPartitionLayer(info[stage], cfg.MODEL.WINDOW_SHAPE, [float(g) / 2 ** stage for g in ds.grid_size])
            plan = part.plan(level.coords, 1, c)
            m = level.coords.shape[0]
            tau = {"shared": torch.full((1, 1, 1), args.tau, device=dev), "torch-cosine": torch.full((1, 1, 1), args.tau, device=dev),
                   "perhead": torch.full((1, 8, 1, 1), args.tau, device=dev)}.get(args.mode)  # None: dot product
            for shift in (0, 1):
                wi = plan.index[shift]
                qk = torch.randn(m, 2 * c, device=dev, requires_grad=args.bwd)
                v = torch.randn(m, c, device=dev, requires_grad=args.bwd)
                g = torch.randn(m, c, device=dev)
                cnt = wi.win_count[: wi.n_windows].double()
                flop = 4.0 * c * float((cnt * cnt).sum())

                def run():
                    if args.mode.startswith("torch"):
                        o = torch_composition(qk, v, tau, 8, wi, args.drop)
                    else:
                        o = ops.window_attention_packed(qk, v, tau, 0.01, 8, wi, args.drop, 1234)
                    if args.bwd:
                        o.backward(g)
                        qk.grad = v.grad = None
                for _ in range(3):
                    run()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.iters):
                    run()
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) / args.iters * 1e3
                layers = depth_split[stage][shift]
                tot_ms += us * layers / 1e3
                tot_fl += flop * layers
                per_stage.append({"stage": stage + 1, "shift": shift, "us": round(us, 1)})
                print(f"stage {stage + 1} C={c} shift {shift}: m={m} windows={wi.n_windows} tiles={wi.n_tiles} chunks={wi.n_qgroups} "
                      f"{us:8.1f} us  {flop * (3.5 if args.bwd else 1.0) / us / 1e6:7.1f} TF/s (algorithmic)", flush=True)
        if stage < 3:
            level = level.down()[0]
    print(f"forward{'+backward' if args.bwd else ''} of the 18 layers: {tot_ms:.3f} ms, {tot_fl / tot_ms / 1e9:.1f} TF/s fwd-algorithmic")
    if args.json:
        rec = {"mode": args.mode, "bwd": args.bwd, "drop": args.drop, "tau": args.tau, "workload": args.workload,
               "iters": args.iters, "layers_18_ms": round(tot_ms, 3), "per_stage": per_stage}
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
