#!/usr/bin/env python3
"""Benchmark of the sparse-voxel segmentation hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--mode fwd|fwdbwd] [--workload ...] [--scenes S]
                    [--full] [--dump-outputs DIR]

One "step" = one pass of the hot path over one batch of synthetic input per GPU: GPU voxelisation of
a resident Waymo-shaped scene (~180 k float32 points, 0.1 m voxels, grid 1440x1440x64, i.e.
configs/waymo_one_sweep.yaml = BASELINE.json configs[1]) followed by Segformer forward + loss +
backward + SGD step (default mode fwdbwd = the metric "points/sec fwd+bwd"; gradients all-reduced
over RCCL when N > 1); mode fwd times the forward-only eval of the same scenes instead.
Scenes shard data-parallel: every rank processes its own scenes,
`value` = points processed by all ranks / max-over-ranks wall time ("scaling": "weak").

A plain run sets up, warms up, times the K steps and prints the line.  --dump-outputs DIR then writes what the last
timed step returned (DIR/<name>.npy, see dump_outputs); the inputs are seeded, so two builds can be compared output for
output.  --full adds everything else the benchmark measures or checks, as listed below: with --full a training run also
times the forward-only eval of the same scenes (`fwd_only`) and probes for host gaps (`idle`), --storage bf16 times its
fp32 side too, and N > 1 times the step without the gradient exchange (`allreduce`).

N > 1: either an outer launcher provides RANK / WORLD_SIZE (python -m torch.distributed.run ... bench.py --gpus N), or
`python bench.py --gpus N` starts its own N ranks (tools/dist_train.sh:7-13 does the same for the reference) -- the
parent spawns fresh children before it ever touches a GPU and relays rank 0's line.

Prints ONE JSON line on rank 0 with the contract fields, plus with --full
  roofline     -- the dominant kernel (sparse-conv gather-GEMM): algorithmic bytes / live HIP-event time
  cpu_baseline -- the CPU oracle (port of the reference algorithm) timed on the host cores, N=1 only
  parity       -- GPU path vs that oracle on the same sample: logits, voxel ids, rulebooks
  fp32_exact   -- the same training step with exact-fp32 products, timed in a child run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec (6290 GB/s measured copy), MI355X_MICROARCH.md:36
MFMA_BF16_TFLOPS = 2500.0  # dense bf16 MFMA peak, MI355X_MICROARCH.md:43
PMC_TRAFFIC_FILES = ("r05_pmc_conv_traffic.json", "r05_pmc_conv_traffic_dense2m.json", "r05_pmc_conv_traffic_cylinder.json",
                     "r05_pmc_conv_traffic_multi_sweeps.json", "r05_pmc_conv_traffic_spnet.json", "r04_pmc_conv_traffic.json", "r04_pmc_conv_traffic_dense2m.json", "r04_pmc_conv_traffic_cylinder.json",
                     "r04_pmc_conv_traffic_multi_sweeps.json", "r04_pmc_conv_traffic_spnet.json", "r03_pmc_conv_traffic.json", "r03_pmc_conv_traffic_dense2m.json", "r03_pmc_conv_traffic_cylinder.json",
                     "r03_pmc_conv_traffic_multi_sweeps.json", "r03_pmc_conv_traffic_spnet.json", "r02_pmc_conv_traffic.json")
ATTENTION_REPORT = None  # filled by conv_roofline's instrumented forward
LAYERS_JSON = os.path.join(ROOT, "bench_out", "bench_layers.json")  # per-layer conv timings of the last --full run
DUMP_BYTES = 64 * 10**6  # --dump-outputs writes at most this much

WORKLOADS = {
    "one_sweep": "waymo_one_sweep (BASELINE configs[1])",
    "cylinder": "waymo_one_sweep_cylinder (BASELINE configs[2] geometry)",
    "multi_sweeps": "waymo_multi_sweeps + image features (BASELINE configs[3])",
    "dense2m": "synthetic dense scene, 2 M points @0.02 m voxels in a 28.8 m x 28.8 m x 1.28 m block "
               "(BASELINE configs[4] / SURVEY 8d Config 5)",
}


def lib_sha16():
    """First 16 hex digits of the sha256 of the loaded libseg3d_hip.so: ties a committed PMC file to the build it measured."""
    import hashlib
    from openseg3d_amd import _lib
    h = hashlib.sha256()
    with open(_lib.LIB_PATH, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()[:16]


def dump_outputs(outputs, out_dir):
    """--dump-outputs: every tensor of `outputs` (what one step returned to its caller) as out_dir/<name>.npy -- float64
    stays float64, integers become float64, other floats float32.  When all of them together exceed DUMP_BYTES, every
    array keeps the same share of its rows, drawn with a fixed seed (sorted); out_dir/<name>_rows.npy then holds the row
    indices (float64)."""
    arrays = {k: v.detach() for k, v in outputs.items() if torch.is_tensor(v)}
    arrays = {k: v.double() if v.dtype == torch.float64 or not v.is_floating_point() else v.float() for k, v in arrays.items()}
    nbytes = lambda v: v.numel() * v.element_size()  # noqa: E731
    rowed = {k for k, v in arrays.items() if v.dim() > 0 and v.shape[0] > 1}
    share = 1.0
    if sum(nbytes(v) for v in arrays.values()) > DUMP_BYTES:  # the sampled rows and their float64 indices must fit
        fixed = sum(nbytes(v) for k, v in arrays.items() if k not in rowed)
        room = DUMP_BYTES - fixed - 2048 * len(arrays)  # (a generous 1 KiB per .npy header)
        share = room / sum(nbytes(arrays[k]) + 8 * arrays[k].shape[0] for k in rowed)
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        if share < 1.0 and k in rowed:
            n = v.shape[0]
            rows = np.sort(np.random.default_rng(0).choice(n, max(int(n * share), 1), replace=False))
            np.save(os.path.join(out_dir, f"{k}_rows.npy"), rows.astype(np.float64))
            v = v[torch.from_numpy(rows).to(v.device)]
        np.save(os.path.join(out_dir, f"{k}.npy"), v.cpu().numpy())


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", choices=["fwd", "fwdbwd"], default="fwdbwd")
    ap.add_argument("--scenes", type=int, default=0, help="distinct resident scenes per rank (0 = 4, dense2m: 2)")
    ap.add_argument("--batch", type=int, default=1, help="scenes per step per GPU")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="one_sweep",
                    help="one_sweep = BASELINE configs[1] (the headline); cylinder = configs[2] geometry "
                         "(waymo_one_sweep_cylinder.yaml, use --batch 4); multi_sweeps = configs[3] "
                         "(waymo_multi_sweeps.yaml + image features, 3 sweeps, use --batch 2); dense2m = configs[4]")
    ap.add_argument("--segmentor", choices=["segformer", "spnet"], default="segformer",
                    help="MODEL.SEGMENTOR (builder.py:8-23); segformer is the headline, spnet = SparseUnet + OCR")
    ap.add_argument("--criterion", choices=["default", "ce"], default="default",
                    help="default = MODEL.LOSSES of the reference config (ohem_ce + lovasz on the point, voxel and "
                         "auxiliary heads, tools/train.py:71-110); ce = plain cross-entropy on the three heads")
    ap.add_argument("--storage", choices=["fp32", "bf16"], default="fp32",
                    help="bf16 = BASELINE configs[4]'s reduced-precision mode as this build defines it (SURVEY D7): the sparse-conv "
                         "feature maps of the INFERENCE forward are stored in bf16 (fp32 accumulate; which tensors may be rounded "
                         "was decided per op family, tools/bf16_storage_probe.py); `fwd_only` is then that forward and the line "
                         "carries its agreement with the fp32-storage forward of the same weights.  The TRAINING step saves bf16 "
                         "copies of the rows its weight gradients multiply with (graph tensors and gradients stay fp32; "
                         "SEG3D_TRAIN_STORAGE=bf16) and is timed after the same steps with fp32 copies (`train_storage`).")
    ap.add_argument("--sweeps", type=int, default=0,
                    help="multi_sweeps only: DATASET.NUM_SWEEPS (0 = 3, what configs/waymo_multi_sweeps.yaml:2-4 sets; 5 = "
                         "DATASET.MAX_NUM_SWEEPS and BASELINE configs[3]'s wording, ~800 k rows per scene)")
    ap.add_argument("--sync-bn", action="store_true", help="tools/train.py --sync_bn: SyncBatchNorm over the ranks")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-fp32-exact", action="store_true",
                    help="skip the child run that times the same step with exact-fp32 products (SEG3D_CONV_PRECISION=fp32)")
    ap.add_argument("--fp64-oracle", action="store_true",
                    help="evaluate the float64 oracle on the parity sample of a workload other than the headline one too "
                         "(the headline workload does it by default)")
    ap.add_argument("--no-fp64-oracle", action="store_true",
                    help="skip the second, float64 evaluation of the CPU oracle on the parity sample (`parity.vs_fp64_oracle`; "
                         "run by default for the headline workload only: it doubles the oracle's time)")
    ap.add_argument("--no-pipeline", action="store_true", help="build each step's batch and index plan at the start of the step "
                    "instead of on the pipeline stream during the previous step")
    ap.add_argument("--cpu-points", type=int, default=-1,
                    help="points of the CPU-baseline / parity sample (0 = whole scene; default: whole scene, "
                         "150000 for dense2m and 30000 current-sweep rows for multi_sweeps so that the run stays within minutes)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: CPU baseline and parity against the "
                         "oracle, the exact-fp32 child run, rooflines and per-layer timings (written to "
                         f"{os.path.relpath(LAYERS_JSON, ROOT)}), fwd_only and the idle probe of a training run, the fp32 "
                         "side of --storage bf16, the exchange cost of N > 1")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step returned to DIR/<name>.npy (float32 / float64, at most "
                         f"{DUMP_BYTES // 10**6} MB in all: a fixed, seeded row sample of a larger output)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def conv_roofline(model, batch, dev):
    """One instrumented forward: HIP events around every seg3d_spconv_fwd launch (same stream)."""
    from openseg3d_amd import ops
    records = []
    orig = ops._conv_apply

    def timed(x, nbr, w_packed, bias, cin, cout, order=None, plan=None):  # noqa: E306
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = orig(x, nbr, w_packed, bias, cin, cout, order, plan)
        e1.record()
        records.append((nbr, cin, cout, e0, e1, x.shape[0], x.element_size(), y.element_size()))
        return y

    orig_act = ops.conv_act  # inference form of the conv blocks (BatchNorm folded, ReLU / residual in the epilogue)

    def timed_act(x, nbr, packed, bias, cin, cout, order=None, addend=None, relu=True, plan=None):  # noqa: E306
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = orig_act(x, nbr, packed, bias, cin, cout, order, addend, relu, plan)
        e1.record()
        records.append((nbr, cin, cout, e0, e1, x.shape[0], x.element_size(), y.element_size()))
        return y

    attn_records = []
    orig_attn = ops.window_attention_packed

    def timed_attn(qk, v, tau, tau_min, heads, wi, *a, **kw):  # noqa: E306
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o = orig_attn(qk, v, tau, tau_min, heads, wi, *a, **kw)
        e1.record()
        attn_records.append((wi, v.shape[1], e0, e1))
        return o

    ops._conv_apply = timed
    ops.conv_act = timed_act
    ops.window_attention_packed = timed_attn
    # per layer the MEDIAN over 5 instrumented forwards: an event bracket also contains whatever the host does between
    # the two records while the GPU idles (an allocator miss -> hipMalloc), and one such stall must not enter the figure
    passes = 5
    try:
        with torch.no_grad():
            for _ in range(passes):
                model(dict(batch))
        torch.cuda.synchronize()
    finally:
        ops._conv_apply = orig
        ops.conv_act = orig_act
        ops.window_attention_packed = orig_attn
    # window attention (all kernels of one layer's attention core): algorithmic FLOPs 4*C*sum_w n_w^2
    sq_cache, a_flop, a_ms = {}, 0.0, 0.0
    by_width = {}
    n_attn = len(attn_records) // passes
    for li in range(n_attn):
        wi, c, _, _ = attn_records[li]
        if id(wi) not in sq_cache:
            cnt = wi.win_count[: wi.n_windows].double()
            sq_cache[id(wi)] = float((cnt * cnt).sum().item())
        fl = 4.0 * c * sq_cache[id(wi)]
        ms = float(np.median([attn_records[li + k * n_attn][2].elapsed_time(attn_records[li + k * n_attn][3]) for k in range(passes)]))
        a_flop += fl
        a_ms += ms
        w = by_width.setdefault(c, [0.0, 0.0, 0])
        w[0] += fl
        w[1] += ms
        w[2] += 1
    attn_tf = a_flop / a_ms / 1e9 if a_ms > 0 else 0.0
    global ATTENTION_REPORT
    ATTENTION_REPORT = {
        "bound": "mfma", "kernel": "window attention core of one forward (18 encoder layers; in-projection / out-projection "
                                   "GEMMs not included)",
        "achieved": round(attn_tf, 2), "peak": MFMA_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(attn_tf / MFMA_BF16_TFLOPS, 5),
        "note": "algorithmic 4*C*sum(n_w^2) FLOPs per layer / HIP-event time; executed MFMA FLOPs are higher (split-bf16 "
                "products, padding of heads and of windows to tiles)",
        "layers": n_attn, "gflop_per_forward": round(a_flop / 1e9, 2), "ms_per_forward": round(a_ms, 3),
        "by_width": {str(c): {"layers": w[2], "us_per_layer": round(w[1] * 1e3 / max(w[2], 1), 1),
                              "TFLOPs": round(w[0] / w[1] / 1e9, 1) if w[1] > 0 else 0.0} for c, w in sorted(by_width.items())}}
    pairs_cache, tot_bytes, tot_ms, foot_bytes = {}, 0.0, 0.0, 0.0
    per_layer = []
    n_layers = len(records) // passes
    for li in range(n_layers):
        nbr, cin, cout, _, _, m_in, s_in, s_out = records[li]
        key = nbr.data_ptr()
        if key not in pairs_cache:
            pairs_cache[key] = int((nbr >= 0).sum().item())
        p = pairs_cache[key]
        algo = p * (cin * s_in + cout * s_out) + 27 * cin * cout * 4 + p * 8  # SURVEY 8d (s = bytes per stored element)
        ms = float(np.median([records[li + k * n_layers][3].elapsed_time(records[li + k * n_layers][4]) for k in range(passes)]))
        tot_bytes += algo
        tot_ms += ms
        m_out = int(nbr.shape[1])
        foot_bytes += m_in * cin * s_in + m_out * cout * s_out + 27 * cin * cout * 4 + 27 * m_out * 4
        # each layer against ITS bound: narrow layers move bytes (footprint = every input / output row once + W + table),
        # wide layers multiply (useful FLOPs against the split-bf16 ceiling = bf16 MFMA peak / 3 products)
        if max(cin, cout) <= 96:
            foot = m_in * cin * s_in + m_out * cout * s_out + 27 * cin * cout * 4 + 27 * m_out * 4
            lay = {"bound": "hbm", "frac": round(foot / ms / 1e6 / HBM_PEAK_GBS, 3)}
        else:
            lay = {"bound": "mfma_bf16x3", "frac": round(2.0 * p * cin * cout / ms / 1e9 / (MFMA_BF16_TFLOPS / 3.0), 3)}
        per_layer.append({"rows": m_out, "pairs": p, "cin": cin, "cout": cout, "us": round(ms * 1e3, 1),
                          "GBs": round(algo / ms / 1e6, 1), **lay})
    n = max(n_layers, 1)
    achieved = tot_bytes / tot_ms / 1e6 if tot_ms > 0 else 0.0
    # HBM traffic per launch QUOTED from the committed PMC passes of this workload (FETCH_SIZE doubled per the gfx950
    # correction + WRITE_SIZE, two separate rocprofv3 --pmc runs; counters cannot be read inside this process); only
    # quoted when the profiled workload is the one just run (same algorithmic bytes), otherwise null.
    traffic, traffic_src, traffic_lib = None, None, None
    for name in PMC_TRAFFIC_FILES:
        pmc = os.path.join(ROOT, "profiles", name)
        if not os.path.exists(pmc):
            continue
        with open(pmc) as f:
            p = json.load(f)
        if abs(p.get("algorithmic_bytes_per_launch", 0) - tot_bytes / n) <= 0.01 * tot_bytes / n:
            traffic, traffic_src = p["traffic_bytes_per_launch"], f"quoted from profiles/{name} (rocprofv3 --pmc, same workload)"
            traffic_lib = p.get("lib_sha16")
            break
    # the counters were read from ONE build of the library: say so when the library that just ran is another one
    here = lib_sha16()
    traffic_stale = None if traffic is None else bool(traffic_lib != here)
    # `frac` follows SURVEY 8(d)'s formula, which counts a row once per offset that gathers it -- a gather RATE, most of which
    # is served by L1 / L2.  What must cross the HBM interface at least once is the footprint (every input and output row
    # once + weights + table): that second fraction is the one to read as HBM utilisation.
    foot_frac = foot_bytes / tot_ms / 1e6 / HBM_PEAK_GBS if tot_ms > 0 else 0.0
    return {"bound": "hbm", "kernel": f"spconv_tile_kernel / spconv_split_kernel (all {n_layers} sparse-conv launches of one forward, per-layer median of {passes} forwards)",
            "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "frac_of_hbm_by_footprint": round(foot_frac, 4),
            "frac_by_counters": None if traffic is None else round(traffic * n / tot_ms / 1e6 / HBM_PEAK_GBS, 4),
            "footprint_bytes_per_launch": int(foot_bytes / n), "traffic": traffic, "traffic_source": traffic_src,
            "traffic_lib_sha16": traffic_lib, "lib_sha16": here, "traffic_stale": traffic_stale,
            "launches": n_layers, "bytes_per_launch": int(tot_bytes / n), "us_per_launch": round(tot_ms * 1e3 / n, 2)}, per_layer


def cpu_baseline(pts, n_cur, image, cfg, ds, model, dtype=torch.float32):
    """The oracle (CPU restatement of the reference algorithm) on the host cores: the sample's points, same weights,
    eval forward.  pts: rows of one scene (all sweeps), n_cur: its current-sweep rows, image: [n_cur, 28] or None.
    dtype float64: the same forward evaluated in double precision (weights and inputs widened exactly; the position
    embedding keeps its float32 values, the reference computes it in float32) -- the reference's FUNCTION without its
    float32 round-off, against which both the float32 oracle and the GPU path can be placed.
    Returns (report, oracle result dict, oracle voxel coords, oracle point->voxel ids)."""
    from oracle import index_ops, model as omodel
    # the GPU box gives one GPU's share of the host (16 cores); never oversubscribe a larger affinity mask
    cores = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 16)
    torch.set_num_threads(cores)
    print(f"[bench] cpu_baseline: oracle forward of {pts.shape[0]} points on {cores} host threads ...", file=sys.stderr, flush=True)
    t0 = time.time()
    coords, ids = index_ops.voxelize(pts, ds.voxel_size, ds.point_cloud_range)
    batch = {"points": torch.from_numpy(np.pad(pts, ((0, 0), (1, 0)))).to(dtype),
             "voxel_coords": torch.from_numpy(np.pad(coords, ((0, 0), (1, 0)))).float(),
             "point_voxel_ids": torch.from_numpy(ids).long(), "batch_size": 1,
             "point_id_offset": torch.tensor([float(n_cur)])}
    if image is not None:
        batch["point_image_features"] = image.detach().cpu().to(dtype)
    ocfg = {"grid_size": index_ops.grid_size_of(ds.voxel_size, ds.point_cloud_range),
            "batching_info": [{int(k): v for k, v in lvl.items()} for lvl in cfg.MODEL.BATCHING_INFO],
            "window_shape": cfg.MODEL.WINDOW_SHAPE, "depths": cfg.MODEL.DEPTHS,
            "use_multi_sweeps": bool(ds.use_multi_sweeps), "use_image_feature": bool(ds.use_image_feature)}
    sd = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    with torch.no_grad():
        res = (omodel.spnet_forward if cfg.MODEL.SEGMENTOR == "spnet" else omodel.segformer_forward)(batch, sd, ocfg)
    dt = time.time() - t0
    report = {"value": round(n_cur / dt, 1), "unit": "points/s", "cores": cores, "kind": "port", "dtype": str(dtype).split(".")[-1],
              "sample": f"1 forward (voxelize + {cfg.MODEL.SEGMENTOR} eval) of {n_cur} points ({pts.shape[0]} rows with history "
                        f"sweeps) of scene seed 0, {coords.shape[0]} voxels, {dt:.1f} s, torch.set_num_threads({cores})"}
    return report, res, coords, ids


def parity_report(pts, n_cur, image, ds, model, dev, oracle_res, oracle_coords, oracle_ids, oracle_f64=None):
    """GPU path vs the oracle on the same sample and the same weights (the `logit parity` half of the metric):
    per-point logits within 1e-3, voxel ids and rulebooks bit-exact (BASELINE.json north_star).  oracle_f64: the result
    of the same oracle evaluated in float64 -- then `vs_fp64_oracle` places BOTH float32 computations (the CPU oracle's and
    the GPU's) against it: at |logit| ~ 200 the float32 oracle's own round-off is a large part of `max_abs_logit_diff`."""
    from openseg3d_amd import batch as B
    b = B.batch_from_resident(B.collate_points([pts], dev), [n_cur], ds.voxel_size, ds.point_cloud_range, image)
    gpu_coords = b["voxel_coords"].int().cpu().numpy()
    ids_ok = bool(np.array_equal(gpu_coords[:, 1:], oracle_coords) and (gpu_coords[:, 0] == 0).all()
                  and np.array_equal(b["point_voxel_ids"].cpu().numpy(), oracle_ids))
    with torch.no_grad():
        res = model(b)
    level = b.get("site_level")
    books_ok = None
    if level is not None and ids_ok:
        books_ok = True
        for k, ref in enumerate(oracle_res["_levels"]):
            books_ok &= bool(np.array_equal(level.subm().cpu().numpy(), ref.subm()))
            if k < 3:
                coarse, fwd, inv = level.down()
                rc, rf, ri = ref.down()
                books_ok &= bool(np.array_equal(coarse.coords.cpu().numpy(), rc.coords)
                                 and np.array_equal(fwd.cpu().numpy(), rf) and np.array_equal(inv.cpu().numpy(), ri))
                level = coarse
    out = {"n_points": int(n_cur), "voxel_ids_bit_exact": ids_ok, "rulebook_bit_exact": books_ok, "tolerance": 1e-3}
    for key, name in (("point_out", "max_abs_logit_diff"), ("voxel_out", "max_abs_voxel_logit_diff"),
                      ("aux_voxel_out", "max_abs_aux_logit_diff")):
        if ids_ok:
            out[name] = float((res[key].float().cpu() - oracle_res[key]).abs().max())
    if ids_ok:
        out["max_abs_logit"] = float(oracle_res["point_out"].abs().max())
        out["max_rel_logit_diff"] = out["max_abs_logit_diff"] / max(out["max_abs_logit"], 1e-30)
    if ids_ok and oracle_f64 is not None:
        v64 = {}
        for key, name in (("point_out", "logit"), ("voxel_out", "voxel_logit"), ("aux_voxel_out", "aux_logit")):
            v64[f"gpu_max_abs_{name}_diff"] = float((res[key].double().cpu() - oracle_f64[key]).abs().max())
            v64[f"oracle_fp32_max_abs_{name}_diff"] = float((oracle_res[key].double() - oracle_f64[key]).abs().max())
        v64["note"] = ("the same oracle evaluated in float64 as the reference point: how far the float32 CPU oracle and the GPU "
                       "path each are from the reference's function without float32 round-off")
        out["vs_fp64_oracle"] = v64
    # what the checker itself is pinned by
    out["pinned_by"] = ("oracle/ = CPU restatement checked against outputs of the reference's own Python (tests/golden/*.npz, "
                        "regenerable with tests/golden/make_golden.py) for voxelizer, window partition, attention, "
                        "Segformer / SPNet wiring and losses; spconv and torch_scatter are absent third-party packages "
                        "(requirements.txt:4,8): their restatement is cross-checked against dense F.conv3d / conv_transpose3d "
                        "only (tests/test_oracle_sparse_conv.py)")
    return out


def main():
    args = parse()
    from openseg3d_amd import dist as D
    if args.gpus > 1 and "RANK" not in os.environ:
        # the driver's command form: start our own ranks (tools/dist_train.sh:7-13).  Nothing in this process has
        # touched the GPU yet -- importing torch does not initialise HIP -- and nothing will: it only waits.
        sys.exit(D.launch_local_ranks([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], args.gpus))
    share = os.environ.get("SEG3D_BENCH_SHARE_GPU", "0") == "1"  # rehearsal on a one-GPU box: all ranks on cuda:0 (gloo)
    rank, world, local = D.init_job(backend=os.environ.get("SEG3D_BENCH_BACKEND") or "nccl", share_device=share)
    torch.cuda.set_device(local)
    import torch.distributed as dist
    distributed = dist.is_available() and dist.is_initialized()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    from openseg3d_amd import batch as B, config, losses as _losses, ops as _ops, scene, segformer
    dev = torch.device("cuda", local)
    cfg = config.default_cfg()  # == configs/waymo_one_sweep.yaml for every key the model path reads
    if args.workload == "cylinder":  # configs/waymo_one_sweep_cylinder.yaml:2-4
        cfg.DATASET.USE_CYLINDER = True
        cfg.DATASET.POINT_CLOUD_RANGE = [0, -3.1415926, -2, 75.2, 3.1415926, 5.2]
        cfg.DATASET.VOXEL_SIZE = [0.05, 0.012, 0.1]
    elif args.workload == "multi_sweeps":  # configs/waymo_multi_sweeps.yaml:1-4 + USE_IMAGE_FEATURE
        cfg.DATASET.USE_MULTI_SWEEPS = True
        cfg.DATASET.USE_IMAGE_FEATURE = True
        if args.sweeps:
            if not 1 <= args.sweeps <= cfg.DATASET.MAX_NUM_SWEEPS:
                raise SystemExit(f"--sweeps {args.sweeps}: 1 .. DATASET.MAX_NUM_SWEEPS = {cfg.DATASET.MAX_NUM_SWEEPS}")
            cfg.DATASET.NUM_SWEEPS = args.sweeps
    elif args.workload == "dense2m":  # BASELINE configs[4]: same 1440 x 1440 x 64 grid at 0.02 m
        cfg.DATASET.POINT_CLOUD_RANGE = list(scene.DENSE_RANGE)
        cfg.DATASET.VOXEL_SIZE = list(scene.DENSE_VOXEL)
    cfg.MODEL.SEGMENTOR = args.segmentor
    ds = config.DatasetSpec(cfg)
    torch.manual_seed(0)
    model = segformer.build_segmentor(cfg, ds).to(dev)

    # resident synthetic scenes: seeds differ per rank (data-parallel shards of the scene stream)
    n_scenes = args.scenes or (2 if args.workload == "dense2m" else 4)
    seeds = [rank * n_scenes * args.batch + i for i in range(n_scenes * args.batch)]
    if args.workload == "multi_sweeps":
        made = [scene.make_multi_sweep_scene(s, cfg.DATASET.NUM_SWEEPS) for s in seeds]
        scenes_np, n_cur = [m[0] for m in made], [m[1] for m in made]
    else:
        make = scene.make_dense_scene if args.workload == "dense2m" else scene.make_scene
        scenes_np = [make(s) for s in seeds]  # cylinder: cartesian rows stay resident, cart2polar runs in the step
        n_cur = [s.shape[0] for s in scenes_np]
    cyl = args.workload == "cylinder"
    groups = [list(range(i * args.batch, (i + 1) * args.batch)) for i in range(n_scenes)]
    resident = [B.collate_points([scenes_np[j] for j in g], dev) for g in groups]
    offsets = [np.cumsum([n_cur[j] for j in g]).tolist() for g in groups]  # cumulative current-sweep rows
    images = [None] * len(groups)
    if args.workload == "multi_sweeps":
        images = [torch.from_numpy(np.concatenate([scene.make_image_features(seeds[j], n_cur[j]) for j in g])).to(dev)
                  for g in groups]
    pts_per_step = [int(o[-1]) for o in offsets]  # points that receive logits

    # logit parity + CPU baseline on the weights the run starts from (seed 0), before anything is timed
    baseline = None
    parity_sample = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        # bounded samples (10-30 s of CPU work): the dense scene's first 150 k points; of a multi-sweep scene the first
        # 30 k current-sweep rows with their image features and twice as many history rows (the oracle's DeepFusion kNN is
        # a brute-force O(n^2) search: minutes on a whole sweep)
        n_cpu = args.cpu_points if args.cpu_points >= 0 else {"dense2m": 150000, "multi_sweeps": 30000}.get(args.workload, 0)
        sample, s_cur, s_img = scenes_np[0], n_cur[0], None
        if args.workload == "multi_sweeps":
            k = min(n_cpu, n_cur[0]) if n_cpu else n_cur[0]
            # history rows: the same number from EVERY history sweep (2k in all), so that a 5-sweep sample sees all five lags
            n_hist = max(cfg.DATASET.NUM_SWEEPS - 1, 1)
            per = (sample.shape[0] - n_cur[0]) // n_hist
            take = min(2 * k // n_hist, per)
            sample = np.concatenate([sample[:k]] + [sample[n_cur[0] + h * per: n_cur[0] + h * per + take] for h in range(n_hist)], axis=0)
            s_cur, s_img = k, images[0][:k]
        elif n_cpu:
            sample = sample[:n_cpu]
            s_cur = sample.shape[0]
        if cyl:  # the oracle takes the polar rows the device built: numpy's atan2f differs from any other libm's in the
            # last bit (tests/test_gpu_parity.py::test_cart2polar_matches_reference), which would move a few boundary points
            sample = _ops.cart2polar(torch.from_numpy(sample).to(dev)).cpu().numpy()
        model.eval()
        report, o_res, o_coords, o_ids = cpu_baseline(sample, s_cur, s_img, cfg, ds, model)
        o64 = None
        if (args.workload == "one_sweep" or args.fp64_oracle) and not args.no_fp64_oracle:
            o64 = cpu_baseline(sample, s_cur, s_img, cfg, ds, model, dtype=torch.float64)[1]
        baseline = (report, parity_report(sample, s_cur, s_img, ds, model, dev, o_res, o_coords, o_ids, o64))
        del o64
        parity_sample = (sample, s_cur, s_img)
        if cyl:
            # how many points land in ANOTHER voxel when phi comes from numpy's float32 arctan2 (what the reference's loader
            # computes, pointops_utils.py:8-11) instead of the device's correctly rounded value (<= 4 ulp apart)
            from oracle import index_ops
            host_rows = scene.cart2polar_rows(scenes_np[0][: sample.shape[0]])
            ch, ih = index_ops.voxelize(host_rows, ds.voxel_size, ds.point_cloud_range)
            cd, idv = index_ops.voxelize(sample, ds.voxel_size, ds.point_cloud_range)
            # voxel numbering is first-seen order on both sides: compare the CELLS (-1 = out of range)
            cell_h = np.where(ih[:, None] >= 0, ch[np.maximum(ih, 0)], -1)
            cell_d = np.where(idv[:, None] >= 0, cd[np.maximum(idv, 0)], -1)
            moved = int((cell_h != cell_d).any(1).sum())
            baseline[1]["cylinder_phi"] = {"points_in_another_voxel_under_numpy_phi": moved, "n_points": int(sample.shape[0]),
                                           "frac": moved / max(int(sample.shape[0]), 1), "bar": 1e-4}
        del o_res

    hi = None
    # the timed loops run on a HIGH-priority stream: the main chain is the critical path, the weight-gradient and pipeline
    # streams (normal priority) fill what it leaves (46.7 -> 46.3 ms per step; SEG3D_BENCH_MAIN_PRIORITY=0 = default stream).
    # It is entered BEFORE the DDP wrapper is built: DDP stashes the parameters' AccumulateGrad nodes with the stream
    # current at construction, and a backward pass on another stream then synchronises at every one of them (one-rank
    # rehearsal: 79.7 instead of 46.9 ms per step -- what the first multi-GPU run would have hit)
    if dev.type == "cuda" and os.environ.get("SEG3D_BENCH_MAIN_PRIORITY", "-1") == "-1":
        hi = torch.cuda.Stream(device=dev, priority=-1)
        hi.wait_stream(torch.cuda.current_stream(dev))
        torch.cuda.set_stream(hi)
    train = args.mode == "fwdbwd"
    net = model
    if train and distributed:  # tools/train.py:246-247, 276-279
        net = D.wrap_data_parallel(model, dev, sync_bn=args.sync_bn)
        model = net.module
    # configs/waymo_one_sweep.yaml: SGD, momentum 0.9, weight decay 1e-4; torch's fused multi-tensor implementation
    # (same arithmetic, 3 launches instead of 24) unless SEG3D_BENCH_FOREACH_SGD=1
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4,
                          fused=os.environ.get("SEG3D_BENCH_FOREACH_SGD", "0") != "1")
    labels = [torch.randint(0, 22, (n,), device=dev) for n in pts_per_step]
    if args.criterion == "ce":
        cfg.MODEL.LOSSES = {"ce": 1.0}
    criterion = _losses.build_criterion(cfg, ds)  # builder.py:26-40
    # voxel labels are part of the collated batch in the reference (WaymoDataset.prepare_voxel_labels in the loader
    # workers): made once per resident scene group here, outside the timed region; the auxiliary-head labels are looked
    # up inside the step, as tools/train.py:86-104 does
    voxel_labels = []
    for j in range(len(resident)):
        b = B.batch_from_resident(resident[j], offsets[j], ds.voxel_size, ds.point_cloud_range, images[j], cyl)
        cur = torch.nonzero(b["points"][:, 4] == 0).view(-1) if args.workload == "multi_sweeps" else None
        voxel_labels.append(_ops.prepare_voxel_labels(b["point_voxel_ids"], labels[j], b["voxel_coords"].shape[0],
                                                      ignore_index=ds.ignore_index, cur_point_indices=cur).long())

    # Input pipeline.  What depends on the raw points alone -- device voxelization, collation and the forward's index plan
    # (site levels, rulebooks, window partitions; ~100 short dependent kernels and all of the forward's host read-backs) --
    # is built for step i+1 on its own stream while step i computes: the reference overlaps the same work in its DataLoader
    # workers (voxel_generator.py in waymo_dataset.py:__getitem__), here it stays on the GPU and inside the timed region
    # (K steps time K voxelizations and K plans; the first timed step's was overlapped with the last warm-up step, the
    # last timed step builds one that is never used).  --no-pipeline builds every batch at the start of its own step.
    pipe_stream = _ops.side_stream(dev, 1) if (dev.type == "cuda" and not args.no_pipeline) else None
    pending = {}

    def build(j):
        b = B.batch_from_resident(resident[j], offsets[j], ds.voxel_size, ds.point_cloud_range, images[j], cyl)
        return model.prepare_batch(b) if pipe_stream is not None else b

    def hand_over(obj, stream, seen):
        """record_stream(stream) on every tensor reachable from a batch built on the pipeline stream (dict / list / plan
        objects): the allocator then knows the consumer stream's kernels read these blocks and will not hand them to a later
        build before those kernels have run, whatever a step function does with its references."""
        if id(obj) in seen:
            return
        seen.add(id(obj))
        if torch.is_tensor(obj):
            if obj.is_cuda:
                obj.record_stream(stream)
        elif isinstance(obj, dict):
            for v in obj.values():
                hand_over(v, stream, seen)
        elif isinstance(obj, (list, tuple, set)):
            for v in obj:
                hand_over(v, stream, seen)
        elif hasattr(obj, "__dict__") or hasattr(obj, "__slots__"):
            if isinstance(obj, (torch.nn.Module, torch.cuda.Stream, torch.cuda.Event)):
                return
            for name in list(getattr(obj, "__dict__", {})) + list(getattr(type(obj), "__slots__", ())):
                try:
                    hand_over(getattr(obj, name), stream, seen)
                except AttributeError:
                    pass

    def next_batch(i):
        """Batch of step i; queues the build of step i+1's."""
        main = torch.cuda.current_stream(dev) if pipe_stream is not None else None
        item = pending.pop(i, None)
        if item is None or len(item) != 2:  # nothing was built ahead (first step of a phase, --no-pipeline)
            b = build(i % len(resident))
        else:
            b, done = item
            main.wait_event(done)
            hand_over(b, main, set())
        if pipe_stream is not None:
            # blocks the pipeline stream's allocator hands out again were freed by steps whose kernels are all in front of
            # this point of the main stream: the build waits for it (not for step i itself)
            mark = torch.cuda.Event()
            mark.record(main)
            pending.clear()
            pending[i + 1] = (mark,)
        return b

    def prefetch(i):
        """Called once step i is enqueued: step i+1's batch on the pipeline stream, beside step i's kernels."""
        item = pending.get(i + 1)
        if pipe_stream is None or item is None or len(item) != 1:
            return
        pipe_stream.wait_event(item[0])
        with torch.cuda.stream(pipe_stream):
            b = build((i + 1) % len(resident))
            done = torch.cuda.Event()
            done.record(pipe_stream)
        pending[i + 1] = (b, done)

    def fwd_step(i):
        b = next_batch(i)
        with torch.no_grad():
            res = model(b)
        prefetch(i)
        return res

    def train_step(i):
        j = i % len(resident)
        b = next_batch(i)
        opt.zero_grad(set_to_none=True)
        res = net(b)
        data = {"point_labels": labels[j], "voxel_labels": voxel_labels[j], "batch_size": b["batch_size"]}
        loss = _losses.compute_loss(res, data, criterion, cfg)
        loss.backward()
        opt.step()
        prefetch(i)
        out = dict(res)
        out["loss"] = loss
        return out

    local_sec = {}
    last = {}  # what the last timed step of each loop returned

    def timed(step_fn, tag):
        for i in range(args.warmup):
            step_fn(i)
        D.job_barrier(dev)
        t0 = time.perf_counter()
        for i in range(args.steps - 1):
            step_fn(args.warmup + i)
        last[tag] = step_fn(args.warmup + args.steps - 1)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        local_sec[tag] = time.perf_counter() - t0  # this rank alone (the job's time below adds the wait for the slowest)
        D.job_barrier(dev)
        sec = time.perf_counter() - t0
        pts = sum(pts_per_step[(args.warmup + i) % len(resident)] for i in range(args.steps))
        return D.aggregate_throughput(sec, pts, dev)

    def idle_probe(first, k):
        """Is the GPU ever waiting for the host inside a step?  (the profiled timeline shows 4 ms of gaps per
        step behind three copies -- before the fused SGD and before two elementwise kernels -- but a profiled host is a slow
        host.)  Un-profiled, with HIP events on the main stream:
          steady  -- k more steps as in the timed loop; events at the start of a step, behind backward() and behind
                     opt.step(); host clocks at the same points;
          fed     -- k steps each enqueued behind a 50 ms device-side sleep, so the whole step is in the queue before its first
                     kernel may start: the step's GPU time with the host out of the picture.
        gpu_idle_ms = steady main-stream time per step (start of a step to the start of the next) minus the fed step's --
        what the host, the launch path or the pipeline hand-over add to a step.  Runs after the timed region."""
        if dev.type != "cuda" or not hasattr(torch.cuda, "_sleep"):
            return None
        main = torch.cuda.current_stream(dev)

        def ev():
            e = torch.cuda.Event(enable_timing=True)
            e.record(main)
            return e

        def one(i, rec):
            j = i % len(resident)
            h0 = time.perf_counter()
            b = next_batch(i)
            e0 = ev()
            opt.zero_grad(set_to_none=True)
            res = net(b)
            ef = ev()
            data = {"point_labels": labels[j], "voxel_labels": voxel_labels[j], "batch_size": b["batch_size"]}
            loss = _losses.compute_loss(res, data, criterion, cfg)
            el = ev()
            loss.backward()
            h1 = time.perf_counter()
            e1 = ev()
            opt.step()
            h2 = time.perf_counter()
            e2 = ev()
            prefetch(i)
            h3 = time.perf_counter()
            rec.append((e0, e1, e2, h0, h1, h2, h3, ef, el))

        steady, fed = [], []
        for i in range(k + 1):
            one(first + i, steady)
        torch.cuda.synchronize(dev)
        for i in range(k):
            torch.cuda._sleep(5_000_000)  # s_memtime ticks at 100 MHz on gfx950: 50 ms, twice the host's enqueue time of a step
            one(first + k + 1 + i, fed)
            torch.cuda.synchronize(dev)
        ms = lambda a, b: a.elapsed_time(b)  # noqa: E731
        mean = lambda v: float(np.mean(v)) if len(v) else 0.0  # noqa: E731
        steady_step = mean([ms(steady[i][0], steady[i + 1][0]) for i in range(k)])
        fed_step = mean([ms(r[0], r[2]) for r in fed])
        return {"steps": k,
                "host_enqueue_ms": round(mean([(r[5] - r[3]) * 1e3 for r in steady[:k]]), 3),
                "host_enqueue_opt_step_ms": round(mean([(r[5] - r[4]) * 1e3 for r in steady[:k]]), 3),
                "host_in_prefetch_ms": round(mean([(r[6] - r[5]) * 1e3 for r in steady[:k]]), 3),
                "gpu_step_ms_steady": round(steady_step, 3),
                "gpu_step_ms_fed": round(fed_step, 3),
                "gpu_opt_step_ms_steady": round(mean([ms(r[1], r[2]) for r in steady[:k]]), 3),
                "gpu_opt_step_ms_fed": round(mean([ms(r[1], r[2]) for r in fed]), 3),
                "gpu_between_steps_ms": round(mean([ms(steady[i][2], steady[i + 1][0]) for i in range(k)]), 3),
                "gpu_idle_ms": round(max(steady_step - fed_step, 0.0), 3),
                # where the steady step is longer than the fed one: forward / criterion / backward segments of the main stream
                "gpu_segments_ms_steady": [round(mean([ms(r[a], r[b]) for r in steady[:k]]), 3) for a, b in ((0, 7), (7, 8), (8, 1))],
                "gpu_segments_ms_fed": [round(mean([ms(r[a], r[b]) for r in fed]), 3) for a, b in ((0, 7), (7, 8), (8, 1))],
                "note": "HIP events on the main stream, no profiler: steady = consecutive steps as timed; fed = each step enqueued "
                        "whole behind a 50 ms device-side sleep (the host cannot be late); gpu_idle_ms = steady - fed per step; "
                        "gpu_opt_step_ms = backward's last kernel to the fused SGD's last (the profiled timeline shows a 2.1 ms "
                        "gap there); gpu_between_steps_ms = SGD's end to the next step's first kernel (pipeline hand-over)"}

    weights_l1 = None
    nosync_ms = None
    idle_report = None
    extra_steps = 0
    train_storage = None
    peak_bytes = None
    if train:
        net.train()
        if args.storage == "bf16" and dev.type == "cuda":
            if args.full:
                # the same steps with the fp32 copies first (same process, same box), then with the opt-in bf16 copies:
                # the headline `value` of a --storage bf16 line is the second
                torch.cuda.reset_peak_memory_stats(dev)
                dt32, n32 = timed(train_step, "train_fp32_copies")
                last.clear()
                train_storage = {"ms_per_step_fp32_copies": round(dt32 / args.steps * 1e3, 3),
                                 "peak_memory_gb_fp32_copies": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 3)}
            _ops.TRAIN_STORAGE = "bf16"
        if dev.type == "cuda":
            torch.cuda.reset_peak_memory_stats(dev)
        dt, n_pts = timed(train_step, "train")
        if dev.type == "cuda":
            peak_bytes = torch.cuda.max_memory_allocated(dev)
        if args.dump_outputs and rank == 0:
            dump_outputs(last["train"], args.dump_outputs)
        last.clear()
        if train_storage is not None:
            train_storage.update({"ms_per_step": round(dt / args.steps * 1e3, 3), "peak_memory_gb": round(peak_bytes / 2 ** 30, 3),
                                  "mode": "bf16 COPIES of the rows each sparse-conv / Linear weight gradient multiplies with are "
                                          "what the forward saves for the backward (graph tensors and all gradients stay fp32; "
                                          "weight-gradient products: 2 MFMAs, 8-byte gathers, no split of x)",
                                  "stated_tolerance": "loss and all input-path gradients identical; conv / Linear weight gradients "
                                                      "within 1e-2 of their largest entry (tests/test_gpu_training.py::"
                                                      "test_bf16_training_copies_stay_within_their_stated_tolerance)"})
        # fingerprint of the weights after the timed steps (fp64 sum of |w| over every parameter): the kernels are
        # deterministic, so the streams, the deferred joins and the input pipeline must leave it unchanged to the last
        # digit (SEG3D_WGRAD_STREAM=0 / --no-pipeline give the single-stream reference); under DDP every rank must hold
        # the same value
        weights_l1 = float(sum(p.detach().double().abs().sum() for p in model.parameters()))
        if args.full and world == 1 and os.environ.get("SEG3D_BENCH_IDLE_PROBE", "1") != "0":
            k_idle = min(max(args.steps, 1), 6)
            idle_report = idle_probe(args.warmup + args.steps, k_idle)
            extra_steps = 2 * k_idle + 1 if idle_report is not None else 0
        if args.full and distributed and world > 1:
            # what the gradient exchange costs on the critical path: the same steps with DDP's all-reduce switched off
            # (no_sync), after the fingerprint -- the ranks' weights diverge from here on, only eval timing follows
            k = min(args.steps, 5)
            D.job_barrier(dev)
            t0 = time.perf_counter()
            with net.no_sync():
                for i in range(k):
                    train_step(args.warmup + args.steps + i)
            D.job_barrier(dev)
            nosync_ms = (time.perf_counter() - t0) / k * 1e3
    net.eval()
    storage_report = None
    if args.storage == "bf16":
        if args.full:
            # the same weights, scene 0, both storages: what the opt-in mode costs in logits and what it buys in time
            b_ref = B.batch_from_resident(resident[0], offsets[0], ds.voxel_size, ds.point_cloud_range, images[0], cyl)
            with torch.no_grad():
                ref_logits = model(b_ref)["point_out"].clone()
            dt_f32, n_pts_f32 = timed(fwd_step, "fwd_fp32")
            last.clear()
            _ops.STORAGE = "bf16"
            with torch.no_grad():
                got = model(B.batch_from_resident(resident[0], offsets[0], ds.voxel_size, ds.point_cloud_range, images[0], cyl))["point_out"]
            err = (got.float() - ref_logits).abs()
            storage_report = {
                "mode": "bf16 storage of the sparse-conv feature maps (inference forward; fp32 accumulate, bias and activation; "
                        "residual stream, attention, norms and per-point MLPs stay fp32: tools/bf16_storage_probe.py)",
                "vs_own_fp32_storage": {"max_abs_logit_diff": float(err.max()), "mean_abs_logit_diff": float(err.mean()),
                                        "max_abs_logit": float(ref_logits.abs().max()),
                                        "argmax_agreement": float((got.argmax(1) == ref_logits.argmax(1)).float().mean()),
                                        "n_points": int(ref_logits.shape[0])},
                "stated_tolerance": {"max_abs_logit_diff": 1e-1, "argmax_agreement": 0.99},
                "fwd_ms_per_step_fp32_storage": round(dt_f32 / args.steps * 1e3, 3)}
            del ref_logits, got
        else:
            _ops.STORAGE = "bf16"
    dt_f = n_pts_f = None
    if args.full or not train:
        dt_f, n_pts_f = timed(fwd_step, "fwd")  # forward-only eval (BASELINE configs[1] as literally worded)
        # (the instrumented passes below stay on the same stream: its allocator pool is warm, so no hipMalloc lands inside
        # an event bracket -- the narrow-head layers of the dense scene once read 11 ms instead of 1.1 ms that way)
    if not train:
        dt, n_pts = dt_f, n_pts_f
        if args.dump_outputs and rank == 0:
            dump_outputs(last["fwd"], args.dump_outputs)
    last.clear()

    rank_report = None
    if distributed:  # one record per rank: a scaling problem shows as one slow rank or as a large exchange share
        mine = {"rank": rank, "device": torch.cuda.get_device_name(dev) if dev.type == "cuda" else "cpu",
                "ms_per_step": round(local_sec["train" if train else "fwd"] / args.steps * 1e3, 3),
                "trained_weights_l1": weights_l1}
        if "fwd" in local_sec:
            mine["fwd_ms_per_step"] = round(local_sec["fwd"] / args.steps * 1e3, 3)
        rank_report = [None] * world
        dist.all_gather_object(rank_report, mine)
    out = None
    if rank == 0:
        model.eval()
        b0 = B.batch_from_resident(resident[0], offsets[0], ds.voxel_size, ds.point_cloud_range, images[0], cyl)
        if args.full:
            roof, per_layer = conv_roofline(model, b0, dev)
        if train:
            step_desc = ("fwd (attention dropout p=0.1, DropPath) + criterion (" + "+".join(cfg.MODEL.LOSSES)
                         + " on 3 heads) + bwd + SGD step")
        else:
            step_desc = "forward-only eval"
        out = {
            "metric": "points/sec fwd+bwd, Waymo 1-sweep ~180k pts @0.1m voxel; logit parity",
            "value": round(n_pts / dt, 1), "unit": "points/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": ("f32 storage/accumulate, bf16x3 products" + ("; training: bf16 copies of the weight-gradient operands saved for "
                                                                     "backward; fwd_only: bf16 storage of the sparse-conv feature maps"
                                                                     if args.storage == "bf16" else ""))
            if _ops.CONV_PRECISION == "bf16x3" else "f32",
            "data": "synthetic",
            "config": {"workload": WORKLOADS[args.workload] + (f", {cfg.DATASET.NUM_SWEEPS} sweeps = {int(resident[0].shape[0])} rows/step"
                                                               if args.workload == "multi_sweeps" else "") + ": synthetic scene, "
                                   f"{pts_per_step[0]} pts/step/GPU, voxel {ds.voxel_size}, grid {ds.grid_size.tolist()}, {step_desc}",
                       "mode": args.mode, "segmentor": args.segmentor, "scenes_per_step_per_gpu": args.batch,
                       "voxels": int(b0["voxel_coords"].shape[0]), "parallelism": f"dp{world}",
                       "collective": (f"{dist.get_backend()} world {dist.get_world_size()}" + (", SyncBatchNorm" if args.sync_bn else ""))
                       if distributed else None,
                       "streams": ("weight gradients + aux-label lookup on a second stream; "
                                   + ("batch i+1's voxelization and index plan on a third stream beside step i (same K "
                                      "voxelizations and plans inside the K timed steps)" if pipe_stream is not None
                                      else "every batch built at the start of its own step (--no-pipeline)"))},
        }
        if dt_f is not None:
            out["fwd_only"] = {"value": round(n_pts_f / dt_f, 1), "unit": "points/s", "ms_per_step": round(dt_f / args.steps * 1e3, 3)}
        if args.full:
            out["roofline"] = roof
            out["conv_layers"] = [{k: l[k] for k in ("rows", "cin", "cout", "us", "bound", "frac")} for l in per_layer]
            out["attention_roofline"] = ATTENTION_REPORT if args.segmentor == "segformer" else None
        if idle_report is not None:
            out["idle"] = idle_report
        if peak_bytes is not None:
            out["peak_memory_gb"] = round(peak_bytes / 2 ** 30, 3)
        if train_storage is not None:
            out["train_storage"] = train_storage
        if storage_report is not None:
            storage_report["fwd_speedup"] = round(storage_report["fwd_ms_per_step_fp32_storage"] / (dt_f / args.steps * 1e3), 3)
            out["storage"] = storage_report
        out["trained_weights_l1"] = weights_l1 if weights_l1 is not None else \
            float(sum(p.detach().double().abs().sum() for p in model.parameters()))
        if rank_report is not None:
            out["ranks"] = rank_report
            if nosync_ms is not None:
                out["allreduce"] = {"ms_per_step_without_exchange": round(nosync_ms, 3),
                                    "exposed_ms_per_step": round(dt / args.steps * 1e3 - nosync_ms, 3),
                                    "gradient_bytes": int(sum(p.numel() for p in model.parameters()) * 4),
                                    "wrapper": type(net).__name__,
                                    "note": "gradient exchange over " + dist.get_backend() + "; exposed = timed step minus the "
                                            "same step under no_sync()"}
        # the attention temperature after the timed steps: below ~0.036 the kernels leave the fixed-maximum softmax
        taus = [float(p.detach()) for n, p in model.named_parameters() if n.endswith(".tau")]
        if taus and out.get("attention_roofline") is not None:
            out["attention_roofline"]["tau_range_after_steps"] = [round(min(taus), 4), round(max(taus), 4)]
        profiled = any(k in os.environ for k in ("ROCPROFILER_SDK_TOOL_LIBRARIES", "ROCP_TOOL_LIBRARIES", "ROCPROF_OUTPUT_PATH")) \
            or "rocprof" in os.environ.get("LD_PRELOAD", "")
        if (args.full and train and world == 1 and not distributed and not profiled and not args.no_fp32_exact
                and _ops.CONV_PRECISION == "bf16x3" and args.workload == "one_sweep" and args.segmentor == "segformer"):
            # the same step with every conv / Linear product an exact fp32 MFMA (the reference's arithmetic), in a fresh child
            # process (the switch is read at import): the same-precision number, driver-recorded
            import subprocess
            # a fresh single-process child: no rendezvous variables of an outer launcher (torchrun with one rank would
            # collide on the port), and never a second process under a profiler that wraps this one
            env = {k: v for k, v in os.environ.items()
                   if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "MASTER_ADDR",
                                "MASTER_PORT", "TORCHELASTIC_RUN_ID", "SEG3D_BENCH_DIST")}
            env["SEG3D_CONV_PRECISION"] = "fp32"
            try:
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", "5", "--warmup", "2", "--scenes", "2",
                                        "--full", "--no-cpu-baseline", "--no-fp32-exact"], capture_output=True, text=True, timeout=600,
                                       env=env)
                fp32 = {"error": child.stderr[-300:]}
                for line in child.stdout.splitlines():
                    if line.startswith("{"):
                        d = json.loads(line)
                        fp32 = {"ms_per_step": d["ms_per_step"], "value": d["value"], "unit": d["unit"], "dtype": d["dtype"],
                                "fwd_only_ms_per_step": d["fwd_only"]["ms_per_step"], "steps": d["steps"],
                                "note": "SEG3D_CONV_PRECISION=fp32: v_mfma_f32_16x16x4_f32 products (1/16 of the bf16 MFMA rate)"}
            except (subprocess.SubprocessError, OSError, ValueError, KeyError, TypeError) as e:  # the record above must survive
                fp32 = {"error": f"{type(e).__name__}: {e}"[:300]}
            out["fp32_exact"] = fp32
        if baseline is not None:
            out["cpu_baseline"], out["parity"] = baseline
            # the trained module against a fresh module loaded from its state_dict: every cached operand (packed weights,
            # folded BatchNorm affines) must have followed the optimizer (fused optimizers do not bump Tensor._version)
            fresh = segformer.build_segmentor(cfg, ds).to(dev).eval()
            fresh.load_state_dict(model.state_dict())
            with torch.no_grad():
                a = model(B.batch_from_resident(resident[0], offsets[0], ds.voxel_size, ds.point_cloud_range, images[0], cyl))
                c = fresh(B.batch_from_resident(resident[0], offsets[0], ds.voxel_size, ds.point_cloud_range, images[0], cyl))
            out["parity"]["trained_vs_reloaded_max_abs_diff"] = float((a["point_out"] - c["point_out"]).abs().max())
            if train and parity_sample is not None:
                # the same comparison on the weights the run ENDS with (a second oracle forward on the host cores)
                _, o_res, o_coords, o_ids = cpu_baseline(*parity_sample, cfg, ds, model)
                after = parity_report(*parity_sample, ds, model, dev, o_res, o_coords, o_ids)
                out["parity"]["after_training"] = {k: after[k] for k in after if k.startswith("max_") or k.endswith("bit_exact")}
                out["parity"]["after_training"]["steps"] = args.steps + args.warmup + extra_steps
        if args.full:
            os.makedirs(os.path.dirname(LAYERS_JSON), exist_ok=True)
            with open(LAYERS_JSON, "w") as f:
                json.dump(per_layer, f, indent=1)
        print(json.dumps(out), flush=True)
    if hi is not None:
        torch.cuda.default_stream(dev).wait_stream(hi)
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
