"""Per-kernel totals inside the training steps of a `rocprofv3 --kernel-trace --output-format csv` run of bench.py.

usage: python tools/trace_summary.py <kernel_trace.csv> [--steps N] [--csv out.csv] [--queue-csv out.csv] [--top 60]
       python tools/trace_summary.py --criterion <kernel_trace.csv[.gz]> [--steps N] [--csv out.csv]
Training steps are delimited by the optimizer's launches (fused SGD): the last N of them bound N steps.
--queue-csv writes the steps' kernels per queue (main = the optimizer's) in the columns of the --criterion table.
--criterion cuts the criterion interval of every step instead (criterion_interval below)."""
import argparse
import collections
import csv
import gzip
import re


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    m = re.match(r"([A-Za-z_0-9:]+(<[^(]*>)?)", name)
    return (m.group(1) if m else name)[:90]


def family(n):
    if "spconv_split_kernel<" in n and ", true," in n:
        return "Linear forward / dX (dense rows through the gather-GEMM)"
    for key, fam in (("spconv_tile_kernel<", "sparse conv gather-GEMM (fwd + dgrad)"), ("spconv_split_kernel<", "sparse conv gather-GEMM (fwd + dgrad)"),
                     ("plan_kernel", "index build + rest"), ("morton_keys", "index build + rest"), ("spconv_fwd_kernel", "exact-fp32 point MLP"),
                     ("wgrad", "weight gradients"), ("attn", "window attention"), ("tau_reduce", "window attention"),
                     ("ln_", "LayerNorm / BatchNorm passes"), ("col_", "LayerNorm / BatchNorm passes"), ("bn_", "LayerNorm / BatchNorm passes"),
                     ("affine_act", "LayerNorm / BatchNorm passes"), ("lovasz", "criterion + kNN"), ("ce_", "criterion + kNN"),
                     ("knn", "criterion + kNN"), ("radix", "criterion + kNN / sorts"), ("pack_weight", "packing"),
                     ("at::native", "torch elementwise / other"), ("multi_tensor", "optimizer")):
        if key in n:
            return fam
    return "index build + rest"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--csv")
    ap.add_argument("--queue-csv", help="kernel,queue,launches_per_step,us_per_step,us_per_launch of the training steps")
    ap.add_argument("--top", type=int, default=60)
    ap.add_argument("--criterion", action="store_true", help="the criterion interval of every step (criterion_interval)")
    a = ap.parse_args()
    if a.criterion:
        return criterion_interval(a.trace, a.steps, a.csv)
    rows = []
    with open(a.trace) as f:
        for r in csv.DictReader(f):
            rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "0")))
    rows.sort(key=lambda r: r[1])
    # the optimizer's own launches only: `_foreach_add_` on the BatchNorm step counters is a multi_tensor_apply kernel too
    opt = [i for i, r in enumerate(rows) if "FusedSgd" in r[0] or "fused_sgd" in r[0].lower()]
    groups = []
    for i in opt:
        if groups and rows[i][1] - rows[groups[-1][-1]][2] < 1_000_000:
            groups[-1].append(i)
        else:
            groups.append([i])
    assert len(groups) > a.steps, f"only {len(groups)} optimizer steps in the trace"
    first = groups[-a.steps - 1][-1] + 1
    last = groups[-1][-1]
    win = rows[first:last + 1]
    span = (win[-1][2] - win[0][1]) / 1e6 / a.steps
    tot = collections.defaultdict(lambda: [0, 0])
    fam = collections.defaultdict(float)
    for n, s, e, _ in win:
        k = short(n)
        tot[k][0] += 1
        tot[k][1] += e - s
        fam[family(k)] += e - s
    busy = sum(v[1] for v in tot.values()) / 1e6 / a.steps
    print(f"{a.steps} training steps: {span:.2f} ms per step wall (first launch to last end), {busy:.2f} ms kernel-busy, "
          f"{len(win) / a.steps:.0f} launches per step")
    for k, v in sorted(fam.items(), key=lambda kv: -kv[1]):
        print(f"  {v / 1e6 / a.steps:7.2f} ms {100 * v / 1e6 / a.steps / busy:5.1f} %  {k}")
    out = sorted(tot.items(), key=lambda kv: -kv[1][1])
    print("launches/step   ms/step   us/launch  kernel")
    for k, (c, ns) in out[: a.top]:
        print(f"{c / a.steps:10.1f} {ns / 1e6 / a.steps:10.3f} {ns / 1e3 / c:10.1f}  {k}")
    if a.csv:
        with open(a.csv, "w") as f:
            f.write("kernel,launches_per_step,ms_per_step,us_per_launch,share\n")
            for k, (c, ns) in out:
                f.write(f"\"{k}\",{c / a.steps:.2f},{ns / 1e6 / a.steps:.4f},{ns / 1e3 / c:.2f},{ns / 1e6 / a.steps / busy:.4f}\n")


    if a.queue_csv:
        main_q = rows[last][3]
        per = collections.defaultdict(lambda: [0, 0])
        for n, s, e, q in win:
            key = (short(n), "main" if q == main_q else "other")
            per[key][0] += 1
            per[key][1] += e - s
        with open(a.queue_csv, "w") as f:
            f.write("kernel,queue,launches_per_step,us_per_step,us_per_launch\n")
            for (n, q), (cnt, ns) in sorted(per.items(), key=lambda kv: -kv[1][1]):
                f.write(f"\"{n}\",{q},{cnt / a.steps:.2f},{ns / 1e3 / a.steps:.2f},{ns / 1e3 / cnt:.2f}\n")
            f.write(f"\"# wall_us per step\",,,{span * 1e3:.2f},\n")
            f.write(f"\"# busy_us per step (sum over kernels)\",,,{busy * 1e3:.2f},\n")


def criterion_interval(trace, steps, out_csv):
    """--criterion: the part of every step between the classifier's last GEMM and the backward's first kernel (the criterion
    kernels `ce_bwd_kernel` / `lovasz_bwd` / `criterion_bwd_kernel`).  Per kernel: launches and time per step, with the
    queue it ran on (main = the criterion's own); then the interval's length, launches, busy time (union over all
    queues), the sum of gaps, and the Lovasz sort calls on their own: the rocPRIM kernels of the MAIN queue (the index
    build's sorts run on the other streams) with the buffer fills between them, their number of calls (runs between two
    other kernels), launches, kernel time and wall time from the first to the last kernel of each call."""
    rows = []
    with (gzip.open(trace, "rt") if trace.endswith(".gz") else open(trace)) as f:
        for r in csv.DictReader(f):
            rows.append((short(r["Kernel_Name"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "0")))
    rows.sort(key=lambda r: r[1])
    first_crit = ("ce_fwd_kernel", "lovasz_keys", "criterion_rows_kernel")
    first_bwd = ("ce_bwd_kernel", "lovasz_bwd", "criterion_bwd_kernel")
    bwd = [i for i, r in enumerate(rows) if r[0].startswith(first_bwd)]
    starts = []  # first backward kernel of every step: one per run of criterion-backward kernels
    for i in bwd:
        if not starts or rows[i][1] - rows[starts[-1]][1] > 5_000_000:
            starts.append(i)
    assert len(starts) >= steps, f"only {len(starts)} criterion backward passes in the trace"
    tot = collections.defaultdict(lambda: [0, 0])
    agg = collections.defaultdict(float)
    for b in starts[-steps:]:
        t1 = rows[b][1]
        # this step's first criterion kernel (the previous step's lies a whole backward and forward earlier)
        c = min(i for i in range(b + 1) if rows[i][0].startswith(first_crit + first_bwd) and t1 - rows[i][1] < 20_000_000)
        main_q = rows[c][3]
        # the classifier's last kernel: its second Linear, a rocBLAS (Cijk_) or library GEMM
        g = max(i for i in range(c) if rows[i][0].startswith(("Cijk_", "spconv_", "linear_")) and rows[i][3] == main_q)
        t0 = rows[g][2]
        win = [r for r in rows if t0 <= r[1] < t1]
        busy, end = 0, t0
        for _, s, e, _ in win:
            if e > end:
                busy += e - max(s, end)
                end = e
        agg["interval_us"] += (t1 - t0) / 1e3
        agg["launches"] += len(win)
        agg["busy_us"] += busy / 1e3
        agg["gap_sum_us"] += (t1 - t0 - busy) / 1e3
        run = []  # a sort call: consecutive rocPRIM kernels and the buffer fills (histogram resets) between them
        for n, s, e, q in win + [("end", t1, t1, main_q)]:
            if n != "end":
                tot[(n, "main" if q == main_q else "other")][0] += 1
                tot[(n, "main" if q == main_q else "other")][1] += e - s
            if q != main_q:
                continue
            if "rocprim" in n or "fillBuffer" in n:
                run.append((n, s, e))
                continue
            while run and "rocprim" not in run[-1][0]:
                run.pop()
            if run:
                agg["lovasz_sort_calls"] += 1
                agg["lovasz_sort_launches"] += len(run)
                agg["lovasz_sort_kernel_us"] += sum(e - s for _, s, e in run) / 1e3
                agg["lovasz_sort_wall_us"] += (run[-1][2] - run[0][1]) / 1e3
            run = []
    lines = ["kernel,queue,launches_per_step,us_per_step,us_per_launch"]
    for (n, q), (cnt, ns) in sorted(tot.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"\"{n}\",{q},{cnt / steps:.2f},{ns / 1e3 / steps:.2f},{ns / 1e3 / cnt:.2f}")
    for k in ("interval_us", "launches", "busy_us", "gap_sum_us", "lovasz_sort_calls", "lovasz_sort_launches",
              "lovasz_sort_kernel_us", "lovasz_sort_wall_us"):
        lines.append(f"\"# {k} per step\",,,{agg[k] / steps:.2f},")
    print("\n".join(lines))
    if out_csv:
        with open(out_csv, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
