"""Record the LR sequences of the reference's WarmupPolyLR into tests/golden/lr_schedules.npz.

    python tests/golden/make_golden_lr.py <root of the reference tree>

Runs only where the reference tree exists; the class is loaded by file path from
seg3d/models/optimizers/lr_scheduler.py and stepped over a 40-iteration schedule with 10 warm-up iterations, once per
variant: 'linear' warm-up, 'constant' warm-up, and linear warm-up with constant_ending = 0.1.  The record is the learning
rate in force at iterations 0 .. 40 for two parameter groups (base rates 0.05 and 0.002), float64, plus the schedule's
arguments.  tests/test_optim_host.py reads the record, never the reference.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_ITERS, WARMUP_ITERS, BASE_LRS = 40, 10, (0.05, 0.002)
VARIANTS = {
    "linear": dict(warmup_method="linear"),
    "constant": dict(warmup_method="constant"),
    "constant_ending": dict(warmup_method="linear", constant_ending=0.1),
}


def main(ref_root):
    spec = importlib.util.spec_from_file_location(
        "ref_lr_scheduler", os.path.join(ref_root, "seg3d", "models", "optimizers", "lr_scheduler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {"max_iters": np.int64(MAX_ITERS), "warmup_iters": np.int64(WARMUP_ITERS), "base_lrs": np.array(BASE_LRS)}
    for name, kw in VARIANTS.items():
        params = [torch.zeros(1, requires_grad=True) for _ in BASE_LRS]
        opt = torch.optim.SGD([{"params": [p], "lr": lr} for p, lr in zip(params, BASE_LRS)], lr=1.0)
        sched = mod.WarmupPolyLR(opt, max_iters=MAX_ITERS, warmup_iters=WARMUP_ITERS, **kw)
        rows = [[g["lr"] for g in opt.param_groups]]
        for _ in range(MAX_ITERS):
            opt.step()
            sched.step()
            rows.append([g["lr"] for g in opt.param_groups])
        out[name] = np.array(rows, dtype=np.float64)
    np.savez(os.path.join(HERE, "lr_schedules.npz"), **out)
    for name in VARIANTS:
        print(name, out[name][:3, 0], "...", out[name][-3:, 0])


if __name__ == "__main__":
    main(sys.argv[1])
