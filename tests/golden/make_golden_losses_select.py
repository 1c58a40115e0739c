#!/usr/bin/env python3
"""Generate tests/golden/losses_select.npz from the REFERENCE's own OHEMCrossEntropyLoss and from nn.CrossEntropyLoss(weight=)
(build container only; see make_golden.py).

Inputs: logits float32 [257, 22] = normal x 2.5, rows 0-7 scaled so that |logit| reaches 40 (very hard and very easy rows);
every 7th label is 255 (ignored); class 7 is absent from the labels; class_weight in [1, 11.5], the spread of the shipped
DATASET.CLASS_WEIGHT lists.

Cases: the reference module (seg3d/models/losses/ohem_cross_entropy_loss.py) {without, with class weights} x {no selector,
keep_thresh 0.7, keep_ratio 0.3}, and nn.CrossEntropyLoss(weight=, ignore_index=255).  Each runs twice: in float64, whose
value and input gradient are the expectation (<case>, <case>_grad), and in float32, whose deviation from the float64 run
is kept (<case>_fp32_val_err absolute, <case>_fp32_grad_err max-abs) as the error a float32 implementation of the same
formulas shows on these inputs.  The keep_ratio cases also store how many rows were kept and the float64 gap between the
last kept loss and the first one left out: the float32 run must (and does) select the same rows.

Usage:  python tests/golden/make_golden_losses_select.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (reference loader)

N, C = 257, 22
KEEP_THRESH, KEEP_RATIO = 0.7, 0.3


def load():
    for pkg in ("seg3d", "seg3d.models", "seg3d.models.losses"):
        if pkg not in sys.modules:
            mg._shell(pkg)
    return mg._load("seg3d.models.losses.ohem_cross_entropy_loss",
                    "seg3d/models/losses/ohem_cross_entropy_loss.py").OHEMCrossEntropyLoss


def inputs():
    g = torch.Generator().manual_seed(23)
    logits = torch.randn(N, C, generator=g) * 2.5
    logits[:8] *= 40.0 / logits[:8].abs().max()
    labels = torch.randint(0, C, (N,), generator=g)
    labels[labels == 7] = 12
    labels[::7] = 255
    weights = 1.0 + 10.5 * torch.rand(C, generator=g, dtype=torch.float64)
    return logits, labels, weights


def cases(OHEM, weights, dtype):
    """name -> module; the weights travel as a tensor of the run's dtype (nn.CrossEntropyLoss wants one)"""
    w = weights.to(dtype)
    return {
        "ohem_none": OHEM(),
        "ohem_thresh": OHEM(keep_thresh=KEEP_THRESH),
        "ohem_ratio": OHEM(keep_ratio=KEEP_RATIO),
        "ohem_weighted_none": OHEM(class_weight=w),
        "ohem_weighted_thresh": OHEM(keep_thresh=KEEP_THRESH, class_weight=w),
        "ohem_weighted_ratio": OHEM(keep_ratio=KEEP_RATIO, class_weight=w),
        "ce_weighted": torch.nn.CrossEntropyLoss(weight=w, ignore_index=255),
    }


def run(fn, logits, labels, dtype):
    x = logits.clone().to(dtype).requires_grad_(True)
    loss = fn(x, labels)
    loss.backward()
    return loss.detach().double().numpy(), x.grad.double().numpy()


def main():
    OHEM = load()
    logits, labels, weights = inputs()
    out = {"logits": logits.numpy(), "labels": labels.numpy(), "class_weight": weights.numpy(),
           "keep_thresh": np.float64(KEEP_THRESH), "keep_ratio": np.float64(KEEP_RATIO)}
    c64, c32 = cases(OHEM, weights, torch.float64), cases(OHEM, weights, torch.float32)
    for name in c64:
        val, grad = run(c64[name], logits, labels, torch.float64)
        val32, grad32 = run(c32[name], logits, labels, torch.float32)
        out[name], out[name + "_grad"] = val, grad
        out[name + "_fp32_val_err"] = np.abs(val32 - val)
        out[name + "_fp32_grad_err"] = np.abs(grad32 - grad).max()
        note = ""
        if name.endswith("ratio"):
            valid = labels != 255
            w = weights if "weighted" in name else None
            per_row = torch.nn.functional.cross_entropy(logits.double(), labels, weight=w, ignore_index=255,
                                                        reduction="none")[valid].sort(descending=True)[0]
            kept = int(per_row.shape[0] * KEEP_RATIO)
            gap = float(per_row[kept - 1] - per_row[kept])
            assert np.array_equal(grad.any(axis=1), grad32.any(axis=1)), "float32 selects other rows"
            assert int(grad.any(axis=1).sum()) == kept and gap > 1e-4
            out[name + "_kept"], out[name + "_gap"] = np.int64(kept), np.float64(gap)
            note = f"  kept {kept}  gap {gap:.2e}"
        print(f"{name}: {float(val):.12g}  grad |max| {np.abs(grad).max():.3e}  fp32 value err "
              f"{float(out[name + '_fp32_val_err']):.2e} ({float(out[name + '_fp32_val_err']) / abs(float(val)):.2e} rel)  "
              f"fp32 grad err {float(out[name + '_fp32_grad_err']):.2e}{note}")
    mg.save("losses_select.npz", **out)


if __name__ == "__main__":
    main()
