#!/usr/bin/env python3
"""Generate tests/golden/losses_pointwise.npz from the REFERENCE's own FocalLoss and DiceLoss (build container only; see
make_golden.py).

Inputs: logits float32 [200, 22] = normal x 2.5, rows 0-7 scaled so that |logit| reaches 40 (sigmoid and log1p saturate
both ways); every 7th label is 255 (ignored); class 7 is absent from the labels; class_weight in [0.5, 1.5].

Per case the reference module (seg3d/models/losses/focal_loss.py, dice_loss.py) runs twice: in float64, whose value and
input gradient are the expectation (<case>, <case>_grad), and in float32, whose deviation from the float64 run is kept
(<case>_fp32_val_err absolute, <case>_fp32_grad_err max-abs) as the error a float32 implementation of the same formulas
shows on these inputs.

One stand-in, for the float64 run of FocalLoss only: focal_loss.py:77 casts the one-hot target to float32, and
F.binary_cross_entropy_with_logits returns the TARGET's dtype, so float64 logits would still get a float32 BCE term
(4e-10 relative on the mean here).  For that run the module's ``F`` hands the target over in the logits' dtype; the
float32 run is the module as it is.

Usage:  python tests/golden/make_golden_losses_pointwise.py
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (reference loader)

N, C = 200, 22


def load():
    for pkg in ("seg3d", "seg3d.utils", "seg3d.models", "seg3d.models.losses"):
        if pkg not in sys.modules:
            mg._shell(pkg)
    mg._load("seg3d.utils.loss_utils", "seg3d/utils/loss_utils.py")
    focal = mg._load("seg3d.models.losses.focal_loss", "seg3d/models/losses/focal_loss.py")
    dice = mg._load("seg3d.models.losses.dice_loss", "seg3d/models/losses/dice_loss.py")
    return focal, dice.DiceLoss


@contextlib.contextmanager
def bce_in_input_dtype(focal_module):
    functional = focal_module.F

    def bce(inputs, targets, **kwargs):
        return functional.binary_cross_entropy_with_logits(inputs, targets.to(inputs.dtype), **kwargs)

    focal_module.F = types.SimpleNamespace(one_hot=functional.one_hot, binary_cross_entropy_with_logits=bce)
    try:
        yield
    finally:
        focal_module.F = functional


def inputs():
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(N, C, generator=g) * 2.5
    logits[:8] *= 40.0 / logits[:8].abs().max()
    labels = torch.randint(0, C, (N,), generator=g)
    labels[labels == 7] = 12
    labels[::7] = 255
    weights = 0.5 + torch.rand(C, generator=g)
    assert float(logits[:8].abs().max()) >= 39.99 and bool((logits[:8] > 30).any()) and bool((logits[:8] < -30).any())
    return logits, labels, weights.tolist()


def cases(FocalLoss, DiceLoss, weights):
    """name -> (module, forward keyword arguments)"""
    return {
        "focal_default": (FocalLoss(num_classes=C), {}),
        "focal_weighted_sum": (FocalLoss(alpha=0.25, gamma=1.5, num_classes=C, class_weight=weights, reduction="sum"), {}),
        "focal_no_alpha": (FocalLoss(alpha=-1.0, num_classes=C), {}),
        "focal_gamma0": (FocalLoss(gamma=0.0, num_classes=C), {}),
        "dice_default": (DiceLoss(), {}),
        "dice_weighted": (DiceLoss(exponent=3, smooth=0.5, class_weight=weights, loss_weight=0.7), {}),
        "dice_avg_factor": (DiceLoss(), {"avg_factor": 3.0}),
    }


def run(fn, kwargs, logits, labels, dtype):
    x = logits.clone().to(dtype).requires_grad_(True)
    loss = fn(x, labels, **kwargs)
    loss.backward()
    return loss.detach().double().numpy(), x.grad.double().numpy()


def main():
    focal_module, DiceLoss = load()
    logits, labels, weights = inputs()
    out = {"logits": logits.numpy(), "labels": labels.numpy(), "class_weight": np.asarray(weights, np.float64)}
    for name, (fn, kwargs) in cases(focal_module.FocalLoss, DiceLoss, weights).items():
        with bce_in_input_dtype(focal_module):
            val, grad = run(fn, kwargs, logits, labels, torch.float64)
        val32, grad32 = run(fn, kwargs, logits, labels, torch.float32)
        out[name], out[name + "_grad"] = val, grad
        out[name + "_fp32_val_err"] = np.abs(val32 - val)
        out[name + "_fp32_grad_err"] = np.abs(grad32 - grad).max()
        print(f"{name}: {float(val):.12g}  grad |max| {np.abs(grad).max():.3e}  fp32 value err "
              f"{float(out[name + '_fp32_val_err']):.2e} ({float(out[name + '_fp32_val_err']) / abs(float(val)):.2e} rel)  "
              f"fp32 grad err {float(out[name + '_fp32_grad_err']):.2e}")
    mg.save("losses_pointwise.npz", **out)


if __name__ == "__main__":
    main()
