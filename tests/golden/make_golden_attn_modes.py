#!/usr/bin/env python3
"""Generate tests/golden/attn_modes.npz from the REFERENCE's own CosineMultiheadAttention (build container only; see
make_golden.py): the two constructor options the shared-tau fixture (cosine_msa.npz) does not cover.

Module: E = 48, 8 heads, eval mode.  Windows of 1, 5, 17 and 33 tokens padded to T = 33 with a key-padding mask,
q = k = x + pos, v = x (point_transformer_layer.py:233-258).  Inputs and parameters are drawn in float32 and stored as
float32 (every run upcasts the same values); only the valid tokens are stored, window after window (x, pos, g: [56, 48]).
  case `perhead`: non_shared_tau=True, tau = [1, 0.5, 0.2, 0.1, 0.05, 0.02, 0.011, 0.004] (the last below tau_min = 0.01)
  case `dot`:     cosine=False
Per case, float64 on the CPU: the output at the valid tokens (<case>_out) and, for the upstream gradient g (loss =
sum(out * g) over the valid tokens), the gradients of x, in_proj_weight, in_proj_bias, out_proj.weight and tau
(<case>_g_x, _g_in_w, _g_in_b, _g_out_w, _g_tau).  The same run in float32: its output and tau gradient as arrays
(<case>_f32_out, _f32_g_tau) and the max-abs deviation of every quantity from the float64 run (<case>_f32_err_<name>), the
error a float32 evaluation of the same formulas shows on these inputs -- the yardstick of the module test.

Usage:  python tests/golden/make_golden_attn_modes.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (reference loader)

E, HEADS, T, TAU_MIN = 48, 8, 33, 0.01
SIZES = (1, 5, 17, 33)
TAUS = (1.0, 0.5, 0.2, 0.1, 0.05, 0.02, 0.011, 0.004)


def load():
    for pkg in ("seg3d", "seg3d.models", "seg3d.models.layers"):
        if pkg not in sys.modules:
            mg._shell(pkg)
    return mg._load("seg3d.models.layers.cosine_msa", "seg3d/models/layers/cosine_msa.py").CosineMultiheadAttention


def inputs():
    g = torch.Generator().manual_seed(41)
    n = sum(SIZES)
    x = torch.randn(n, E, generator=g)
    pos = torch.randn(n, E, generator=g) * 0.5
    up = torch.randn(n, E, generator=g)
    par = {"in_proj_weight": torch.randn(3 * E, E, generator=g) * 0.2, "in_proj_bias": torch.randn(3 * E, generator=g) * 0.1,
           "out_proj.weight": torch.randn(E, E, generator=g) * 0.2, "out_proj.bias": torch.randn(E, generator=g) * 0.1}
    return x, pos, up, par


def padded(flat, dtype):
    """[n, E] valid tokens, window after window -> [T, W, E] (batch_first=False), zeros at the padding"""
    out = torch.zeros(T, len(SIZES), E, dtype=dtype)
    s = 0
    for w, n in enumerate(SIZES):
        out[:n, w] = flat[s:s + n].to(dtype)
        s += n
    return out


def valid(t):
    return torch.cat([t[:n, w] for w, n in enumerate(SIZES)])


def run(Msa, case, dtype):
    x, pos, up, par = inputs()
    kw = dict(cosine=True, non_shared_tau=True) if case == "perhead" else dict(cosine=False)
    msa = Msa(E, HEADS, dropout=0.1, batch_first=False, tau_min=TAU_MIN, **kw).to(dtype).eval()
    with torch.no_grad():
        for k, v in par.items():
            dict(msa.named_parameters())[k].copy_(v.to(dtype))
        if case == "perhead":
            msa.tau.copy_(torch.tensor(TAUS, dtype=dtype).reshape(1, HEADS, 1, 1))
    xp = padded(x, dtype).requires_grad_()
    pp = padded(pos, dtype)
    pad = torch.ones(len(SIZES), T, dtype=torch.bool)
    for w, n in enumerate(SIZES):
        pad[w, :n] = False
    y, _ = msa(xp + pp, xp + pp, value=xp, key_padding_mask=pad)
    out = valid(y)
    (out * up.to(dtype)).sum().backward()
    res = {"out": out.detach(), "g_x": valid(xp.grad), "g_in_w": msa.in_proj_weight.grad, "g_in_b": msa.in_proj_bias.grad,
           "g_out_w": msa.out_proj.weight.grad}
    if case == "perhead":
        res["g_tau"] = msa.tau.grad
    return res


def main():
    Msa = load()
    x, pos, up, par = inputs()
    data = {"x": x.numpy(), "pos": pos.numpy(), "g": up.numpy(), "sizes": np.array(SIZES, np.int64),
            "tau": np.array(TAUS, np.float64), "meta": np.array([E, HEADS, T], np.int64), "tau_min": np.float64(TAU_MIN)}
    data.update({"param_" + k.replace(".", "_"): v.numpy() for k, v in par.items()})
    for case in ("perhead", "dot"):
        r64, r32 = run(Msa, case, torch.float64), run(Msa, case, torch.float32)
        for k, v in r64.items():
            data[f"{case}_{k}"] = v.numpy()
            data[f"{case}_f32_err_{k}"] = np.float64((r32[k].double() - v).abs().max())
        data[f"{case}_f32_out"] = r32["out"].numpy()
        if "g_tau" in r32:
            data[f"{case}_f32_g_tau"] = r32["g_tau"].numpy()
    path = os.path.join(HERE, "attn_modes.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(data):
        if "_f32_err_" in k:
            print(f"  {k:28s} {float(data[k]):.3e}")


if __name__ == "__main__":
    main()
