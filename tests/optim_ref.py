"""Shared by tests/test_optim_host.py and tests/test_gpu_optim.py: the tensor sizes at which the multi-tensor optimizer
step can go wrong, a float64 restatement of its two algorithms, and the error measure (units in the last place)."""
import math

import numpy as np
import torch


def sizes(block):
    """Element counts: below / at / above one vector, one wave, one workgroup chunk (``block`` elements), two chunks and a
    tail; plus an empty tensor."""
    return [1, 3, 4, 5, 63, 64, 65, block - 1, block, block + 1, 2 * block + 7, 0]


SHAPES = [(48, 3, 3, 3, 48), (96, 48)]  # a sparse-conv weight and a Linear weight

SGD_GROUPS = [dict(lr=0.05, weight_decay=1e-4, momentum=0.9), dict(lr=0.013, weight_decay=0.0, momentum=0.8)]
ADAMW_GROUPS = [dict(lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8),
                dict(lr=3e-3, weight_decay=0.1, betas=(0.85, 0.99), eps=1e-6)]


def make_params(block, seed=0):
    """float32 CPU tensors (no grad): the sizes above as vectors, then the two weight shapes."""
    gen = torch.Generator().manual_seed(seed)
    shapes = [(n,) for n in sizes(block)] + SHAPES
    return [torch.randn(*s, generator=gen) for s in shapes]


def make_grads(params, step, seed=100):
    gen = torch.Generator().manual_seed(seed + step)
    return [torch.randn(*p.shape, generator=gen) * 0.5 for p in params]


def split_groups(params, group_kw):
    """Alternate the tensors over the groups, so that every group holds small and large ones."""
    groups = [dict(kw, params=[]) for kw in group_kw]
    for i, p in enumerate(params):
        groups[i % len(groups)]["params"].append(p)
    return groups


class Ref64:
    """The algorithms of include/seg3d_hip.h (seg3d_optim_step) in float64.  The scalars (decay factor, bias corrections
    from each parameter's own step count) are restated here from the hyper-parameters and take nothing from
    openseg3d_amd.optim, so a wrong scalar there moves the code under test away from this reference.
    ``grads[i] is None`` skips parameter i: no state, no step count."""

    def __init__(self, algo, params, group_of, group_kw):
        self.algo, self.group_of, self.group_kw = algo, group_of, group_kw
        self.p = [p.double().clone() for p in params]
        self.m = [None] * len(params)
        self.v = [None] * len(params)
        self.steps = [0] * len(params)

    def step(self, grads):
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = g.double()
            kw = self.group_kw[self.group_of[i]]
            self.steps[i] += 1
            if self.algo == "sgd":
                lr, wd, mu = float(kw["lr"]), float(kw["weight_decay"]), float(kw["momentum"])
                if wd != 0:
                    g = g + wd * self.p[i]
                if mu != 0:
                    self.m[i] = g.clone() if self.m[i] is None else mu * self.m[i] + g
                    g = self.m[i]
                self.p[i] = self.p[i] - lr * g
            else:
                lr, wd, eps, (beta1, beta2), t = kw["lr"], kw["weight_decay"], kw["eps"], kw["betas"], self.steps[i]
                bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t  # the bias corrections of this parameter's own step count
                if self.m[i] is None:
                    self.m[i], self.v[i] = torch.zeros_like(g), torch.zeros_like(g)
                self.p[i] = self.p[i] * (1.0 - lr * wd)
                self.m[i] = self.m[i] + (g - self.m[i]) * (1.0 - beta1)
                self.v[i] = self.v[i] * beta2 + (1.0 - beta2) * g * g
                self.p[i] = self.p[i] - (lr / bc1) * self.m[i] / (self.v[i].sqrt() / math.sqrt(bc2) + eps)


def ulp_error(got32, ref64):
    """max |got - ref| / ulp(|ref|), ulp taken in float32 at the reference value; 0 for an empty tensor."""
    if ref64.numel() == 0:
        return 0.0
    ref = ref64.detach().cpu().numpy().astype(np.float64)
    got = got32.detach().cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got - ref) / ulp))
