"""Plain float64 reference of the row-wise normalisation layers, written from the formulas (no torch.nn module, no
autograd): BatchNorm1d over [rows, c] with an optional residual and ReLU, LayerNorm with a residual and a per-row scale,
and the "ranks" form of BatchNorm -- one BatchNorm over the concatenation of several row blocks, returned per block, which
is what SyncBatchNorm computes.  tests/test_norm_ref_host.py checks it against torch's own fp64 modules and autograd.

Every function takes CPU tensors of any float type, computes in float64 and returns a SimpleNamespace of float64 tensors."""
from types import SimpleNamespace

import torch


def _d(t):
    return None if t is None else t.detach().to(torch.float64)


def batch_norm(x, gamma, beta, eps, res=None, relu=False, dy=None, running_mean=None, running_var=None, momentum=0.1,
               num_batches_tracked=0, training=True):
    """act(BatchNorm(x) (+ res)).  Training: batch statistics (biased variance); the running buffers are updated as torch
    updates them -- unbiased variance, momentum=None = the cumulative average 1 / (batches seen, this one included).
    Eval: the running buffers normalise.  With dy: dx, dres, dgamma, dbeta of sum(y * dy).
    ``pre`` is the value the ReLU sees; a test must keep it away from zero."""
    x, gamma, beta, res, dy = _d(x), _d(gamma), _d(beta), _d(res), _d(dy)
    m = x.shape[0]
    out = SimpleNamespace()
    if training:
        mean = x.sum(0) / m
        var = ((x - mean) ** 2).sum(0) / m
        out.mean, out.var = mean, var
        out.var_unbiased = var * m / (m - 1) if m > 1 else var
        if running_mean is not None:
            out.num_batches_tracked = int(num_batches_tracked) + 1
            mom = 1.0 / out.num_batches_tracked if momentum is None else float(momentum)
            out.running_mean = _d(running_mean) * (1 - mom) + mean * mom
            out.running_var = _d(running_var) * (1 - mom) + out.var_unbiased * mom
    else:
        mean, var = _d(running_mean), _d(running_var)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    pre = xhat * gamma + beta
    if res is not None:
        pre = pre + res
    out.pre = pre
    out.y = pre.clamp(min=0.0) if relu else pre
    if dy is not None:
        g = dy * (pre > 0) if relu else dy
        out.dres = g if res is not None else None
        out.dbeta = g.sum(0)
        out.dgamma = (g * xhat).sum(0)
        if training:
            out.dx = gamma * rstd * (g - out.dbeta / m - xhat * (out.dgamma / m))
        else:
            out.dx = gamma * rstd * g
    return out


def batch_norm_ranks(xs, gamma, beta, eps, ress=None, relu=False, dys=None):
    """One training-mode BatchNorm over the rows of all blocks ``xs`` (a block may have no rows).  Lists per block: y, pre,
    dx, dres, and the block-local dgamma_local / dbeta_local (what each rank keeps); mean, var, var_unbiased, dgamma and dbeta
    belong to the union."""
    rows = [int(x.shape[0]) for x in xs]

    def cat(ts):
        return None if ts is None else torch.cat([_d(t) for t in ts])

    full = batch_norm(cat(xs), gamma, beta, eps, res=cat(ress), relu=relu, dy=cat(dys))
    out = SimpleNamespace(mean=full.mean, var=full.var, var_unbiased=full.var_unbiased, rows=rows)

    def split(t):
        return None if t is None else list(torch.split(t, rows))

    out.y, out.pre = split(full.y), split(full.pre)
    if dys is not None:
        out.dx, out.dres = split(full.dx), split(full.dres)
        out.dgamma, out.dbeta = full.dgamma, full.dbeta
        rstd = 1.0 / torch.sqrt(full.var + eps)
        out.dgamma_local, out.dbeta_local = [], []
        for x, pre, dy in zip(xs, out.pre, dys):
            g = _d(dy) * (pre > 0) if relu else _d(dy)
            out.dbeta_local.append(g.sum(0))
            out.dgamma_local.append((g * (_d(x) - full.mean) * rstd).sum(0))
    return out


def layer_norm(x, gamma, beta, eps, res=None, rowscale=None, dy=None):
    """y = res + rowscale[:, None] * (LayerNorm(x) * gamma + beta) over the last dim (res, rowscale optional; rowscale
    carries no gradient).  With dy: dx, dres (= dy), dgamma, dbeta of sum(y * dy)."""
    x, gamma, beta, res, dy = _d(x), _d(gamma), _d(beta), _d(res), _d(dy)
    c = x.shape[1]
    s = torch.ones(x.shape[0], 1, dtype=torch.float64) if rowscale is None else _d(rowscale).reshape(-1, 1)
    mean = x.sum(1, keepdim=True) / c
    var = ((x - mean) ** 2).sum(1, keepdim=True) / c
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    y = s * (xhat * gamma + beta)
    out = SimpleNamespace(mean=mean[:, 0], rstd=rstd[:, 0], y=y if res is None else res + y)
    if dy is not None:
        ds = dy * s
        out.dres = dy if res is not None else None
        out.dbeta = ds.sum(0)
        out.dgamma = (ds * xhat).sum(0)
        gy = ds * gamma
        out.dx = rstd * (gy - gy.sum(1, keepdim=True) / c - xhat * ((gy * xhat).sum(1, keepdim=True) / c))
    return out


# Row 0 as an outlier of its column (the shift of the kernels' statistics): the relative error of the batch variance is
# bounded by OUTLIER_K * 2^-24 * (1 + delta^2), delta = (x[0] - mean) / sigma.  shifted_stats_fp32 on outlier_input(delta),
# against float64, measures 2.92, 5.32, 6.56 and 5.92 of those units at delta = 0, 8, 30, 100 (relative errors 1.7e-7, 2.1e-5,
# 3.5e-4, 3.5e-3); K is four times the largest, the margin being for the kernel's other order of summation.
OUTLIER_DELTAS = (0, 8, 30, 100)
OUTLIER_K = 26.3


def outlier_input(delta, m=20000, c=64):
    """float32 [m, c] rows of O(1) with a non-zero column mean whose row 0 sits at mean + delta * sigma of its column, mean and
    sigma being those of the whole column, row 0 included: with mu, s of the other rows that is x[0] = mu + t s,
    t^2 = delta^2 m / (m - 1 - delta^2)."""
    assert delta * delta < m - 1
    gen = torch.Generator().manual_seed(20000 + int(delta))
    x = torch.randn(m, c, generator=gen) * (0.5 + 2.0 * torch.rand(c, generator=gen)) + 3.0 * torch.randn(c, generator=gen)
    xd = x[1:].double()
    t = (delta * delta * m / (m - 1.0 - delta * delta)) ** 0.5
    x[0] = (xd.mean(0) + t * xd.std(0, unbiased=False)).float()
    return x


def shifted_stats_fp32(x):
    """(mean, biased variance) by the kernels' formula, evaluated in float32 on the CPU with torch's order of summation:
    s1 = sum(x - x[0]), s2 = sum((x - x[0])^2), mean = x[0] + s1 / m, var = max(s2 / m - (s1 / m)^2, 0)."""
    x = x.detach().to(torch.float32)
    m = x.shape[0]
    d = x - x[0]
    s1, s2 = d.sum(0), (d * d).sum(0)
    inv_m = torch.tensor(1.0 / m, dtype=torch.float32)
    dm = s1 * inv_m
    return x[0] + dm, (s2 * inv_m - dm * dm).clamp(min=0.0)
