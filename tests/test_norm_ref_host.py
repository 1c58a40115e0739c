"""tests/norm_ref.py, the fp64 reference of the norm-kernel tests, is itself checked (no GPU): its BatchNorm, LayerNorm and
"ranks" forms against torch's own float64 modules with autograd, to 1e-12; the float32 emulation of the kernels' shifted
statistics against float64 under the bound the GPU outlier test uses."""
import pytest
import torch
import torch.nn as nn

import norm_ref

TOL = 1e-12


def _err(a, b):
    return float((a - b).abs().max()) if a.numel() else 0.0


def _bn_pair(c, eps, momentum, gen):
    ref = nn.BatchNorm1d(c, eps=eps, momentum=momentum).double()
    with torch.no_grad():
        ref.weight.copy_(1 + 0.2 * torch.randn(c, generator=gen, dtype=torch.float64))
        ref.bias.copy_(0.1 * torch.randn(c, generator=gen, dtype=torch.float64))
        ref.running_mean.copy_(torch.randn(c, generator=gen, dtype=torch.float64))
        ref.running_var.copy_(0.5 + torch.rand(c, generator=gen, dtype=torch.float64))
    return ref


@pytest.mark.parametrize("m,c", [(2, 4), (3, 8), (17, 12), (50, 36)])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("momentum", [0.01, None])
def test_batch_norm_matches_torch_fp64(m, c, relu, with_res, momentum):
    gen = torch.Generator().manual_seed(m * 100 + c)
    x = torch.randn(m, c, generator=gen, dtype=torch.float64) * 1.5 + 3.0
    r = torch.randn(m, c, generator=gen, dtype=torch.float64)
    g = torch.randn(m, c, generator=gen, dtype=torch.float64)
    ref = _bn_pair(c, 1e-3, momentum, gen)
    rm, rv, nbt = ref.running_mean.clone(), ref.running_var.clone(), 0
    for _ in range(2):  # two training passes: momentum=None averages over both
        ref.train().zero_grad()
        xr, rr = x.clone().requires_grad_(), r.clone().requires_grad_()
        pre = ref(xr) + (rr if with_res else 0)
        y = torch.relu(pre) if relu else pre
        y.backward(g)
        o = norm_ref.batch_norm(x, ref.weight, ref.bias, 1e-3, res=r if with_res else None, relu=relu, dy=g, running_mean=rm,
                                running_var=rv, momentum=momentum, num_batches_tracked=nbt)
        rm, rv, nbt = o.running_mean, o.running_var, o.num_batches_tracked
        assert _err(o.y, y.detach()) < TOL and _err(o.pre, pre.detach()) < TOL
        assert _err(o.dx, xr.grad) < TOL
        assert (o.dres is None) == (not with_res)
        if with_res:
            assert _err(o.dres, rr.grad) < TOL
        assert _err(o.dgamma, ref.weight.grad) < TOL and _err(o.dbeta, ref.bias.grad) < TOL
        assert _err(rm, ref.running_mean) < TOL and _err(rv, ref.running_var) < TOL
        assert nbt == int(ref.num_batches_tracked)
        x = x * 0.7 + 1.0
    # eval: the running buffers normalise
    ref.eval().zero_grad()
    xr = x.clone().requires_grad_()
    pre = ref(xr) + (r if with_res else 0)
    y = torch.relu(pre) if relu else pre
    y.backward(g)
    o = norm_ref.batch_norm(x, ref.weight, ref.bias, 1e-3, res=r if with_res else None, relu=relu, dy=g, running_mean=rm,
                            running_var=rv, training=False)
    assert _err(o.y, y.detach()) < TOL and _err(o.dx, xr.grad) < TOL
    assert _err(o.dgamma, ref.weight.grad) < TOL and _err(o.dbeta, ref.bias.grad) < TOL


@pytest.mark.parametrize("m,c", [(1, 4), (1, 96), (5, 8), (33, 28), (40, 260)])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("with_scale", [True, False])
def test_layer_norm_matches_torch_fp64(m, c, with_res, with_scale):
    gen = torch.Generator().manual_seed(m * 1000 + c)
    x = torch.randn(m, c, generator=gen, dtype=torch.float64) * 2 + 0.5
    r = torch.randn(m, c, generator=gen, dtype=torch.float64)
    g = torch.randn(m, c, generator=gen, dtype=torch.float64)
    scale = (torch.rand(m, generator=gen) < 0.8).double() / 0.8 if with_scale else None
    ln = nn.LayerNorm(c).double()
    with torch.no_grad():
        ln.weight.copy_(1 + 0.2 * torch.randn(c, generator=gen, dtype=torch.float64))
        ln.bias.copy_(0.1 * torch.randn(c, generator=gen, dtype=torch.float64))
    xr, rr = x.clone().requires_grad_(), r.clone().requires_grad_()
    y = ln(xr)
    if with_scale:
        y = y * scale[:, None]
    if with_res:
        y = rr + y
    y.backward(g)
    o = norm_ref.layer_norm(x, ln.weight, ln.bias, ln.eps, res=r if with_res else None, rowscale=scale, dy=g)
    assert _err(o.y, y.detach()) < TOL and _err(o.dx, xr.grad) < TOL
    assert (o.dres is None) == (not with_res)
    if with_res:
        assert _err(o.dres, rr.grad) < TOL
    assert _err(o.dgamma, ln.weight.grad) < TOL and _err(o.dbeta, ln.bias.grad) < TOL


@pytest.mark.parametrize("rows", [[1, 7, 20], [2, 0, 31], [0, 1, 4]])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
def test_batch_norm_ranks_matches_torch_fp64_on_the_concatenation(rows, relu, with_res):
    c = 8
    gen = torch.Generator().manual_seed(sum(rows))
    xs = [torch.randn(n, c, generator=gen, dtype=torch.float64) * (1 + 0.5 * i) + 0.3 * i for i, n in enumerate(rows)]
    rs = [torch.randn(n, c, generator=gen, dtype=torch.float64) for n in rows]
    gs = [torch.randn(n, c, generator=gen, dtype=torch.float64) for n in rows]
    ref = _bn_pair(c, 1e-3, 1.0, gen).train()
    xa, ra = torch.cat(xs).requires_grad_(), torch.cat(rs).requires_grad_()
    pre = ref(xa) + (ra if with_res else 0)
    y = torch.relu(pre) if relu else pre
    y.backward(torch.cat(gs))
    o = norm_ref.batch_norm_ranks(xs, ref.weight, ref.bias, 1e-3, ress=rs if with_res else None, relu=relu, dys=gs)
    lo = 0
    for i, n in enumerate(rows):
        assert o.y[i].shape == (n, c) and o.dx[i].shape == (n, c)
        assert _err(o.y[i], y.detach()[lo:lo + n]) < TOL and _err(o.dx[i], xa.grad[lo:lo + n]) < TOL
        if with_res:
            assert _err(o.dres[i], ra.grad[lo:lo + n]) < TOL
        lo += n
    assert _err(o.dgamma, ref.weight.grad) < TOL and _err(o.dbeta, ref.bias.grad) < TOL
    assert _err(sum(o.dgamma_local), o.dgamma) < TOL and _err(sum(o.dbeta_local), o.dbeta) < TOL
    assert _err(o.mean, ref.running_mean) < TOL and _err(o.var_unbiased, ref.running_var) < TOL  # momentum = 1
    assert _err(o.var, torch.cat(xs).var(0, unbiased=False)) < TOL


def test_shifted_stats_fp32_stays_under_the_outlier_bound():
    """The float32 evaluation of mean = x[0] + s1/m, var = s2/m - (s1/m)^2 on the inputs of the GPU outlier test: its
    relative variance error, in units of 2^-24 (1 + delta^2), was measured as norm_ref.OUTLIER_K / 4 at its largest; here it
    must stay under K / 2 (torch's order of summation may differ between CPUs), and the mean within float32 rounding of
    the shift."""
    for delta in norm_ref.OUTLIER_DELTAS:
        x = norm_ref.outlier_input(delta)
        xd = x.double()
        mean64 = xd.mean(0)
        var64 = xd.var(0, unbiased=False)
        mean32, var32 = norm_ref.shifted_stats_fp32(x)
        ratio = float(((var32.double() - var64).abs() / var64).max()) / (2.0 ** -24 * (1 + delta * delta))
        print(f"delta {delta}: relative variance error / (2^-24 (1 + delta^2)) = {ratio:.3f}")
        assert ratio <= norm_ref.OUTLIER_K / 2
        assert float(((mean32.double() - mean64).abs() / var64.sqrt()).max()) < 8 * 2.0 ** -24 * (3 + delta)
