"""rownorm.hip over the kernels' own layouts, against the float64 reference of tests/norm_ref.py.

tests/test_gpu_norms.py follows the widths of the model; the cases here follow the launch code instead:
  * BatchNorm column passes: a 256-thread block is quads = c/4 column groups x lanes = 256/quads row lanes -- one lane
    (c > 512), 256 lanes (c = 4), idle threads (256 % quads != 0), one block more or less than full, the grid capped at 1024
    blocks, the four-chain loop of the block sums at its full length;
  * LayerNorm: p = 8, 16, 32, 64 lanes per row, one and two quads per lane, rows past the forward cap (2048 blocks x 4 waves)
    and the backward cap (1024 blocks x 16 row batches), where the grid-stride loops run;
  * the SyncBatchNorm halves (seg3d_colstats_about, seg3d_batchnorm_bwd_reduce, seg3d_batchnorm_bwd_apply) with the ranks
    simulated by row blocks in one process, and with three real ranks (tests/_syncbn_cases_rank.py);
  * seg3d_colstats and seg3d_batchnorm_stats with row 0 an outlier of its column: the shift of the statistics.
Tolerances are those of tests/test_gpu_norms.py and tests/_syncbn_rank.py.  Every figure is printed before it is asserted."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import norm_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BN_EPS, BN_MOMENTUM = 1e-3, 0.01


class _Checks:
    """Collects (name, error, bound), prints each, and fails at the end with all that missed: one run shows every figure."""

    def __init__(self):
        self.bad = []

    def close(self, name, got, ref, tol, rel=False):
        got = got.detach().cpu().double()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err = float((got - ref).abs().max()) if ref.numel() else 0.0
        bound = tol * max(1.0, float(ref.abs().max()) if ref.numel() else 0.0) if rel else tol
        print(f"  {name}: err {err:.3e} bound {bound:.3e}")
        if not err < bound:  # (a NaN misses too)
            self.bad.append((name, err, bound))

    def done(self):
        assert not self.bad, self.bad


def _move_off_the_kink(tensors, pre_of):
    """Nudge the float32 inputs until every float64 pre-activation is at least 2e-3 from zero: the fp32 statistics differ
    from the reference's by rounding, and an element within rounding of zero may take the other ReLU branch."""
    for _ in range(10):
        pres = pre_of()
        if not any(bool((p.abs() < 2e-3).any()) for p in pres):
            return
        for t, p in zip(tensors, pres):
            t[p.abs() < 2e-3] += 0.05


# ------------------------------------------------------------------------------------------ BatchNorm, ops.batch_norm_act
def _bn_case(m, c, relu, with_res, seed_salt=0):
    gen = torch.Generator().manual_seed(m * 3 + c + seed_salt)
    x = torch.randn(m, c, generator=gen) * 1.5 + 3.0  # O(1), non-zero column mean
    r = torch.randn(m, c, generator=gen) if with_res else None
    g = torch.randn(m, c, generator=gen)
    gamma = (1 + 0.2 * torch.randn(c, generator=gen)).clamp_(min=0.3)
    beta = 0.1 * torch.randn(c, generator=gen)
    rm, rv = torch.randn(c, generator=gen), 0.5 + torch.rand(c, generator=gen)
    if relu and m > 1:
        _move_off_the_kink([x], lambda: [norm_ref.batch_norm(x, gamma, beta, BN_EPS, res=r).pre])
    return x, r, g, gamma, beta, rm, rv


def _bn_module(c, gamma, beta, rm, rv, momentum=BN_MOMENTUM, cls=nn.BatchNorm1d):
    bn = cls(c, eps=BN_EPS, momentum=momentum)
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    return bn.to(DEV)


def _check_batch_norm(m, c, relu, with_res, fused):
    from openseg3d_amd import ops
    x, r, g, gamma, beta, rm, rv = _bn_case(m, c, relu, with_res)
    ref = norm_ref.batch_norm(x, gamma, beta, BN_EPS, res=r, relu=relu, dy=g, running_mean=rm, running_var=rv,
                              momentum=BN_MOMENTUM)
    if relu:
        assert float(ref.pre.abs().min()) > 1e-3
    bn = _bn_module(c, gamma, beta, rm, rv).train()
    xg = x.to(DEV).requires_grad_()
    rg = r.to(DEV).requires_grad_() if with_res else None
    y = ops.batch_norm_act(xg, bn, relu=relu, res=rg)
    assert type(y.grad_fn).__name__.startswith("_BatchNormActFn") == fused, type(y.grad_fn).__name__
    y.backward(g.to(DEV))
    ck = _Checks()
    ck.close("y", y, ref.y, 5e-5)
    ck.close("dx", xg.grad, ref.dx, 5e-5)
    if with_res:
        ck.close("dres", rg.grad, ref.dres, 1e-6)
    ck.close("dgamma", bn.weight.grad, ref.dgamma, 1e-3, rel=True)
    ck.close("dbeta", bn.bias.grad, ref.dbeta, 1e-3, rel=True)
    ck.close("running_mean", bn.running_mean, ref.running_mean, 1e-5)
    ck.close("running_var", bn.running_var, ref.running_var, 1e-4)
    assert int(bn.num_batches_tracked) == ref.num_batches_tracked == 1
    # eval: the running statistics, folded into one affine pass
    with torch.no_grad():
        ye = ops.batch_norm_act(x.to(DEV), bn.eval(), relu=relu, res=None if r is None else r.to(DEV))
    refe = norm_ref.batch_norm(x, gamma, beta, BN_EPS, res=r, relu=relu, running_mean=ref.running_mean,
                               running_var=ref.running_var, training=False)
    ck.close("y eval", ye, refe.y, 5e-5)
    ck.done()


BN_SHAPES = [
    (300, 4),       # lanes = 256
    (301, 20),      # 51 lanes, one idle thread
    (1000, 100),    # 10 lanes, six idle threads
    (2049, 128), (700, 384),  # model widths
    (16401, 516),   # lanes = 1, 127 idle threads, 1024 blocks (the cap), 17 of them take a second row
    (2050, 1024),   # the widest accepted
    (3, 64),
    (255, 64), (257, 64),  # 16 lanes x 16 rows: one block covers 256 rows
]


@pytest.mark.parametrize("m,c", BN_SHAPES)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
def test_batchnorm_act_over_the_column_layouts(m, c, relu, with_res):
    _check_batch_norm(m, c, relu, with_res, fused=True)


@pytest.mark.parametrize("relu,with_res", [(True, True), (True, False), (False, False)])
def test_batchnorm_act_capped_grid_is_bit_reproducible(relu, with_res):
    """(16401, 516), 1024 blocks summed by the four-chain loop at full length: the sums are fixed-order, so two runs give
    the same bits (ReLU without a residual runs col_reduce_pre_kernel, the others col_reduce_kernel<1>)."""
    from openseg3d_amd import ops
    m, c = 16401, 516
    x, r, g, gamma, beta, rm, rv = _bn_case(m, c, False, with_res)
    runs = []
    for _ in range(2):
        bn = _bn_module(c, gamma, beta, rm, rv).train()
        xg = x.to(DEV).requires_grad_()
        y = ops.batch_norm_act(xg, bn, relu=relu, res=None if r is None else r.to(DEV))
        assert type(y.grad_fn).__name__.startswith("_BatchNormActFn")
        y.backward(g.to(DEV))
        runs.append((y.detach(), xg.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
def test_batchnorm_act_wider_than_1024_falls_back_to_torch(relu, with_res):
    _check_batch_norm(300, 1028, relu, with_res, fused=False)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
def test_batchnorm_act_single_row_falls_back_to_torch(relu, with_res):
    """(1, 64): the batch statistics of one row do not exist -- training raises as torch's BatchNorm1d does, eval runs
    torch's module and matches float64."""
    from openseg3d_amd import ops
    x, r, g, gamma, beta, rm, rv = _bn_case(1, 64, relu, with_res)
    bn = _bn_module(64, gamma, beta, rm, rv)
    rg = None if r is None else r.to(DEV)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.batch_norm_act(x.to(DEV).requires_grad_(), bn.train(), relu=relu, res=rg)
    with torch.no_grad():
        ye = ops.batch_norm_act(x.to(DEV), bn.eval(), relu=relu, res=rg)
    refe = norm_ref.batch_norm(x, gamma, beta, BN_EPS, res=r, relu=relu, running_mean=rm, running_var=rv, training=False)
    ck = _Checks()
    ck.close("y eval", ye, refe.y, 5e-5)
    ck.close("running_mean", bn.running_mean, rm.double(), 1e-12)  # untouched
    ck.done()


# ------------------------------------------------------------------------------------------ LayerNorm, ops.layer_norm_residual
def _ln_case(m, c, with_res, with_scale):
    gen = torch.Generator().manual_seed(m + c)
    x = torch.randn(m, c, generator=gen) * 2 + 0.5
    r = torch.randn(m, c, generator=gen) if with_res else None
    g = torch.randn(m, c, generator=gen)
    scale = (torch.rand(m, generator=gen) < 0.8).float() / 0.8 if with_scale else None  # 0 or 1 / 0.8
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=gen), 0.1 * torch.randn(c, generator=gen)
    return x, r, g, scale, gamma, beta


def _check_layer_norm(m, c, with_res, with_scale, fused):
    from openseg3d_amd import ops
    x, r, g, scale, gamma, beta = _ln_case(m, c, with_res, with_scale)
    ln = nn.LayerNorm(c)
    with torch.no_grad():
        ln.weight.copy_(gamma), ln.bias.copy_(beta)
    ln = ln.to(DEV)
    ref = norm_ref.layer_norm(x, gamma, beta, ln.eps, res=r, rowscale=scale, dy=g)
    xg = x.to(DEV).requires_grad_()
    rg = r.to(DEV).requires_grad_() if with_res else None
    y = ops.layer_norm_residual(xg, rg, ln, rowscale=None if scale is None else scale.to(DEV))
    assert type(y.grad_fn).__name__.startswith("_LayerNormResidualFn") == fused, type(y.grad_fn).__name__
    y.backward(g.to(DEV))
    ck = _Checks()
    ck.close("y", y, ref.y, 2e-5)
    ck.close("dx", xg.grad, ref.dx, 2e-5)
    if with_res:
        ck.close("dres", rg.grad, ref.dres, 1e-6)
    ck.close("dgamma", ln.weight.grad, ref.dgamma, 1e-3, rel=True)
    ck.close("dbeta", ln.bias.grad, ref.dbeta, 1e-3, rel=True)
    ck.done()


LN_SHAPES = [
    (33, 4), (1000, 28), (131101, 8),            # p = 8; the last past both caps (65536 / 131072 rows)
    (129, 36), (500, 64),                        # p = 16
    (65, 68), (777, 128),                        # p = 32
    (300, 132), (1000, 256),                     # p = 64, one quad per lane
    (1000, 260), (16401, 384), (16401, 512),     # two quads per lane; 16401 rows pass the caps of 8192 / 16384 rows
    (1, 96),
]


@pytest.mark.parametrize("m,c", LN_SHAPES)
@pytest.mark.parametrize("with_res", [True, False])
def test_layernorm_residual_over_the_row_layouts(m, c, with_res):
    _check_layer_norm(m, c, with_res, False, fused=True)


@pytest.mark.parametrize("m,c", [(16401, 384), (1000, 260)])
@pytest.mark.parametrize("with_res", [True, False])
def test_layernorm_residual_row_scale_in_the_two_item_form(m, c, with_res):
    _check_layer_norm(m, c, with_res, True, fused=True)


@pytest.mark.parametrize("with_res", [True, False])
def test_layernorm_residual_wider_than_512_falls_back_to_torch(with_res):
    _check_layer_norm(300, 516, with_res, True, fused=False)


def test_layernorm_bwd_partials_entry_matches_the_one_call_backward():
    """seg3d_layernorm_bwd_partials + seg3d_reduce_partials (what an encoder layer's backward queues on its fork) at
    (16401, 384): dx bit for bit seg3d_layernorm_bwd's, dgamma / dbeta -- summed by another kernel in another order --
    within the tolerance of float64."""
    from openseg3d_amd import _lib
    from openseg3d_amd.ops import _ptr, _stream
    m, c = 16401, 384
    x, _, g, scale, gamma, beta = _ln_case(m, c, False, True)
    ref = norm_ref.layer_norm(x, gamma, beta, 1e-5, rowscale=scale, dy=g)
    x, g, scale, gamma, beta = (t.to(DEV) for t in (x, g, scale, gamma, beta))
    f32 = dict(dtype=torch.float32, device=DEV)
    y, mean, rstd = torch.empty_like(x), torch.empty(m, **f32), torch.empty(m, **f32)
    _lib.call("seg3d_layernorm_fwd", _ptr(x), None, _ptr(gamma), _ptr(beta), _ptr(scale), 1e-5, m, c, _ptr(y), _ptr(mean),
              _ptr(rstd), _stream())
    ws_bytes = _lib.query("seg3d_layernorm_bwd_workspace_bytes", m, c)
    assert ws_bytes == 1024 * 2 * c * 4
    out = []
    for entry in ("seg3d_layernorm_bwd", "seg3d_layernorm_bwd_partials"):
        ws = torch.full((ws_bytes // 4,), float("nan"), **f32)
        dx, dg, db = torch.full_like(x, float("nan")), torch.full((c,), float("nan"), **f32), torch.full((c,), float("nan"), **f32)
        if entry == "seg3d_layernorm_bwd":
            _lib.call(entry, _ptr(g), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(scale), m, c, _ptr(dx), _ptr(dg),
                      _ptr(db), _ptr(ws), ws_bytes, _stream())
        else:
            nb = ctypes.c_int32(0)
            _lib.call(entry, _ptr(g), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(scale), m, c, _ptr(dx), _ptr(ws),
                      ws_bytes, ctypes.byref(nb), _stream())
            assert nb.value == 1024  # ceil(16401 / 16) = 1026 row batches of a block, capped
            _lib.call("seg3d_reduce_partials", _ptr(ws), nb.value, 2 * c, c, _ptr(dg), _ptr(db), _stream())
        out.append((dx, dg, db))
    assert torch.equal(out[0][0], out[1][0])
    ck = _Checks()
    ck.close("y", y, ref.y, 2e-5)
    ck.close("mean", mean, ref.mean, 2e-5)
    ck.close("dx", out[1][0], ref.dx, 2e-5)
    for name, (_, dg, db) in zip(("one call", "partials"), out):
        ck.close(f"dgamma {name}", dg, ref.dgamma, 1e-3, rel=True)
        ck.close(f"dbeta {name}", db, ref.dbeta, 1e-3, rel=True)
    ck.done()


# ------------------------------------------------------------------------------------------ SyncBatchNorm halves, one process
def _sync_case(rows, c, relu, with_res, seed):
    """Row blocks that differ in mean and scale, as the ranks of tests/_syncbn_rank.py do."""
    gen = torch.Generator().manual_seed(seed)
    xs = [torch.randn(n, c, generator=gen) * (1.0 + 0.5 * i) + 0.3 * i for i, n in enumerate(rows)]
    rs = [torch.randn(n, c, generator=gen) for n in rows] if with_res else None
    gs = [torch.randn(n, c, generator=gen) for n in rows]
    gamma, beta = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen)
    if relu:
        _move_off_the_kink(xs, lambda: norm_ref.batch_norm_ranks(xs, gamma, beta, BN_EPS, ress=rs).pre)
    return xs, rs, gs, gamma, beta


def _sync_halves(xs, rs, gs, gamma, beta, relu):
    """The steps of ops._sync_batch_norm_act / _SyncBatchNormActFn with the exchange between ranks replaced by a stack and a
    float32 sum in block order.  Returns per-block y, dx, dres, sums and the merged mean, biased and unbiased variance."""
    from openseg3d_amd import _lib, ops
    from openseg3d_amd.ops import _ptr, _stream, _workspace
    c = gamma.numel()
    f32 = dict(dtype=torch.float32, device=DEV)

    def ws_for(m):
        nbytes = _lib.query("seg3d_batchnorm_workspace_bytes", m, c)
        return _workspace(nbytes, torch.device(DEV)), nbytes

    # (mean, M2, count) per block by the function _sync_batch_norm_act itself uses: seg3d_colstats_about the mean of the
    # block's first rows; a block without rows contributes zeros
    allg = torch.stack([ops._local_moments(x) for x in xs]).double()
    assert allg.shape == (len(xs), 2 * c + 1) and [int(n) for n in allg[:, 2 * c]] == [x.shape[0] for x in xs]
    mean, m2, total = (t.float() for t in ops.combine_moments(allg[:, :c], allg[:, c:2 * c], allg[:, 2 * c:]))
    var = (m2 / total).clamp_(min=0.0)
    rstd = torch.rsqrt(var + BN_EPS)
    scale = (gamma * rstd).contiguous()
    shift = (beta - mean * scale).contiguous()
    unbiased = m2 / (total - 1).clamp_(min=1.0)
    inv_count = (1.0 / total).to(torch.float32).contiguous()
    mean, rstd = mean.contiguous(), rstd.contiguous()

    ys, block_sums = [], []
    for i, x in enumerate(xs):
        m = x.shape[0]
        y = torch.empty_like(x)
        if m > 0:
            _lib.call("seg3d_affine_act", _ptr(x), _ptr(rs[i]) if rs is not None else None, _ptr(scale), _ptr(shift), int(relu),
                      m, c, _ptr(y), _stream())
        ys.append(y)
    for x, y, g in zip(xs, ys, gs):
        m = x.shape[0]
        sums = torch.zeros((2, c), **f32)
        if m > 0:
            sums.fill_(float("nan"))
            ws, nbytes = ws_for(m)
            _lib.call("seg3d_batchnorm_bwd_reduce", _ptr(g), _ptr(y), _ptr(x), _ptr(mean), _ptr(rstd), int(relu), m, c,
                      _ptr(sums), _ptr(ws), nbytes, _stream())
        block_sums.append(sums)
    tot = torch.zeros((2, c), **f32)
    for s in block_sums:
        tot = tot + s
    dxs, dress = [], []
    for x, y, g in zip(xs, ys, gs):
        m = x.shape[0]
        dx = torch.full_like(x, float("nan"))
        dres = torch.full_like(x, float("nan")) if rs is not None else None
        if m > 0:
            _lib.call("seg3d_batchnorm_bwd_apply", _ptr(g), _ptr(y), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(tot),
                      _ptr(inv_count), int(relu), m, c, _ptr(dx), _ptr(dres), _stream())
        dxs.append(dx), dress.append(dres)
    return ys, dxs, dress, block_sums, tot, mean, var, unbiased


@pytest.mark.parametrize("rows", [[1, 37, 300, 4099], [2, 0, 16401]], ids=["1-37-300-4099", "2-0-16401"])
@pytest.mark.parametrize("c", [4, 48, 64, 256, 516])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
def test_sync_batchnorm_halves_with_row_blocks_as_ranks(rows, c, relu, with_res):
    xs, rs, gs, gamma, beta = _sync_case(rows, c, relu, with_res, seed=sum(rows) + c)
    ref = norm_ref.batch_norm_ranks(xs, gamma, beta, BN_EPS, ress=rs, relu=relu, dys=gs)
    if relu:
        assert min(float(p.abs().min()) for p in ref.pre if p.numel()) > 1e-3

    def dev(ts):
        return None if ts is None else [t.to(DEV) for t in ts]

    ys, dxs, dress, block_sums, tot, mean, var, unbiased = _sync_halves(dev(xs), dev(rs), dev(gs), gamma.to(DEV), beta.to(DEV),
                                                                        relu)
    ck = _Checks()
    for i in range(len(rows)):
        ck.close(f"y[{i}]", ys[i], ref.y[i], 1e-5, rel=True)
        ck.close(f"dx[{i}]", dxs[i], ref.dx[i], 1e-5, rel=True)
        if with_res:
            ck.close(f"dres[{i}]", dress[i], ref.dres[i], 1e-6, rel=True)
        ck.close(f"dbeta local[{i}]", block_sums[i][0], ref.dbeta_local[i], 1e-5, rel=True)
        ck.close(f"dgamma local[{i}]", block_sums[i][1], ref.dgamma_local[i], 1e-5, rel=True)
    ck.close("dbeta", tot[0], ref.dbeta, 1e-5, rel=True)
    ck.close("dgamma", tot[1], ref.dgamma, 1e-5, rel=True)
    ck.close("mean", mean, ref.mean, 1e-6, rel=True)
    ck.close("var", var, ref.var, 1e-6, rel=True)
    ck.close("var unbiased", unbiased, ref.var_unbiased, 1e-6, rel=True)
    ck.done()


@pytest.mark.parametrize("rows", [[1, 37, 300, 4099], [2, 16401]], ids=["1-37-300-4099", "2-16401"])
@pytest.mark.parametrize("c", [4, 48, 64, 256, 516])
def test_colstats_about_row0_over_the_column_layouts(rows, c):
    """seg3d_colstats itself (sums about row 0; ops.span_mean's entry) on the blocks of the case above.  Mean and variance
    are formed from its float32 sums in float64, so only the kernel's summation is measured, and held to the outlier bound
    per column: with delta = (x[0] - mean) / sigma of that column, the variance within OUTLIER_K 2^-24 (1 + delta^2) of
    itself, the mean within OUTLIER_K 2^-24 (1 + |delta|) sigma."""
    from openseg3d_amd import _lib
    from openseg3d_amd.ops import _ptr, _stream, _workspace
    xs = _sync_case(rows, c, False, False, seed=sum(rows) + c)[0]
    worst = []
    for x in xs:
        m = x.shape[0]
        xd = x.double()
        mean64, var64 = xd.mean(0), xd.var(0, unbiased=False)
        xg = x.to(DEV)
        sums = torch.full((2, c), float("nan"), dtype=torch.float32, device=DEV)
        nbytes = _lib.query("seg3d_batchnorm_workspace_bytes", m, c)
        ws = _workspace(nbytes, torch.device(DEV))
        _lib.call("seg3d_colstats", _ptr(xg), m, c, _ptr(sums), _ptr(ws), nbytes, _stream())
        s = sums.cpu().double()
        d = s[0] / m
        mean, var = xd[0] + d, s[1] / m - d * d
        u = norm_ref.OUTLIER_K * 2.0 ** -24
        sigma = var64.sqrt()
        delta = (xd[0] - mean64).abs() / sigma.clamp(min=1e-30)
        var_bound = u * (1 + delta * delta) * var64
        mean_bound = u * (1 + delta) * sigma
        worst.append((m, float(((var - var64).abs() - var_bound).max()), float(((mean - mean64).abs() - mean_bound).max()),
                      float(delta.max())))
        print(f"  rows {m}: variance error - bound {worst[-1][1]:.3e}, mean error - bound {worst[-1][2]:.3e}, "
              f"largest delta {worst[-1][3]:.2f}")
    assert all(v <= 0 and mu <= 0 for _, v, mu, _ in worst), worst


def test_sync_batchnorm_cases_on_three_ranks():
    """ops.batch_norm_act on a SyncBatchNorm in a three-rank gloo group sharing cuda:0 (tests/_syncbn_cases_rank.py): a rank
    without rows and one with a single row, two widths, ReLU and residual on and off, momentum=None over two passes."""
    drv = ("import sys; sys.path.insert(0, %r); from openseg3d_amd import dist as D; "
           "sys.exit(D.launch_local_ranks([sys.executable, %r], 3))" % (ROOT, os.path.join(ROOT, "tests", "_syncbn_cases_rank.py")))
    out = subprocess.run([sys.executable, "-c", drv], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    print(out.stdout[-3000:])
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    assert "SYNCBN CASES OK" in out.stdout


# ------------------------------------------------------------------------------------------ row 0 as an outlier
@pytest.mark.parametrize("delta", norm_ref.OUTLIER_DELTAS)
def test_batchnorm_statistics_with_row0_an_outlier(delta):
    """The statistics are sums of x - x[0]; with row 0 at mean + delta * sigma of its column the variance s2/m - d^2 cancels
    1 + delta^2 to 1.  Bound: OUTLIER_K * 2^-24 * (1 + delta^2) relative to float64 (norm_ref.OUTLIER_K: four times what the
    float32 evaluation of the formula measures on the CPU), and on y of the other rows what follows from it,
    |y| * (that bound) / 2 + 5e-5 (beta = 0, so y is proportional to rstd).  The batch variance is read back from
    running_var with momentum = 1."""
    from openseg3d_amd import ops
    m, c = 20000, 64
    x = norm_ref.outlier_input(delta, m, c)
    gen = torch.Generator().manual_seed(5)
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=gen), torch.zeros(c)
    ref = norm_ref.batch_norm(x, gamma, beta, BN_EPS, running_mean=torch.zeros(c), running_var=torch.ones(c), momentum=1.0)
    sigma = ref.var.sqrt()
    got_delta = (x[0].double() - ref.mean) / sigma
    assert float((got_delta - delta).abs().max()) < 1e-3 * max(delta, 1)
    bn = _bn_module(c, gamma, beta, torch.zeros(c), torch.ones(c), momentum=1.0).train()
    with torch.no_grad():
        y = ops.batch_norm_act(x.to(DEV), bn, relu=False)
    var_gpu = bn.running_var.cpu().double() * (m - 1) / m
    rel = float(((var_gpu - ref.var).abs() / ref.var).max())
    bound = norm_ref.OUTLIER_K * 2.0 ** -24 * (1 + delta * delta)
    mean_err = float(((bn.running_mean.cpu().double() - ref.mean).abs() / sigma).max())
    y_err = (y.cpu().double() - ref.y).abs()[1:]
    y_bound = ref.y.abs()[1:] * bound / 2 + 5e-5
    worst = float((y_err / y_bound).max())
    print(f"  delta {delta}: relative variance error {rel:.3e} = {rel / bound * norm_ref.OUTLIER_K:.2f} x 2^-24 (1 + delta^2), "
          f"bound {bound:.3e}; mean error {mean_err:.3e} sigma; y error {float(y_err.max()):.3e}, worst error / bound {worst:.3f}")
    assert rel <= bound
    assert worst <= 1.0
