"""Reference and derived error bounds for the one-channel submanifold conv and the fused SALayer gate
(include/seg3d_hip.h, csrc/sa_gate.hip), shared by tests/test_sa_gate_host.py and tests/test_gpu_sa_gate.py.

Site sets are small and built here; their neighbour table comes from oracle.sparse_conv.Sites.subm().  The float64
reference is oracle.sparse_conv.apply_rulebook with the [1, 3, 3, 3, C] weight, then sigmoid and product, gradients by
torch autograd in float64.

Bounds (u = 2^-24, the float32 unit round-off; never taken from an observed error).  A sum of n rounded products in ANY
order is within gamma(n) * sum |terms| of the exact sum, gamma(n) = n u / (1 - n u)  (n - 1 additions + 1 product rounding).
  s      gamma(T_i + 1) * (sum |x w| + |bias|),  T_i = C * (neighbours of row i)
  g      B_s / 4  (the sigmoid's slope is <= 1/4)  +  6 u g  (expf to 1 ulp = 2 u, 1 + e, the division, and e's own error
         through the quotient)  +  2^-148 (denormal results)
  y      |x| B_g + u |x g|
  dg     gamma(C) * sum |dy x|
  ds     B_dg g (1 - g)  +  |dg| B_g  (d[g (1 - g)] / dg = 1 - 2 g, |.| <= 1; the computed 1 - g carries g's absolute error)
         +  3 u |ds|  (two products and the subtraction)
  dx     |dy| B_g + u |dy g|  +  sum_k B_ds[n_k] |w|  +  gamma(K_j + 1) * (|dy g| + sum_k |ds w|),  K_j terms
  dw     sum_j B_ds[n_j] |x_j|  +  gamma(N + 1) * sum_j |ds x|,  N = rows with that neighbour
  dbias  sum B_ds + gamma(M) * sum |ds|
The plain conv has ds = dout exactly: B_ds = 0 there.  Every bound is multiplied by 1 + 1e-3 for the second-order terms
the first-order propagation drops (the largest n u here is 10368 * 2^-24 = 6e-4).
"""
import numpy as np
import torch

from oracle import sparse_conv as sc

U = 2.0 ** -24
ROWS = 128  # SEG3D_SUBM_DOT_ROWS
SLACK = 1.0 + 1e-3
CHANNELS = (4, 32, 48, 96, 192, 384)
ROW_COUNTS = (0, 1, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, 3 * ROWS + 5)


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------ site sets
def solid_sites(m, side=6):
    """The first m sites of a side x side x * block in raster order (m = side^3: a solid cube; interior rows have all 27
    neighbours, corners 8)."""
    i = np.arange(m)
    coords = np.stack([np.zeros(m, np.int64), i // (side * side), (i // side) % side, i % side], 1).astype(np.int32)
    return coords, [max(int(-(-m // (side * side))), 1) + 2, side + 2, side + 2], 1


def isolated_sites(m):
    """Sites two apart along x: every row has its centre only."""
    i = np.arange(m)
    coords = np.stack([np.zeros(m, np.int64), np.ones(m, np.int64), np.ones(m, np.int64), 2 * i], 1).astype(np.int32)
    return coords, [3, 3, 2 * max(m, 1) + 1], 1


def batch_sites(side=6):
    """Two samples: sample 0 fills z in [0, side / 2), sample 1 z in [side / 2, side) of the same side^3 cube -- the blocks
    touch in coordinates, never in batch index."""
    c, shape, _ = solid_sites(side ** 3, side)
    c = c.copy()
    c[:, 0] = (c[:, 1] >= side // 2).astype(np.int32)
    return c, shape, 2


def table(coords, shape):
    """The oracle's [27, M] table, with the centre and mirror properties asserted (the backward relies on them)."""
    m = coords.shape[0]
    if m == 0:
        return np.zeros((27, 0), np.int32)
    nbr = sc.Sites(coords, shape).subm()
    assert nbr.shape == (27, m) and nbr.dtype == np.int32
    assert np.array_equal(nbr[13], np.arange(m)), "centre property"
    for k in range(27):
        rows = np.flatnonzero(nbr[k] >= 0)
        assert np.array_equal(nbr[26 - k][nbr[k][rows]], rows), f"mirror property at offset {k}"
        assert np.all(coords[nbr[k][rows], 0] == coords[rows, 0]), "a neighbour crosses the batch boundary"
    return nbr


def make_case(m, c, sites="solid", seed=0, w_scale=None, bias=True, x_scale=1.0):
    rng = np.random.default_rng(seed * 7919 + 13 * m + c)
    coords, shape, bs = {"solid": solid_sites, "isolated": isolated_sites}[sites](m) if sites != "batch" else batch_sites()
    m = coords.shape[0]
    nbr = table(coords, shape)
    x = (rng.standard_normal((m, c)) * x_scale).astype(np.float32)
    ws = w_scale if w_scale is not None else 1.0 / np.sqrt(27 * c)
    w = (rng.standard_normal((1, 3, 3, 3, c)) * ws).astype(np.float32)
    b = (rng.standard_normal((1,)) * 0.1).astype(np.float32) if bias else None
    dy = rng.standard_normal((m, c)).astype(np.float32)
    dout = rng.standard_normal((m, 1)).astype(np.float32)
    return dict(m=m, c=c, coords=coords, shape=shape, bs=bs, nbr=nbr, x=x, w=w, b=b, dy=dy, dout=dout)


# ------------------------------------------------------------------------------------------------ float64 + bounds
def _t64(a, grad=True):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).requires_grad_(grad)


def _gather_abs(nbr, a, wabs):
    """[M] sum over the present neighbours and channels of |a[nbr]| |w[k]|, and the neighbour count."""
    m = nbr.shape[1]
    mag, cnt = np.zeros(m), np.zeros(m)
    for k in range(27):
        rows = np.flatnonzero(nbr[k] >= 0)
        mag[rows] += np.abs(a[nbr[k][rows]]) @ wabs[k]
        cnt[rows] += 1
    return mag, cnt


def reference(case, gate, bias=True):
    """float64 results and bounds: dict name -> (value, bound) for s, y (gate only), dx, dw, db (bias only)."""
    nbr, m, c = case["nbr"], case["m"], case["c"]
    use_b = bias and case["b"] is not None and not gate
    if m == 0:  # nothing to compute: empty results, zero weight gradients, all exact
        z = np.zeros
        res = {"s": (z(0), z(0)), "dx": (z((0, c)), z((0, c))), "dw": (z((27, c)), z((27, c)))}
        res.update({"y": (z((0, c)), z((0, c)))} if gate else {})
        res.update({"db": (z(1), z(1))} if use_b else {})
        return res
    x, w = _t64(case["x"]), _t64(case["w"])
    b = _t64(case["b"]) if use_b else None
    s = sc.apply_rulebook(x, nbr, w, b)
    wf = np.abs(case["w"].astype(np.float64)).reshape(27, c)
    xa = case["x"].astype(np.float64)
    mag_s, cnt = _gather_abs(nbr, xa, wf)
    b_s = gamma(c * cnt + 1) * (mag_s + (abs(float(case["b"][0])) if use_b else 0.0)) * SLACK
    res = {"s": (s.detach().numpy().reshape(m), b_s)}
    if gate:
        g = torch.sigmoid(s)
        y = x * g
        y.backward(_t64(case["dy"], False))
        gn = g.detach().numpy().reshape(m)
        b_g = (b_s / 4 + 6 * U * gn + 2.0 ** -148) * SLACK
        res["g"] = (gn, b_g)
        res["y"] = (y.detach().numpy(), (np.abs(xa) * b_g[:, None] + U * np.abs(xa * gn[:, None])) * SLACK)
        dy = case["dy"].astype(np.float64)
        dg = (dy * xa).sum(1)
        b_dg = gamma(c) * np.abs(dy * xa).sum(1)
        ds = dg * gn * (1 - gn)
        b_ds = (b_dg * gn * (1 - gn) + np.abs(dg) * b_g + 3 * U * np.abs(ds)) * SLACK
        res["ds"] = (ds, b_ds)
    else:
        s.backward(_t64(case["dout"], False))
        ds, b_ds = case["dout"].astype(np.float64).reshape(m), np.zeros(m)
        dy = gn = b_g = None
    # dx: row j gathers ds[nbr[k][j]] w[26 - k]
    wflip = wf[::-1]
    k_cnt = cnt  # terms of row j's sum = its neighbours
    dx_b = np.zeros((m, c))
    dx_mag = np.zeros((m, c))
    for k in range(27):
        rows = np.flatnonzero(nbr[k] >= 0)
        dx_b[rows] += b_ds[nbr[k][rows], None] * wflip[k][None, :]
        dx_mag[rows] += np.abs(ds[nbr[k][rows], None]) * wflip[k][None, :]
    if gate:
        own = np.abs(dy * gn[:, None])
        dx_b += np.abs(dy) * b_g[:, None] + U * own
        dx_mag += own
    res["dx"] = (x.grad.numpy(), (dx_b + gamma(k_cnt + 2)[:, None] * dx_mag) * SLACK)
    # dw[k] = sum_j ds[nbr[26 - k][j]] x_j
    dw_b = np.zeros((27, c))
    for k in range(27):
        rows = np.flatnonzero(nbr[26 - k] >= 0)
        src = nbr[26 - k][rows]
        dw_b[k] = (b_ds[src, None] * np.abs(xa[rows])).sum(0) + \
            gamma(rows.size + 1) * (np.abs(ds[src, None]) * np.abs(xa[rows])).sum(0)
    res["dw"] = (w.grad.numpy().reshape(27, c), dw_b * SLACK)
    if use_b:
        res["db"] = (b.grad.numpy().reshape(1), np.array([(b_ds.sum() + gamma(max(m, 1)) * np.abs(ds).sum()) * SLACK]))
    return res


def ratio(name, got, ref_bound):
    """max |got - ref| / bound (rows whose bound is 0 must match exactly); printed, returned."""
    ref, bound = ref_bound
    got = np.asarray(got, dtype=np.float64).reshape(np.shape(ref))
    assert np.all(np.isfinite(got)), f"{name}: non-finite values"
    err = np.abs(got - ref)
    zero = bound == 0
    assert np.all(err[zero] == 0), f"{name}: error where the bound is exactly 0"
    r = float((err[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.0
    print(f"{name}: max error / bound = {r:.3f}  (max error {float(err.max()) if err.size else 0.0:.3e})")
    return r


# ------------------------------------------------------------------------------------------------ the ops under test
def run_ops(case, gate, device, need_x=True, need_w=True, need_b=True, bias=True):
    """ops.sa_gate (gate) or ops.subm_dot on ``device`` ('cpu' = the host twins), forward and one backward ->
    dict of numpy arrays: s (the logits: the output of subm_dot, the saved tensor of sa_gate), y, dx, dw, db."""
    from openseg3d_amd import ops
    dev = torch.device(device)
    x = torch.from_numpy(case["x"]).to(dev).requires_grad_(need_x)
    w = torch.from_numpy(case["w"]).to(dev).requires_grad_(need_w)
    use_b = bias and case["b"] is not None and not gate
    b = torch.from_numpy(case["b"]).to(dev).requires_grad_(need_b) if use_b else None
    nbr = torch.from_numpy(case["nbr"]).to(dev)
    out = {}
    if gate:
        y = ops.sa_gate(x, w, nbr)
        out["y"] = y.detach().cpu().numpy()
        if y.grad_fn is not None:
            out["s"] = y.grad_fn.saved_tensors[3].cpu().numpy()
        seed = torch.from_numpy(case["dy"]).to(dev)
    else:
        y = ops.subm_dot(x, w, b, nbr)
        assert tuple(y.shape) == (case["m"], 1)
        out["s"] = y.detach().cpu().numpy().reshape(-1)
        seed = torch.from_numpy(case["dout"]).to(dev)
    if y.requires_grad:
        y.backward(seed)
    for name, t in (("dx", x), ("dw", w), ("db", b)):
        if t is not None and t.grad is not None:
            out[name] = t.grad.cpu().numpy().reshape(27, case["c"]) if name == "dw" else t.grad.cpu().numpy()
    return out


def check_all(tag, got, ref):
    """Every result present in ``got`` against its float64 value and bound; -> the largest ratio."""
    worst = 0.0
    for name in ("s", "y", "dx", "dw", "db"):
        if name in got and name in ref:
            r = ratio(f"{tag} {name}", got[name], ref[name])
            assert r <= 1.0, f"{tag} {name}: max error / bound = {r}"
            worst = max(worst, r)
    return worst


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def saturation_check(device):
    """Two touching half cubes with uniform-sign inputs in [1, 2) (sample 0 positive, sample 1 negative) times a uniform
    weight of 50: |s| >= 8 * 4 * 50 there; a third sample of isolated rows with inputs of 1e-3 keeps moderate logits in
    the same call.  On the saturated rows the gate is exactly 1 or 0 and ds exactly 0 (so dx = dy g exactly and they add
    nothing to dw); nothing is NaN anywhere.  (expf(-|s|) is exactly 0 from |s| >= 104 on: include/seg3d_hip.h.)"""
    from openseg3d_amd import ops
    c, n_iso = 4, 20
    cube, shape, _ = batch_sites()
    iso = np.stack([np.full(n_iso, 2), np.ones(n_iso, np.int64), np.ones(n_iso, np.int64), 2 * np.arange(n_iso)], 1)
    coords = np.concatenate([cube, iso.astype(np.int32)])
    nbr = table(coords, [shape[0], shape[1], 2 * n_iso + 1])
    m = coords.shape[0]
    rng = np.random.default_rng(5)
    x = (rng.random((m, c)) + 1.0).astype(np.float32)
    x[coords[:, 0] == 1] *= -1
    x[coords[:, 0] == 2] *= 1e-3
    w = np.full((1, 3, 3, 3, c), 50.0, np.float32)
    dy = rng.standard_normal((m, c)).astype(np.float32)
    s64 = sc.apply_rulebook(torch.from_numpy(x).double(), nbr, torch.from_numpy(w).double()).numpy().reshape(m)
    sat = np.abs(s64) > 100
    assert sat.sum() == 216 and np.all(np.abs(s64[sat]) >= 1600) and np.all(np.abs(s64[~sat]) < 1)
    dev = torch.device(device)
    xt = torch.from_numpy(x).to(dev).requires_grad_()
    wt = torch.from_numpy(w).to(dev).requires_grad_()
    y = ops.sa_gate(xt, wt, torch.from_numpy(nbr).to(dev))
    y.backward(torch.from_numpy(dy).to(dev))
    yv, dx, dw = y.detach().cpu().numpy(), xt.grad.cpu().numpy(), wt.grad.cpu().numpy().reshape(27, c)
    assert all(np.isfinite(t).all() for t in (yv, dx, dw))
    g = (s64[sat] > 0).astype(np.float32)[:, None]
    assert same_bits(yv[sat], x[sat] * g), "the gate is not exactly 0 or 1 on the saturated rows"
    assert same_bits(dx[sat], dy[sat] * g + np.float32(0)), "ds is not exactly 0 on the saturated rows"
    # only the isolated rows (centre offset only) reach the weight gradient
    assert np.all(dw[np.arange(27) != 13] == 0) and np.any(dw[13] != 0)
