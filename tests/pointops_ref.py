"""Restatements of query_and_group / interpolation (seg3d/utils/pointops_utils.py:25-61) for the tests, written from the
semantics in include/seg3d_hip.h:

  * float32 "as written": every operation rounded to float32, sums left to right (backward: per source row over its pairs
    in ascending pair index, lists longer than CHUNK entries cut into chunks that are summed on their own and added in
    chunk order) -- the host and device entries must return these bits;
  * float64 (numpy for the forward, torch autograd for the backward), taking the float32 dist as given -- the reference
    for the derived error bounds, with u = 2^-24.

An index outside [0, n) is a slot of zeros (grouping) or a slot that adds nothing but stays in the norm (interpolation).
"""
import numpy as np
import torch

U = 2.0 ** -24
CHUNK = 512  # SEG3D_POINTOPS_CHUNK
F32 = np.float32
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def inside(idx, n):
    return (idx >= 0) & (idx < n)


# ------------------------------------------------------------------------------------------------ float32, as written
def group_f32(xyz, new_xyz, feat, idx, use_xyz=True):
    n = feat.shape[0]
    ok = inside(idx, n)
    j = np.where(ok, idx, 0).astype(np.int64)
    parts = []
    if use_xyz:
        parts.append((xyz[j] - new_xyz[:, None, :]).astype(F32))  # float32 operands: one rounded subtraction
    parts.append(feat[j])
    out = np.concatenate(parts, axis=-1) if n else np.zeros(idx.shape + ((3 if use_xyz else 0) + feat.shape[1],), F32)
    out[~ok] = 0
    return out


def interp_weights_f32(dist):
    rcp = (F32(1.0) / (dist + F32(1e-8))).astype(F32)
    norm = rcp[:, 0].copy()
    for i in range(1, dist.shape[1]):
        norm = (norm + rcp[:, i]).astype(F32)
    return (rcp / norm[:, None]).astype(F32)


def interp_f32(feat, idx, dist):
    n, c = feat.shape
    w = interp_weights_f32(dist)
    out = np.zeros((idx.shape[0], c), F32)
    for i in range(idx.shape[1]):
        ok = inside(idx[:, i], n)
        j = np.where(ok, idx[:, i], 0).astype(np.int64)
        term = (feat[j] * w[:, i:i + 1]).astype(F32) if n else np.zeros_like(out)
        out = np.where(ok[:, None], (out + term).astype(F32), out)
    return out, w


def scatter_f32(terms, idx, n):
    """terms float32 [pairs, width] -> [n, width]: row j = the sum of the terms of the pairs with idx = j in the contract's
    order."""
    flat = idx.reshape(-1)
    out = np.zeros((n, terms.shape[1]), F32)
    pairs = np.flatnonzero(inside(flat, n))
    pairs = pairs[np.argsort(flat[pairs], kind="stable")]
    bounds = np.concatenate([[0], np.cumsum(np.bincount(flat[pairs], minlength=n))])
    for j in range(n):
        lst = pairs[bounds[j]:bounds[j + 1]]
        total = None
        for s in range(0, max(len(lst), 1), CHUNK):
            acc = np.zeros((terms.shape[1],), F32)
            for p in lst[s:s + CHUNK]:
                acc = (acc + terms[p]).astype(F32)
            total = acc if total is None else (total + acc).astype(F32)
        out[j] = total
    return out


def group_bwd_f32(dout, idx, n, use_xyz=True):
    """-> (dxyz, dnew_xyz, dfeat) as written (dxyz / dnew_xyz None without use_xyz)."""
    m, k, w = dout.shape
    rows = scatter_f32(dout.reshape(m * k, w), idx, n)
    if not use_xyz:
        return None, None, rows
    acc = np.zeros((m, 3), F32)
    for i in range(k):
        ok = inside(idx[:, i], n)
        acc = np.where(ok[:, None], (acc + dout[:, i, :3]).astype(F32), acc)
    return rows[:, :3].copy(), -acc, rows[:, 3:].copy()


def interp_bwd_f32(dout, w, idx, n):
    m, k = idx.shape
    terms = (dout[:, None, :] * w[:, :, None]).astype(F32).reshape(m * k, -1)
    return scatter_f32(terms, idx, n)


# ------------------------------------------------------------------------------------------------ float64
def interp_f64(feat, idx, dist):
    """-> (out, bound): bound = (2K + 4) u sum_i w_i |feat[idx_i]| per element."""
    n, c = feat.shape
    k = idx.shape[1]
    ok = inside(idx, n)
    j = np.where(ok, idx, 0).astype(np.int64)
    rcp = 1.0 / (dist.astype(np.float64) + 1e-8)
    w = rcp / rcp.sum(1, keepdims=True)
    g = feat.astype(np.float64)[j] * ok[..., None] if n else np.zeros(idx.shape + (c,))
    out = (g * w[..., None]).sum(1)
    bound = (2 * k + 4) * U * (np.abs(g) * w[..., None]).sum(1)
    return out, bound


def _t64(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).requires_grad_(grad)


def group_bwd_f64(xyz, new_xyz, feat, idx, dout, use_xyz=True):
    """float64 torch autograd of the restatement -> dict of gradients and of their bounds ((L_j - 1) u sum |terms| for
    dxyz / dfeat, (K - 1) u sum |terms| for dnew_xyz)."""
    n, c = feat.shape
    m, k = idx.shape
    ok = torch.from_numpy(inside(idx, n))
    j = torch.from_numpy(np.where(inside(idx, n), idx, 0).astype(np.int64))
    x, q, f = _t64(xyz, True), _t64(new_xyz, True), _t64(feat, True)
    parts = ([(x[j] - q[:, None, :]) * ok[..., None]] if use_xyz else []) + [f[j] * ok[..., None]]
    out = torch.cat(parts, -1)
    out.backward(_t64(dout))
    flat = idx.reshape(-1)
    keep = inside(flat, n)
    length = np.bincount(flat[keep], minlength=n)
    mag = np.zeros((n, dout.shape[2]))
    np.add.at(mag, flat[keep], np.abs(dout.reshape(m * k, -1).astype(np.float64))[keep])
    lim = np.maximum(length - 1, 0)[:, None] * U * mag
    res = {"dfeat": f.grad.numpy(), "dfeat_bound": lim[:, (3 if use_xyz else 0):]}
    if use_xyz:
        qmag = (np.abs(dout[:, :, :3].astype(np.float64)) * inside(idx, n)[..., None]).sum(1)
        res.update(dxyz=x.grad.numpy(), dxyz_bound=lim[:, :3], dnew_xyz=q.grad.numpy(), dnew_xyz_bound=(k - 1) * U * qmag)
    return res


def interp_bwd_f64(feat, idx, dist, dout):
    """-> (dfeat, bound): bound = (L_j + K + 3) u sum |w dout| over row j's list."""
    n, c = feat.shape
    m, k = idx.shape
    okn = inside(idx, n)
    ok = torch.from_numpy(okn)
    j = torch.from_numpy(np.where(okn, idx, 0).astype(np.int64))
    f = _t64(feat, True)
    rcp = 1.0 / (_t64(dist) + 1e-8)
    w = rcp / rcp.sum(1, keepdim=True)
    out = ((f[j] * ok[..., None]) * w[..., None]).sum(1)
    out.backward(_t64(dout))
    flat = idx.reshape(-1)
    keep = inside(flat, n)
    length = np.bincount(flat[keep], minlength=n)
    terms = np.abs(dout.astype(np.float64))[:, None, :] * w.numpy()[:, :, None]
    mag = np.zeros((n, c))
    np.add.at(mag, flat[keep], terms.reshape(m * k, c)[keep])
    return f.grad.numpy(), (length + k + 3)[:, None] * U * mag


# ------------------------------------------------------------------------------------------------ cases
def make_case(n, m, k, c, seed=0, scale=1.0, outside=False, hub=None, n_read=None):
    """Random clouds and a neighbour table.  outside: -1, n, INT32_MAX and INT32_MIN scattered into idx; hub: that source
    row is every query's first neighbour; n_read: only rows below it are listed (the others are read by nobody).
    dist holds exact zeros and the 1e5 of seg3d_knn_query's slots beyond a short segment."""
    rng = np.random.default_rng(seed)
    xyz = (rng.standard_normal((n, 3)) * 20).astype(F32)
    new_xyz = (rng.standard_normal((m, 3)) * 20).astype(F32)
    feat = (rng.standard_normal((n, c)) * scale).astype(F32)
    idx = rng.integers(0, max(n_read or n, 1), (m, k)).astype(np.int32)
    if hub is not None:
        idx[:, 0] = hub
    if outside and m * k:
        flat = idx.reshape(-1)
        where = rng.choice(m * k, size=max(1, (m * k) // 7), replace=False)
        flat[where] = np.resize(np.array([-1, n, INT32_MAX, INT32_MIN, n + 5, -7], np.int64), where.size).astype(np.int32)
    dist = np.sqrt(rng.random((m, k)) * 9).astype(F32)
    dist[rng.random((m, k)) < 0.05] = 0
    dist[rng.random((m, k)) < 0.05] = 1e5
    dout_g = rng.standard_normal((m, k, 3 + c)).astype(F32)
    dout_i = rng.standard_normal((m, c)).astype(F32)
    return dict(n=n, m=m, k=k, c=c, xyz=xyz, new_xyz=new_xyz, feat=feat, idx=idx, dist=dist, dout_g=dout_g, dout_i=dout_i)


# every value of c in {1, 3, 4, 6, 32, 33, 64, 67, 256}, K in {1, 3, 16, 17, 64}, m in {1, 63, 64, 65, 1000} and n in
# {1, 64, 500} at least once: both alignment paths, rows shorter and longer than a wave-instruction, tails, one and many
# workgroups; n = 1 with m K > CHUNK makes every list a chunked one
SHAPES = [  # (n, m, k, c)
    (500, 1000, 16, 32), (500, 1000, 3, 64), (64, 65, 17, 33), (1, 1000, 3, 4), (64, 63, 64, 67), (500, 64, 1, 256),
    (1, 1, 1, 1), (64, 1000, 16, 3), (500, 65, 64, 6), (1, 63, 17, 64), (500, 1, 3, 1), (64, 64, 16, 256),
]
