"""Shared pieces of the window-attention tests (test_gpu_attention.py, test_gpu_attention_scale.py): window sets of chosen
sizes on chosen window cells, the fp64 restatement of _scaled_cosine_attention (cosine_msa.py:115-177) evaluated per window
and head from the CSR, and the library's own account of the schedule a call takes (seg3d_window_attn_schedule)."""
import collections
import ctypes

import numpy as np
import torch

import refcfg

WINDOW_SIZES = [1, 2, 15, 16, 17, 31, 32, 33, 64, 100, 129, 257, 300, 640]
# windows whose LAST 32-token tile holds 16 / 17 tokens (the backward skips the tile's empty second half) and the 128-token
# chunk edge with the same remainders
HALF_TILE_SIZES = [48, 49, 80, 81, 144, 145, 176, 177]

# wi: the WindowIndex; m: rows; which[w]: index into the size list of window w (the CSR's order); tok / starts / counts:
# host copies of wi.tok, win_start, win_count (rows(w) = flat rows of window w in the CSR's token order); owner[row]: index
# into the size list of the window a flat row was built for
Windows = collections.namedtuple("Windows", "wi m which tok starts counts owner")


def rows_of(ws, w):
    return ws.tok[ws.starts[w]:ws.starts[w] + ws.counts[w]]


def n_cells(stage=0):
    grid = refcfg.GRID_CART // 2 ** stage
    return [int(-(-int(g) // w)) for g, w in zip(grid, refcfg.WINDOW_SHAPE)]  # (x, y, z): 144 x 144 x 8 at stage 0


def windows_of(dev, sizes, stage=0, seed=0):
    """Voxel coordinates whose shift-0 windows hold exactly `sizes` tokens -- window i of the list on a window cell of its own
    (any number of windows up to the stage's canvas: 144 x 144 x 8 = 165 888 cells at stage 0), each on a subset of its cell's
    voxels, rows shuffled -- and their plan.  What belongs to which window is read back from the plan's CSR."""
    from openseg3d_amd.swformer import SparseWindowPartitionLayer
    wx, wy, wz = refcfg.WINDOW_SHAPE
    vol = wx * wy * wz
    cx, cy, cz = n_cells(stage)
    sizes = np.asarray(sizes, dtype=np.int64)
    n_win = sizes.shape[0]
    assert n_win <= cx * cy * cz and int(sizes.max()) <= vol and int(sizes.min()) >= 1
    rs = np.random.RandomState(seed)
    owner = np.repeat(np.arange(n_win), sizes)
    if n_win <= 64 and stage == 0:
        # short lists: a random subset of the cell's sites per window, the windows along a strip of cells (x cell 1 + i, y cell
        # 1 + i % 3, z cell 1) -- draw for draw the layout the small attention tests have always used
        site = np.concatenate([rs.permutation(vol)[:n] for n in sizes])
        i = np.arange(n_win)
        cell = (cz > 1) * cx * cy + (1 + i % 3) * cx + 1 + i
    else:  # any number of windows on random cells, each on a random rotation of a fixed stride walk over its cell's sites
        cell = rs.permutation(cx * cy * cz)[:n_win]
        first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        assert np.gcd(333, vol) == 1  # distinct sites for n <= vol
        site = (rs.randint(0, vol, n_win)[owner] + (np.arange(owner.shape[0]) - first[owner]) * 333) % vol
    z, y, x = site // (wx * wy), (site // wx) % wy, site % wx
    c = cell[owner]
    coords = np.stack([np.zeros_like(c), (c // (cx * cy)) * wz + z, ((c // cx) % cy) * wy + y, (c % cx) * wx + x], axis=1).astype(np.int32)
    perm = rs.permutation(coords.shape[0])
    coords, owner = coords[perm], owner[perm]
    grid = (refcfg.GRID_CART // 2 ** stage).tolist()
    part = SparseWindowPartitionLayer(refcfg.BATCHING_INFO[stage], refcfg.WINDOW_SHAPE, grid)
    wi = part.plan(torch.from_numpy(coords).to(dev), 1, 48).index[0]
    assert wi.n_windows == n_win and wi.n_dropped == 0
    tok = wi.tok[: coords.shape[0]].cpu().long()
    starts, counts = wi.win_start[:n_win].cpu().long(), wi.win_count[:n_win].cpu().long()
    owner_t = torch.from_numpy(owner)
    which = owner_t[tok[starts]]
    assert torch.equal(counts, torch.from_numpy(sizes)[which]) and torch.equal(which.sort().values, torch.arange(n_win))
    # every token of a window was built for that window
    assert torch.equal(owner_t[tok], torch.repeat_interleave(which, counts))
    return Windows(wi, coords.shape[0], which, tok, starts.tolist(), counts.tolist(), owner_t)


def reference(qk, v, tau, tau_min, heads, wi, keep=None):
    """fp64, one (window, head) at a time; keep[(w, h)] = optional [n, n] dropout factor (0 or 1 / keep_prob)."""
    m, c = v.shape
    dh = c // heads
    q, k = qk[:, :c], qk[:, c:]
    tok = wi.tok.cpu().long()
    starts, counts = wi.win_start[: wi.n_windows].cpu().tolist(), wi.win_count[: wi.n_windows].cpu().tolist()
    out = torch.zeros(m, c, dtype=torch.float64)
    scale = 1.0 / torch.clamp(tau.reshape(()), min=tau_min)
    pieces = []
    for w, (s, n) in enumerate(zip(starts, counts)):
        rows = tok[s:s + n]
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            qh = torch.nn.functional.normalize(q[rows][:, sl], dim=-1, eps=1e-12)
            kh = torch.nn.functional.normalize(k[rows][:, sl], dim=-1, eps=1e-12)
            p = torch.softmax(qh @ kh.t() * scale, dim=-1)
            if keep is not None:
                p = p * keep[(w, h)]
            pieces.append((rows, sl, p @ v[rows][:, sl]))
    for rows, sl, o in pieces:
        out[rows, sl] = out[rows, sl] + o  # index_put on disjoint (rows, head) blocks: differentiable
    return out


def reference_grouped(qk, v, tau, tau_min, heads, wi):
    """reference() without dropout for MANY small windows: the windows of one size are evaluated as one batch [windows, heads,
    n, dh] (the per-(window, head) loop takes 15 s for 1 000 windows of 1 .. 5 tokens, this 0.1 s).  Same operations per
    window and head, same fp64; test_attn_ref.py holds it to reference() on a mixed window set, forward and autograd."""
    m, c = v.shape
    dh = c // heads
    tok = wi.tok.cpu().long()
    starts, counts = wi.win_start[: wi.n_windows].cpu().long(), wi.win_count[: wi.n_windows].cpu().long()
    scale = 1.0 / torch.clamp(tau.reshape(()), min=tau_min)
    out = torch.zeros(m, c, dtype=torch.float64)
    for n in sorted(set(counts.tolist())):
        rows = tok[starts[counts == n][:, None] + torch.arange(n)[None, :]]  # [windows, n]
        nw = rows.shape[0]
        qh, kh, vh = (t[rows.reshape(-1)].reshape(nw, n, heads, dh).transpose(1, 2) for t in (qk[:, :c], qk[:, c:], v))
        qh = torch.nn.functional.normalize(qh, dim=-1, eps=1e-12)
        kh = torch.nn.functional.normalize(kh, dim=-1, eps=1e-12)
        p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
        out = out.index_put((rows.reshape(-1),), (p @ vh).transpose(1, 2).reshape(nw * n, c))  # disjoint rows
    return out


Schedule = collections.namedtuple("Schedule", "kernel cap grid walked xcd_block bwd_blocks")
FUSED, VECTOR_ALU = 0, 1


def schedule(n_tiles, n_chunks, heads, dh, p=0.0):
    """What the library says a call with these counts runs (computed by the launchers' own host code): forward kernel, forward
    grid cap, forward grid, most units one forward workgroup walks, items per XCD block, workgroups of a backward pass."""
    from openseg3d_amd import _lib
    out = (ctypes.c_int32 * 6)()
    rc = _lib.load().seg3d_window_attn_schedule(int(n_tiles), int(n_chunks), int(heads), int(dh), float(p), out)
    assert rc == 0, rc
    return Schedule(*list(out))


def schedule_of(wi, heads, dh, p=0.0):
    return schedule(wi.n_tiles, wi.n_qgroups, heads, dh, p)
