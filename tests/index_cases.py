"""Input builders and plain references for the integer structures (voxel list, coordinate hash, neighbour tables, chained
coarse site lists, window CSR and attention work items), shared by tests/test_index_range_host.py (no GPU: the host
voxelizer and these references against the oracle) and tests/test_gpu_index_range.py (the device against both).

Every input is inside the documented contract: coordinates inside the declared shape, distinct sites, batch ids in
[0, batch).  Nothing here is a tolerance: all comparisons made with these references are exact."""
import functools

import numpy as np
import torch

from oracle import index_ops
from oracle import window as owin

# ------------------------------------------------------------------------------------------ A: voxelizer
SMALL_RANGE, SMALL_VOXEL = [-1.6, -0.8, -0.3, 1.6, 0.8, 0.5], [0.1, 0.1, 0.1]        # grid 32 x 16 x 8, inexact 0.1
PAT_RANGE, PAT_VOXEL = [-4.0, -4.0, -1.0, 4.0, 4.0, 1.0], [0.125, 0.125, 0.125]      # grid 64 x 64 x 16, exact
BIG_RANGE, BIG_VOXEL = [-512.0, -512.0, -8.0, 512.0, 512.0, 8.0], [0.125, 0.125, 0.125]  # grid 8192 x 8192 x 128
PATTERN_SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]  # wave, workgroup and 2048-element scan chunk edges
DTYPES = ["float32", "float64"]


def voxelize_loop(points, voxel_size, point_cloud_range, xyz_col=0, batch_col=-1):
    """Plain first-seen loop: cells = np.floor((p - lo) / vs) in the point dtype with the float32 constants widened, a dict
    keyed by (b, z, y, x).  A point with a cell outside [0, grid) -- every comparison with a NaN is false, so a NaN is
    outside -- gets id -1 and creates nothing.  Returns (coords int32 [M, 4], ids int32 [N])."""
    pts = np.asarray(points)
    dt = pts.dtype
    lo = np.asarray(point_cloud_range[:3], dtype=np.float32).astype(dt)
    vs = np.asarray(voxel_size, dtype=np.float32).astype(dt)
    grid = index_ops.grid_size_of(voxel_size, point_cloud_range).astype(dt)
    with np.errstate(invalid="ignore"):
        c = np.floor((pts[:, xyz_col:xyz_col + 3] - lo) / vs)
        assert c.dtype == dt
        ok = ((c >= 0) & (c < grid)).all(axis=1)
    b = pts[:, batch_col].astype(np.int64) if batch_col >= 0 else np.zeros(pts.shape[0], np.int64)
    ids = np.full((pts.shape[0],), -1, dtype=np.int32)
    seen, rows = {}, []
    for i in np.nonzero(ok)[0]:
        key = (int(b[i]), int(c[i, 2]), int(c[i, 1]), int(c[i, 0]))
        j = seen.get(key)
        if j is None:
            j = seen[key] = len(rows)
            rows.append(key)
        ids[i] = j
    return np.array(rows, dtype=np.int32).reshape(-1, 4), ids


def _centres(cells_xyz, rng, vs, dtype):
    """Centre of every cell (exact in float32 for the 0.125 grids; well inside the cell for the 0.1 grid)."""
    lo = np.asarray(rng[:3], dtype=np.float64)
    return ((np.asarray(cells_xyz, dtype=np.float64) + 0.5) * np.asarray(vs, dtype=np.float64) + lo).astype(dtype)


def _edge_values(axis):
    """Every lo + k * vs of one axis of the small grid, as float32 arithmetic, as float64 arithmetic on the widened float32
    constants and as the decimal value, each with its float32 and float64 neighbours on both sides; +-0, hi, and the
    neighbours just inside hi and just outside lo.  float64 values (the float32 test rounds them)."""
    lo32, hi32, vs32 = (np.float32(SMALL_RANGE[axis]), np.float32(SMALL_RANGE[3 + axis]), np.float32(SMALL_VOXEL[axis]))
    g = int(index_ops.grid_size_of(SMALL_VOXEL, SMALL_RANGE)[axis])
    inf = np.inf
    vals = [0.0, -0.0]
    for k in range(g + 1):
        for e in (float(np.float32(lo32 + np.float32(k) * vs32)), float(lo32) + k * float(vs32),
                  round(SMALL_RANGE[axis] + k * 0.1, 6)):
            e32 = np.float32(e)
            vals += [e, float(np.nextafter(e32, np.float32(inf))), float(np.nextafter(e32, np.float32(-inf))),
                     float(e32), float(np.nextafter(e, inf)), float(np.nextafter(e, -inf))]
    vals += [float(hi32), float(np.nextafter(hi32, np.float32(-inf))), float(np.nextafter(float(hi32), -inf)),
             float(np.nextafter(lo32, np.float32(-inf))), float(np.nextafter(float(lo32), -inf))]
    return np.array(vals, dtype=np.float64)


def _edge_points(dtype):
    rs = np.random.RandomState(11)
    mid = _centres([[3, 5, 2]], SMALL_RANGE, SMALL_VOXEL, np.float64)[0]
    vals = [_edge_values(a) for a in range(3)]
    rows = []
    for a in range(3):  # one axis walks its edge values, the other two stay in one cell
        p = np.tile(mid, (vals[a].shape[0], 1))
        p[:, a] = vals[a]
        rows.append(p)
    rows.append(np.stack([vals[a][rs.randint(0, vals[a].shape[0], 700)] for a in range(3)], axis=1))
    return np.concatenate(rows).astype(dtype)


def _nonfinite_points(dtype):
    """(points, bad mask): valid points with rows that hold NaN / +Inf / -Inf in each column mixed in, at the first row, at
    wave edges and in the middle."""
    rs = np.random.RandomState(12)
    n = 420
    cells = np.stack([rs.randint(0, 32, n), rs.randint(0, 16, n), rs.randint(0, 8, n)], axis=1)
    cells[rs.rand(n) < 0.3] = cells[0]  # a cell that many points share
    pts = _centres(cells, SMALL_RANGE, SMALL_VOXEL, np.float64) + rs.uniform(-0.03, 0.03, (n, 3))
    at = [0, 1, 63, 64, 65, 127, 128, 200, 255, 256, 300, n - 1]
    bad = np.zeros(n, bool)
    specials = [(c, v) for c in range(3) for v in (np.nan, np.inf, -np.inf)]
    for i, (c, v) in zip(at, specials):
        pts[i, c] = v
        bad[i] = True
    pts[at[9]] = np.nan
    pts[at[10]] = (np.inf, np.nan, -np.inf)
    pts[at[11], 2] = np.nan
    bad[[at[9], at[10], at[11]]] = True
    return pts.astype(dtype), bad


def _pat_cells(lin):
    lin = np.asarray(lin, dtype=np.int64)
    return np.stack([lin % 64, (lin // 64) % 64, lin // 4096], axis=1)


def _pat_points(lin, dtype, reject=None):
    pts = _centres(_pat_cells(lin), PAT_RANGE, PAT_VOXEL, dtype)
    if reject is not None:
        pts[np.asarray(reject, bool), 0] = 5.0  # x beyond hi: rejected
    return pts


def _runs(with_reject):
    """Runs of equal cells of lengths 1 .. 130 end to end (a cell comes back every 97 runs); optionally a rejected point in
    the middle of every run of two or more."""
    lin, rej = [], []
    for length in range(1, 131):
        cell = 100 + (length * 7) % 97
        run, r = [cell] * length, [False] * length
        if with_reject and length >= 2:
            run.insert(length // 2, cell)
            r.insert(length // 2, True)
        lin += run
        rej += r
    return np.array(lin), np.array(rej)


def _layout(xyz, batch, stride, xyz_col, batch_col, dtype, seed):
    rows = np.random.RandomState(seed).uniform(-50, 50, (xyz.shape[0], stride))
    rows[:, xyz_col:xyz_col + 3] = xyz
    if batch_col >= 0:
        rows[:, batch_col] = batch
    return rows.astype(dtype)


@functools.lru_cache(maxsize=None)
def voxel_cases(dtype):
    """name -> dict(points, voxel, range, xyz_col, batch_col) for section A, in the given point dtype."""
    dt = np.dtype(dtype)
    cases = {}

    def add(name, points, voxel, rng, xyz_col=0, batch_col=-1):
        cases[name] = dict(points=np.ascontiguousarray(points, dtype=dt), voxel=voxel, range=rng, xyz_col=xyz_col,
                           batch_col=batch_col)

    add("edges", _edge_points(dt), SMALL_VOXEL, SMALL_RANGE)
    add("nonfinite", _nonfinite_points(dt)[0], SMALL_VOXEL, SMALL_RANGE)
    for n in PATTERN_SIZES + [100003]:
        add(f"one_cell_{n}", _pat_points(np.full(n, 12345), dt), PAT_VOXEL, PAT_RANGE)
    for n in PATTERN_SIZES:
        add(f"own_cell_{n}", _pat_points((np.arange(n) * 40503) % 65536, dt), PAT_VOXEL, PAT_RANGE)
        add(f"alternating_{n}", _pat_points(np.where(np.arange(n) % 2 == 0, 777, 40000), dt), PAT_VOXEL, PAT_RANGE)
    lin, _ = _runs(False)
    add("runs", _pat_points(lin, dt), PAT_VOXEL, PAT_RANGE)
    lin, rej = _runs(True)
    add("runs_rejected", _pat_points(lin, dt, rej), PAT_VOXEL, PAT_RANGE)
    rej = np.zeros(256, bool)
    rej[[0, 63, 64, 127, 128, 191, 192, 255]] = True  # lanes 0 and 63 of every wave of one workgroup
    add("run_rejected_lane_0_63", _pat_points(np.full(256, 4242), dt, rej), PAT_VOXEL, PAT_RANGE)
    lin = (np.arange(600) * 40503) % 65536
    lin[256] = lin[255]  # first seen by the last point of workgroup 0, revisited by the first point of workgroup 1
    lin[512] = lin[511] = lin[10]  # seen early, revisited on both sides of the next workgroup edge
    add("workgroup_edge", _pat_points(lin, dt), PAT_VOXEL, PAT_RANGE)

    rs = np.random.RandomState(13)
    pool = np.stack([rs.randint(0, 32, 60), rs.randint(0, 16, 60), rs.randint(0, 8, 60)], axis=1)
    xyz = _centres(pool[rs.randint(0, 60, 500)], SMALL_RANGE, SMALL_VOXEL, np.float64) + rs.uniform(-0.03, 0.03, (500, 3))
    xyz[rs.rand(500) < 0.05, 1] = 7.0  # some rejected points
    batch = np.array([0, 2, 3])[rs.randint(0, 3, 500)]  # interleaved; sample 1 is empty
    for stride, xc, bc in [(3, 0, -1), (5, 1, -1), (6, 2, -1), (4, 1, 0), (7, 1, 0), (6, 2, 0), (6, 2, 1), (4, 0, 3),
                           (6, 0, 5), (6, 1, 4)]:
        add(f"layout_s{stride}_x{xc}_b{bc}", _layout(xyz, batch, stride, xc, bc, dt, 14), SMALL_VOXEL, SMALL_RANGE, xc, bc)

    # linear cell index ((b * 128 + z) * 8192 + y) * 8192 + x: (z, z + 64) and (b, b + 1) differ by multiples of 2^32
    rs = np.random.RandomState(15)
    rows = []
    for _ in range(12):
        z, y, x = rs.randint(0, 64), rs.randint(0, 8192), rs.randint(0, 8192)
        rows += [(b, zz, y, x) for b in (0, 1, 2) for zz in (z, z + 64)]
    rows = np.array(rows + rows)[rs.permutation(2 * len(rows))]
    assert (((rows[:, 0] * 128 + rows[:, 1]) * 8192 + rows[:, 2]) * 8192 + rows[:, 3]).max() >= 2 ** 32
    pts = np.concatenate([rows[:, :1].astype(np.float64), _centres(rows[:, [3, 2, 1]], BIG_RANGE, BIG_VOXEL, np.float64)], 1)
    add("keys_beyond_2_32", pts, BIG_VOXEL, BIG_RANGE, 1, 0)
    return cases


@functools.lru_cache(maxsize=None)
def voxel_expected(name, dtype):
    """(coords [M, 4], ids [N]) of a case by the plain loop; for "nonfinite" the loop runs on the input with the non-finite
    rows deleted, and those rows get -1."""
    c = voxel_cases(dtype)[name]
    if name == "nonfinite":
        _, bad = _nonfinite_points(np.dtype(dtype))
        coords, good_ids = voxelize_loop(c["points"][~bad], c["voxel"], c["range"])
        ids = np.full((bad.shape[0],), -1, dtype=np.int32)
        ids[~bad] = good_ids
        return coords, ids
    return voxelize_loop(c["points"], c["voxel"], c["range"], c["xyz_col"], c["batch_col"])


def is_single_sample(case):
    """The oracle takes one sample with xyz in the first three columns."""
    return case["batch_col"] < 0 and case["xyz_col"] == 0


# ------------------------------------------------------------------------------------------ B: site structures
def full_sites(shape, batch=1):
    b, z, y, x = np.meshgrid(np.arange(batch), np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    return np.stack([b.ravel(), z.ravel(), y.ravel(), x.ravel()], axis=1).astype(np.int32)


def corner_sites(shape, batch=1):
    c = full_sites(shape, batch)
    hi = np.asarray(shape) - 1
    return c[(((c[:, 1:] == 0) | (c[:, 1:] == hi)).all(axis=1))]


def random_sites(shape, batch, m, seed):
    """m distinct sites in random order."""
    cells = int(np.prod(shape)) * batch
    lin = np.random.RandomState(seed).permutation(cells)[:m]
    x, r = lin % shape[2], lin // shape[2]
    y, r = r % shape[1], r // shape[1]
    return np.stack([r // shape[0], r % shape[0], y, x], axis=1).astype(np.int32)


def _shuffled(coords, seed):
    return coords[np.random.RandomState(seed).permutation(coords.shape[0])]


ROW_COUNTS = [0, 1, 255, 256, 257, 2049]


@functools.lru_cache(maxsize=None)
def site_cases():
    """name -> (coords int32 [M, 4] in random order, shape zyx, batch)."""
    cases = {}
    for shape in ([1, 1, 1], [1, 1, 2], [2, 3, 5], [7, 6, 5], [8, 11, 8]):
        tag = "x".join(str(s) for s in shape)
        cases[f"full_{tag}"] = (_shuffled(full_sites(shape), 1), shape, 1)
        cases[f"corners_{tag}"] = (_shuffled(corner_sites(shape), 2), shape, 1)
    # coarse level of [7, 6, 5] is [4, 3, 3] = 36 cells per sample: bitmap words straddle samples
    cases["batch3_full_7x6x5"] = (_shuffled(full_sites([7, 6, 5], 3), 3), [7, 6, 5], 3)
    cases["batch3_corners_7x6x5"] = (_shuffled(corner_sites([7, 6, 5], 3), 4), [7, 6, 5], 3)
    cases["batch3_random_7x6x5"] = (random_sites([7, 6, 5], 3, 200, 5), [7, 6, 5], 3)
    for m in ROW_COUNTS:
        if m == 1:
            cases["rows_1"] = (np.array([[1, 7, 11, 9]], dtype=np.int32), [16, 24, 20], 2)  # away from every border
        else:
            cases[f"rows_{m}"] = (random_sites([16, 24, 20], 2, m, 6 + m), [16, 24, 20], 2)
    # a fully occupied block but for one site: 8191 rows in a table of 16384 slots, the highest load (and the longest probe
    # chains) the capacity rule of >= 2 m + 2 slots allows
    cases["hash_block_8191"] = (_shuffled(full_sites([16, 16, 32]), 7)[:-1], [16, 16, 32], 1)
    return cases


def big_key_sites():
    """Sparse sites in a 128 x 8192 x 8192 shape, batch 2: site keys above 2^32 in groups that alias under 32-bit
    truncation ((z, z + 64) and (b, b + 1) differ by multiples of 2^32), each with a neighbour or two so the table has hits."""
    rs = np.random.RandomState(8)
    shape = [128, 8192, 8192]
    rows = set()
    for _ in range(10):
        z, y, x = rs.randint(1, 63), rs.randint(1, 8191), rs.randint(1, 8191)
        for b in (0, 1):
            for zz in (z, z + 64):
                rows.add((b, zz, y, x))
        rows.add((0, z, y, x + 1))
        rows.add((1, z + 64, y + 1, x))
        rows.add((1, z + 1, y - 1, x - 1))
    coords = _shuffled(np.array(sorted(rows), dtype=np.int32), 9)
    key = ((coords[:, 0].astype(np.int64) * 128 + coords[:, 1]) * 8192 + coords[:, 2]) * 8192 + coords[:, 3]
    assert key.max() >= 2 ** 32 and np.unique(key & 0xFFFFFFFF).shape[0] < key.shape[0]
    return coords, shape, 2


def subm_dict(coords, shape):
    """[27, M] submanifold table by a dict lookup on (b, z, y, x) tuples."""
    rows = {tuple(int(v) for v in c): i for i, c in enumerate(coords)}
    nbr = np.full((27, coords.shape[0]), -1, dtype=np.int32)
    for k in range(27):
        dz, dy, dx = k // 9 - 1, (k // 3) % 3 - 1, k % 3 - 1
        for i, (b, z, y, x) in enumerate(coords):
            p = (int(b), int(z) + dz, int(y) + dy, int(x) + dx)
            if 0 <= p[1] < shape[0] and 0 <= p[2] < shape[1] and 0 <= p[3] < shape[2]:
                nbr[k, i] = rows.get(p, -1)
    return nbr


def parity_ref(coords):
    """Rows grouped by (z & 1, y & 1, x & 1), original order kept inside a group."""
    key = (coords[:, 1] & 1) * 4 + (coords[:, 2] & 1) * 2 + (coords[:, 3] & 1)
    return np.argsort(key, kind="stable").astype(np.int32)


STALE_COUNTS = [0, 1, 255, 256, 300]


def stale_tail_buffer():
    """(buffer of 600 distinct sites, shape, batch): any prefix is a valid site list; the rows behind it are valid sites of
    the same shape that would add output sites if they were read."""
    return random_sites([13, 22, 19], 3, 600, 21), [13, 22, 19], 3


# ------------------------------------------------------------------------------------------ C: window partition
def levels_of(info):
    return [(v["batching_range"][0], v["batching_range"][1], v["max_tokens"]) for _, v in sorted(info.items())]


def window_ids_ref(coords, sparse_shape_xyz, window_shape, do_shift):
    """(win int64 [M], in_win int64 [M, 3]) by the oracle's get_window_coors."""
    win, in_win = owin.window_coords(torch.from_numpy(np.asarray(coords)).long(), sparse_shape_xyz, window_shape, do_shift)
    return win.numpy(), in_win.numpy()


def levels_ref(win, info):
    """(rank, level, slot) of every voxel from the oracle's batching_single_shift and flat2win_inds: the slot counts a
    level's own windows only; a voxel whose rank reaches its level's max_tokens, or whose window matches no range, has
    slot -1 (the oracle's slot formula is kept for every other voxel)."""
    w = torch.from_numpy(np.asarray(win, dtype=np.int64))
    keep, level = owin.batching_single_shift(w, info)
    inds = owin.flat2win_inds(w, level, info)
    slot = np.full((w.shape[0],), -1, dtype=np.int64)
    for bl in info:
        if bl in inds:
            s, (rows,) = inds[bl]
            slot[rows.numpy()] = s.numpy()
    slot[~keep.numpy()] = -1
    return index_ops.ingroup_rank(w.numpy()), level.numpy(), slot


def window_expect(win):
    """Closed form of the CSR and the attention work items from the window ids: windows in ascending id order, tokens in
    ascending row order, one tile_item per 32 tokens and one qg_item per 128 tokens of a window."""
    win = np.asarray(win, dtype=np.int64)
    uniq, cnt = np.unique(win, return_counts=True)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64) if cnt.size else np.zeros(0, np.int64)

    def items(per):
        nt = (cnt + per - 1) // per
        first = np.concatenate([[0], np.cumsum(nt)[:-1]]).astype(np.int64) if nt.size else np.zeros(0, np.int64)
        w = np.repeat(np.arange(uniq.shape[0]), nt)
        t = np.arange(int(nt.sum())) - np.repeat(first, nt)
        return first, np.stack([w, t, start[w], cnt[w]], axis=1).reshape(-1, 4)

    tile0, tile_item = items(32)
    _, qg_item = items(128)
    return dict(tok=np.argsort(win, kind="stable"), win_start=start, win_count=cnt, win_tile0=tile0, tile_item=tile_item,
                qg_item=qg_item, n_windows=uniq.shape[0], n_tiles=tile_item.shape[0], n_qgroups=qg_item.shape[0])


WINDOW_SHAPES = [[10, 10, 8], [2, 3, 2], [5, 7, 3]]
# per window shape: grid (x, y, z) a multiple of the window, not a multiple, and with sz == wz (no z shift)
GEOMETRY_GRIDS = {0: [[40, 30, 16], [37, 23, 13], [37, 23, 8]], 1: [[8, 9, 4], [7, 8, 5], [7, 8, 2]],
                  2: [[20, 21, 9], [19, 17, 8], [19, 17, 3]]}


def geometry_coords(grid_xyz, batch, seed):
    """Up to 1500 distinct voxels per sample in random order, with the corner at 0 and the corner at the largest coordinate."""
    shape = [grid_xyz[2], grid_xyz[1], grid_xyz[0]]
    cells = int(np.prod(shape))
    c = random_sites(shape, batch, min(cells * batch, 1500 * batch), seed)
    ends = np.array([[b, z, y, x] for b in range(batch) for z, y, x in ([0, 0, 0], [s - 1 for s in shape])], dtype=np.int32)
    return _shuffled(np.unique(np.concatenate([ends, c]), axis=0), seed)


OCCUPANCIES = [1, 0, 31, 1, 32, 0, 33, 1, 127, 0, 128, 1, 129, 0, 257, 1, 800]  # separated by empty and one-token windows


def occupancy_coords(window_shape, do_shift, per_sample):
    """Windows filled cell by cell to the given occupancies, one after the other along x (window (j + 1, 1, 1) of sample b
    gets per_sample[b][j] voxels), rows in random order.  Returns (coords, sparse_shape_xyz); the grid is two windows deep
    in y and z, so the z shift applies."""
    wx, wy, wz = window_shape
    n = max(len(p) for p in per_sample)
    sparse = [(n + 1) * wx, 2 * wy, 2 * wz]
    shift = [wx // 2, wy // 2, wz // 2] if do_shift else [wx, wy, wz]
    cz, cy, cx = np.meshgrid(np.arange(wz), np.arange(wy), np.arange(wx), indexing="ij")
    cell = np.stack([cz.ravel(), cy.ravel(), cx.ravel()], axis=1)
    rows = []
    for b, occ in enumerate(per_sample):
        for j, k in enumerate(occ):
            c = cell[:k]
            rows.append(np.stack([np.full(k, b), wz - shift[2] + c[:, 0], wy - shift[1] + c[:, 1],
                                  (j + 1) * wx - shift[0] + c[:, 2]], axis=1))
    coords = np.concatenate(rows).astype(np.int32)
    assert coords.min() >= 0 and (coords[:, 1:].max(axis=0) < np.array(sparse[::-1])).all()
    return _shuffled(coords, 31), sparse


LEVEL_TABLES = {
    "one_level": {0: {"max_tokens": 800, "batching_range": [0, 100000]}},
    "overlapping": {0: {"max_tokens": 800, "batching_range": [0, 200]}, 1: {"max_tokens": 800, "batching_range": [30, 130]},
                    2: {"max_tokens": 800, "batching_range": [100, 100000]}},
    # the occupancies 31, 32, 127, 128, 257, 800 are a range's hi - 1, lo, hi - 1, lo, hi (= the next lo) and hi - 1
    "range_ends": {0: {"max_tokens": 32, "batching_range": [1, 32]}, 1: {"max_tokens": 128, "batching_range": [32, 128]},
                   2: {"max_tokens": 256, "batching_range": [128, 257]}, 3: {"max_tokens": 800, "batching_range": [257, 801]}},
    # op level only: occupancies above max_tokens
    "over_cap": {0: {"max_tokens": 100, "batching_range": [0, 100000]}},
    # op level only: 128 and 129 match no range; their windows lie below the level-3 windows (257, 800) in id
    "unmatched": {0: {"max_tokens": 16, "batching_range": [0, 16]}, 1: {"max_tokens": 64, "batching_range": [16, 64]},
                  2: {"max_tokens": 128, "batching_range": [64, 128]}, 3: {"max_tokens": 800, "batching_range": [200, 100000]}},
}

CANVAS_SIZES = [2047, 2048, 2049, 524289, 526337]
CANVAS_WINDOW = [1, 1, 4]
CANVAS_INFO = {l: {"max_tokens": l + 1, "batching_range": [l + 1, l + 2]} for l in range(4)}  # occupancy o -> level o - 1


def canvas_coords(n_canvas):
    """Voxels of a [1, 1, n_canvas] window canvas with 4-cell windows along z: the first and the last canvas entry and the
    entries on both sides of every 2048 boundary, with 1 .. 4 voxels each (so all four scan lanes carry sums).  Returns
    (coords in random order, the canvas entry of each row)."""
    e = np.unique(np.concatenate([[0, n_canvas - 1], np.arange(2048, n_canvas, 2048) - 1, np.arange(2048, n_canvas, 2048)]))
    occ = 1 + (e * 7 // 3) % 4
    z = np.concatenate([4 * ee + np.arange(o) for ee, o in zip(e, occ)])
    z = z[np.random.RandomState(41).permutation(z.shape[0])]
    coords = np.zeros((z.shape[0], 4), dtype=np.int32)
    coords[:, 1] = z
    return coords, z // 4


def all_in_window(window_shape):
    """Every in-window coordinate (z, y, x) of a window, once."""
    wx, wy, wz = window_shape
    z, y, x = np.meshgrid(np.arange(wz), np.arange(wy), np.arange(wx), indexing="ij")
    return np.stack([z.ravel(), y.ravel(), x.ravel()], axis=1).astype(np.int32)
