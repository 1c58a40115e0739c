"""numpy float32 restatement of furthest-point sampling and of the sector partition of sectorized_fps, written from the
semantics stated in include/seg3d_hip.h (reference: seg3d/ops/sampling/src/sampling_cuda.cu:19-134 and
seg3d/ops/sampling/sampling.py:28-86), plus the input cases the host and device tests share.

fps_ref(..., tie="lowest") is the library's rule; tie="reference_tree" reproduces the CUDA kernel's per-thread strided scan
(:54-64, strict >) and its shared-memory tree (__update, :10-15, and :69-128) for a given block size, so that the tests can
show the tie rule to be the only divergence."""
import numpy as np
import torch

FAR = np.float32(1e10)
RESIDENT = 1024 * 16  # rows a workgroup keeps in registers (kFpsResident of csrc/sampling.hip)


def _tree_argmax(tmp, block):
    """Row the reference's block of `block` threads selects: thread tid scans rows tid, tid + block, .. with best = -1,
    besti = 0 and a strict >, then __update(tid, tid + half) for half = block / 2 .. 1 keeps i2 only where v2 > v1."""
    n = tmp.shape[0]
    rows = -(-n // block)
    pad = np.full((rows * block,), -1.0, np.float32)
    pad[:n] = tmp
    grid = pad.reshape(rows, block)
    first = np.argmax(grid, axis=0)  # first maximum down a thread's rows = the strict > of the scan
    vals = grid[first, np.arange(block)]
    inds = first * block + np.arange(block)
    inds[vals < 0] = 0  # a thread without rows keeps besti = start_n
    half = block // 2
    while half >= 1:
        v1, v2, i1, i2 = vals[:half], vals[half:2 * half], inds[:half], inds[half:2 * half]
        inds = np.where(v2 > v1, i2, i1)
        vals = np.maximum(v1, v2)
        half //= 2
    return int(inds[0])


def fps_ref(xyz, offset, new_offset, order=None, tie="lowest", block=1024, stats=None):
    """idx int32 [new_offset[-1]].  stats (a dict) receives 'tied_argmax' = the number of picks at which the largest
    running distance was attained by more than one row."""
    xyz = np.asarray(xyz, np.float32)
    offset, new_offset = np.asarray(offset, np.int64), np.asarray(new_offset, np.int64)
    idx = np.zeros((int(new_offset[-1]) if new_offset.size else 0,), np.int32)
    tied = 0
    for i in range(offset.shape[0]):
        s_n, e_n = (int(offset[i - 1]) if i else 0), int(offset[i])
        s_m, e_m = (int(new_offset[i - 1]) if i else 0), int(new_offset[i])
        if e_m <= s_m:
            continue
        if e_n <= s_n:
            idx[s_m:e_m] = -1
            continue
        rows = np.arange(s_n, e_n) if order is None else np.asarray(order)[s_n:e_n]
        x, y, z = (np.ascontiguousarray(xyz[rows, c]) for c in range(3))
        tmp = np.full((e_n - s_n,), FAR, np.float32)
        last = 0
        idx[s_m] = rows[0]
        for j in range(s_m + 1, e_m):
            dx, dy, dz = x - x[last], y - y[last], z - z[last]
            d = (dx * dx + dy * dy) + dz * dz  # float32 arrays: every operation rounded, nothing fused
            tmp = np.fmin(tmp, d)  # fminf: a NaN distance is dropped
            if stats is not None and np.count_nonzero(tmp == tmp.max()) > 1:
                tied += 1
            last = int(np.argmax(tmp)) if tie == "lowest" else _tree_argmax(tmp, block)
            idx[j] = rows[last]
    if stats is not None:
        stats["tied_argmax"] = tied
    return idx


def sector_partition_ref(xyz, offset, new_offset, num_sectors, min_points=10000):
    """sampling.py:37-69 with angle = float32(arctan2(float64 x, float64 y)): (indices int64 = rows grouped by sector,
    sector_offset, new_sector_offset), the last two cumulative."""
    xyz = np.asarray(xyz, np.float32)
    last, sizes, new_sizes, indices = 0, [], [], []
    for i in range(len(offset)):
        size = int(offset[i]) - last
        s = 1 if size < min_points else num_sectors
        b = xyz[last:last + size]
        angle = np.arctan2(b[:, 0].astype(np.float64), b[:, 1].astype(np.float64)).astype(np.float32)
        edges = torch.linspace(torch.tensor(angle.min()), torch.tensor(angle.max()) + 1e-4, s + 1).numpy()
        for t in range(s):
            indices.append(np.where((angle >= edges[t]) & (angle < edges[t + 1]))[0] + last)
            sizes.append(indices[-1].shape[0])
        new_size = int(new_offset[i]) - (int(new_offset[i - 1]) if i else 0)
        q = [new_size // s for _ in range(s)]
        q[-1] += new_size % s
        new_sizes += q
        last = int(offset[i])
    return np.concatenate(indices).astype(np.int64), np.cumsum(sizes), np.cumsum(new_sizes)


def sectorized_fps_ref(xyz, offset, new_offset, num_sectors, min_points=10000):
    """sampling.py:70-83: sample the gathered sector cloud, map the picks back."""
    xyz = np.asarray(xyz, np.float32)
    indices, sector_offset, new_sector_offset = sector_partition_ref(xyz, offset, new_offset, num_sectors, min_points)
    return indices[fps_ref(xyz[indices], sector_offset, new_sector_offset).astype(np.int64)]


# ------------------------------------------------------------------------------------------------------------ cases
def _cum(v):
    return np.cumsum(np.asarray(v, np.int64)).astype(np.int32)


def mixed_batch():
    """One batch of segments at every edge of the kernel: wave (64) and workgroup (1024) sizes, the last resident sizes
    (RESIDENT - 1, RESIDENT), the first streaming size and one of three times that, a segment with 0 slots, one with 1 slot
    and one asked for more picks than it has rows.  (length, picks) per segment."""
    segs = [(1, 1), (2, 2), (63, 40), (64, 64), (65, 33), (1023, 100), (77, 0), (1024, 256), (1025, 129), (50, 1),
            (RESIDENT - 1, 200), (RESIDENT, 256), (5, 9), (RESIDENT + 1, 101), (3 * RESIDENT + 5, 64)]
    rng = np.random.default_rng(20260)
    xyz = rng.standard_normal((sum(s for s, _ in segs), 3)).astype(np.float32)
    return xyz, _cum([s for s, _ in segs]), _cum([m for _, m in segs])


def tie_free_batch():
    """Random normal coordinates, every segment asked for fewer picks than it has rows: no exact tie is expected at any
    arg-max (the tests assert it), so every tie rule picks the same rows."""
    segs = [(2, 1), (63, 40), (65, 64), (1023, 100), (1025, 256), (3000, 200), (RESIDENT + 1, 60)]
    rng = np.random.default_rng(20261)
    xyz = rng.standard_normal((sum(s for s, _ in segs), 3)).astype(np.float32)
    return xyz, _cum([s for s, _ in segs]), _cum([m for _, m in segs])


def tie_cloud(streaming):
    """512 rows = 64 distinct points, 8 copies each, shuffled; 200 picks: exact ties among the copies from the second pick
    on, and after 64 picks every running distance is 0.  streaming: padded past the resident size with copies of one
    far-away point (themselves one large group of ties, spread over every thread)."""
    rng = np.random.default_rng(20262)
    pts = np.repeat(rng.standard_normal((64, 3)).astype(np.float32), 8, axis=0)[rng.permutation(512)]
    if streaming:
        pts = np.concatenate([pts, np.full((RESIDENT, 3), 1000.0, np.float32)])
    return pts, _cum([pts.shape[0]]), _cum([200])


def lidar_like(n, seed, gap=None):
    """A flat, ring-shaped cloud around the origin; gap = (lo, hi): no point with atan2(x, y) in that interval."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-np.pi, np.pi, 2 * n)
    if gap is not None:
        a = a[(a < gap[0]) | (a > gap[1])]
    a = a[:n]
    r = rng.uniform(3.0, 60.0, n)
    return np.stack([r * np.sin(a), r * np.cos(a), rng.normal(0.0, 1.0, n)], axis=1).astype(np.float32)


SECTOR_CASES = {
    # two samples: 30 000 rows in 8 sectors of 100 picks, 5 000 rows (< min_points) in one sector
    "two_samples": ([30000, 5000], [800, 128], 8, 10000),
    # 103 = 5 * 20 + 3: the last sector takes 23
    "remainder": ([12000], [103], 5, 10000),
}


def sector_case(name):
    sizes, new_sizes, num_sectors, min_points = SECTOR_CASES[name]
    xyz = np.concatenate([lidar_like(n, 100 + i) for i, n in enumerate(sizes)])
    return xyz, np.cumsum(sizes).astype(np.int32), np.cumsum(new_sizes).astype(np.int32), num_sectors, min_points
