"""Furthest-point sampling on the host: seg3d_furthest_sampling_host and the CPU / numpy paths of ops.furthestsampling and
ops.sectorized_fps against the numpy restatement (tests/fps_ref.py), bit for bit -- the results are row indices."""
import numpy as np
import pytest
import torch

import fps_ref
from fps_ref import SECTOR_CASES, fps_ref as ref_fps, sector_case


@pytest.fixture(scope="module")
def ops():
    from openseg3d_amd import ops
    return ops


@pytest.mark.parametrize("case", ["mixed", "tie_free", "ties", "ties_streaming"])
def test_host_entry_equals_restatement(ops, case):
    xyz, off, noff = {"mixed": fps_ref.mixed_batch, "tie_free": fps_ref.tie_free_batch,
                      "ties": lambda: fps_ref.tie_cloud(False), "ties_streaming": lambda: fps_ref.tie_cloud(True)}[case]()
    got = ops.furthestsampling(xyz, off, noff)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == (int(noff[-1]),)
    assert np.array_equal(got, ref_fps(xyz, off, noff))
    t = ops.furthestsampling(torch.from_numpy(xyz), torch.from_numpy(off), torch.from_numpy(noff))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int32 and np.array_equal(t.numpy(), got)


def test_every_row_once_and_degenerate_segments(ops):
    rng = np.random.default_rng(5)
    xyz = rng.standard_normal((2048, 3)).astype(np.float32)
    got = ops.furthestsampling(xyz, [2048], [2048])
    assert got[0] == 0 and np.array_equal(np.sort(got), np.arange(2048))
    assert np.array_equal(got, ref_fps(xyz, [2048], [2048]))
    # 0 slots: nothing written, the neighbours' slots untouched; more picks than rows: the lowest row of distance 0 again
    got = ops.furthestsampling(xyz[:12], [5, 9, 12], [3, 3, 9])
    assert got[:3].tolist() == ref_fps(xyz[:12], [5], [3]).tolist() and got[3] == 9
    assert sorted(got[3:6].tolist()) == [9, 10, 11] and got[6:].tolist() == [9, 9, 9]
    assert ops.furthestsampling(xyz[:12], [12], [0]).shape == (0,)


def test_tie_rule_is_the_only_divergence_from_the_reference_tree(ops):
    """On inputs without an exact tie at any arg-max (asserted, not assumed) the reference's reduction tree selects the
    rows the lowest-index rule selects, whatever its block size; with exact ties the two rules differ."""
    xyz, off, noff = fps_ref.tie_free_batch()
    stats = {}
    lowest = ref_fps(xyz, off, noff, stats=stats)
    assert stats["tied_argmax"] == 0
    for block in (64, 512, 1024):
        assert np.array_equal(ref_fps(xyz, off, noff, tie="reference_tree", block=block), lowest), block
    assert np.array_equal(ops.furthestsampling(xyz, off, noff), lowest)  # and so does the library's host entry
    xyz, off, noff = fps_ref.tie_cloud(False)
    stats = {}
    lowest = ref_fps(xyz, off, noff, stats=stats)
    assert stats["tied_argmax"] > 0
    trees = [ref_fps(xyz, off, noff, tie="reference_tree", block=b) for b in (64, 512)]
    assert not np.array_equal(trees[0], lowest) or not np.array_equal(trees[1], lowest)
    # the same points are chosen, only which copy differs
    assert np.array_equal(xyz[trees[0][:64]], xyz[lowest[:64]])


def test_order_indirection_host(ops):
    rng = np.random.default_rng(6)
    cloud = rng.standard_normal((4000, 3)).astype(np.float32)
    off, noff = np.array([1500, 4000], np.int32), np.array([40, 100], np.int32)
    perm = rng.permutation(4000)
    shuffled = np.ascontiguousarray(cloud[perm])  # shuffled[j] = cloud[perm[j]]
    order = np.argsort(perm).astype(np.int32)     # shuffled[order[k]] = cloud[k]
    flat = ops._fps_host(cloud, None, off, noff, 100)
    assert np.array_equal(ops._fps_host(shuffled, order, off, noff, 100), order[flat])
    assert np.array_equal(ref_fps(shuffled, off, noff, order=order), order[flat])


@pytest.mark.parametrize("name", sorted(SECTOR_CASES))
def test_sectorized_fps_cpu_equals_restatement(ops, name):
    xyz, off, noff, num_sectors, min_points = sector_case(name)
    got = ops.sectorized_fps(torch.from_numpy(xyz), torch.from_numpy(off), torch.from_numpy(noff), num_sectors, min_points)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.shape == (int(noff[-1]),)
    assert np.array_equal(got.numpy(), fps_ref.sectorized_fps_ref(xyz, off, noff, num_sectors, min_points))
    assert np.array_equal(ops.sectorized_fps(xyz, off, noff, num_sectors, min_points), got.numpy())
    # quotas sum to the requested sizes; the picks of sample i are rows of sample i
    _, _, new_sector_offset = fps_ref.sector_partition_ref(xyz, off, noff, num_sectors, min_points)
    assert new_sector_offset[-1] == noff[-1]
    lo_n = lo_m = 0
    for hi_n, hi_m in zip(off.tolist(), noff.tolist()):
        part = got.numpy()[lo_m:hi_m]
        assert ((part >= lo_n) & (part < hi_n)).all()
        lo_n, lo_m = hi_n, hi_m
    if name == "remainder":
        quotas = np.diff(new_sector_offset, prepend=0)
        assert quotas.tolist() == [20, 20, 20, 20, 23]


def test_sector_plan_quotas(ops):
    sizes, new_sizes = np.array([20000, 300, 15000]), np.array([1003, 77, 6])
    minmax = np.array([[-3.0, 3.0]] * 3, np.float32)
    edges, sector_offset, new_sector_offset, names = ops._sector_plan(sizes, new_sizes, minmax, 16, 10000)
    assert sector_offset.tolist() == [0, 16, 17, 33] and len(names) == 33 and edges.shape == (33 + 3,)
    quotas = np.diff(new_sector_offset, prepend=0)
    assert quotas[:16].sum() == 1003 and quotas[15] == 62 + 11 and quotas[16] == 77 and quotas[17:].tolist() == [0] * 15 + [6]
    assert np.array_equal(edges[:17], torch.linspace(torch.tensor(-3.0), torch.tensor(3.0) + 1e-4, 17).numpy())


def test_value_errors(ops):
    xyz = fps_ref.lidar_like(4000, 7)
    with pytest.raises(ValueError, match="segment 1 has no rows"):
        ops.furthestsampling(xyz, [4000, 4000], [10, 12])
    bad = xyz.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="sample 0 has a row with NaN"):
        ops.sectorized_fps(bad, [4000], [64], 8, min_points=1000)
    # a ring with an angular gap: sectors 3 and 4 of 8 (angles -pi/4 .. pi/4) hold no point
    ring = fps_ref.lidar_like(4000, 8, gap=(-0.9, 0.9))
    with pytest.raises(ValueError, match="sector 3 of sample 0 holds no point"):
        ops.sectorized_fps(ring, [4000], [64], 8, min_points=1000)
    assert ops.sectorized_fps(ring, [4000], [64], 8, min_points=5000).shape == (64,)  # one sector: nothing is empty
