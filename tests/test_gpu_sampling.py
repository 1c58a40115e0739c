"""Furthest-point sampling on the device (csrc/sampling.hip): seg3d_furthest_sampling and ops.sectorized_fps against the
numpy restatement (tests/fps_ref.py) and the host entry, bit for bit.  Shapes are the smallest at which each path of the
kernel runs: wave and workgroup edges, both sides of the resident / streaming threshold, at most 256 picks a segment."""
import numpy as np
import pytest
import torch

import fps_ref
from fps_ref import RESIDENT, SECTOR_CASES, fps_ref as ref_fps, sector_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from openseg3d_amd import ops
    return ops


def _device(ops, dev, xyz, off, noff):
    out = ops.furthestsampling(torch.from_numpy(xyz).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(noff).to(dev))
    assert out.is_cuda and out.dtype == torch.int32 and out.shape == (int(noff[-1]),)
    return out.cpu().numpy()


@pytest.mark.parametrize("case", ["mixed", "tie_free", "ties", "ties_streaming"])
def test_device_equals_restatement_and_host(ops, dev, case):
    """mixed: segments of 1, 2, 63, 64, 65, 1023, 1024, 1025, RESIDENT - 1, RESIDENT, RESIDENT + 1 and 3 RESIDENT + 5 rows,
    one with 0 slots, one with 1 slot, one asked for more picks than it has rows.  ties: 64 points 8 times each, in the
    resident tier and (padded with copies of a far point) in the streaming tier."""
    xyz, off, noff = {"mixed": fps_ref.mixed_batch, "tie_free": fps_ref.tie_free_batch,
                      "ties": lambda: fps_ref.tie_cloud(False), "ties_streaming": lambda: fps_ref.tie_cloud(True)}[case]()
    got = _device(ops, dev, xyz, off, noff)
    assert np.array_equal(got, ref_fps(xyz, off, noff))
    assert np.array_equal(got, ops.furthestsampling(xyz, off, noff))
    assert np.array_equal(got, _device(ops, dev, xyz, off, noff))  # a second run gives the same rows


def test_zero_slot_segment_writes_nothing_and_empty_segment_gets_minus_one(ops, dev):
    """The raw entry on segments of (100 rows, 4 slots), (100, 0), (0, 3), (100, 2): the segment without slots leaves its
    neighbours' slots alone, the one without rows gets -1 (the wrapper raises before it comes to that)."""
    xyz = torch.from_numpy(fps_ref.lidar_like(300, 3)).to(dev)
    off = torch.tensor([100, 200, 200, 300], dtype=torch.int32, device=dev)
    noff = torch.tensor([4, 4, 7, 9], dtype=torch.int32, device=dev)
    idx = ops._fps_device(xyz, None, off, noff, 9).cpu().numpy()
    assert idx[0] == 0 and ((idx[:4] >= 0) & (idx[:4] < 100)).all()
    assert idx[4:7].tolist() == [-1, -1, -1] and idx[7] == 200 and 200 <= idx[8] < 300
    with pytest.raises(ValueError, match="segment 2 has no rows"):
        ops.furthestsampling(xyz, off, noff)


def test_every_row_exactly_once(ops, dev):
    xyz = np.random.default_rng(5).standard_normal((2048, 3)).astype(np.float32)
    one = np.array([2048], np.int32)
    got = _device(ops, dev, xyz, one, one)
    assert got[0] == 0 and np.array_equal(np.sort(got), np.arange(2048))
    assert np.array_equal(got, ops.furthestsampling(xyz, one, one))


def test_order_indirection(ops, dev):
    """A permuted `order` over a shuffled cloud = the flat call on the gathered cloud, mapped back; one resident and one
    streaming segment."""
    rng = np.random.default_rng(6)
    n = 3000 + RESIDENT + 700
    cloud = rng.standard_normal((n, 3)).astype(np.float32)
    off, noff = np.array([3000, n], np.int32), np.array([64, 128], np.int32)
    perm = rng.permutation(n)
    shuffled, order = np.ascontiguousarray(cloud[perm]), np.argsort(perm).astype(np.int32)
    flat = _device(ops, dev, cloud, off, noff)
    t = lambda a: torch.from_numpy(a).to(dev)
    got = ops._fps_device(t(shuffled), t(order), t(off), t(noff), 128).cpu().numpy()
    assert np.array_equal(got, order[flat])
    assert np.array_equal(got, ops._fps_host(shuffled, order, off, noff, 128))


def test_non_default_stream(ops, dev):
    xyz, off, noff = fps_ref.tie_free_batch()
    want = _device(ops, dev, xyz, off, noff)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = _device(ops, dev, xyz, off, noff)
    torch.cuda.current_stream(dev).wait_stream(side)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", sorted(SECTOR_CASES))
def test_sectorized_fps_equals_restatement_and_host(ops, dev, name):
    xyz, off, noff, num_sectors, min_points = sector_case(name)
    got = ops.sectorized_fps(torch.from_numpy(xyz).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(noff).to(dev),
                             num_sectors, min_points)
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == (int(noff[-1]),)
    got = got.cpu().numpy()
    assert np.array_equal(got, fps_ref.sectorized_fps_ref(xyz, off, noff, num_sectors, min_points))
    assert np.array_equal(got, ops.sectorized_fps(xyz, off, noff, num_sectors, min_points))


def test_sectorized_fps_value_errors(ops, dev):
    ring = fps_ref.lidar_like(4000, 8, gap=(-0.9, 0.9))  # sectors 3 and 4 of 8 hold no point
    off, noff = torch.tensor([4000], device=dev), torch.tensor([64], device=dev)
    with pytest.raises(ValueError, match="sector 3 of sample 0 holds no point"):
        ops.sectorized_fps(torch.from_numpy(ring).to(dev), off, noff, 8, min_points=1000)
    ring[17, 0] = np.nan
    with pytest.raises(ValueError, match="sample 0 has a row with NaN"):
        ops.sectorized_fps(torch.from_numpy(ring).to(dev), off, noff, 8, min_points=1000)
