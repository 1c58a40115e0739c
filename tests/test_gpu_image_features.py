"""GPU checks of ``seg3d_point_image_features`` (csrc/image_features.hip): the device entry against its host twin, bit for
bit, over the matrix of tests/test_image_features_host.py (the twin is compared with the numpy restatement there, and
once more here), at sizes around the wave and the 256-row tile and over many workgroups; element offsets past 2^31 on a
map that is allocated but never filled; ``WaymoDataset.assemble`` on a frame read from the packed file.  Everything is a
copy, so every comparison is exact; outputs are pre-filled with NaN / -7."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dataset_fixture as fx
from test_image_features_host import call_host, make_maps, make_rows, same, want

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_maps(maps, layout):
    """The same (C, H, W) views on the device, with the host arrays' strides."""
    out = {}
    for cam, m in maps.items():
        if layout == "chw":
            out[cam] = _t(m)
        elif layout == "hwc":
            out[cam] = _t(m.transpose(1, 2, 0)).permute(2, 0, 1)
        else:
            buf = torch.zeros((2 * m.shape[0],) + m.shape[1:], dtype=_t(m[:1]).dtype, device=DEV)
            buf[1::2] = _t(m)
            out[cam] = buf[1::2]
        assert list(out[cam].stride()) == [s // m.itemsize for s in m.strides]
    return out


def call_dev(rows, maps, cp_col=6, channels=None, outputs=None):
    """The device entry on outputs pre-filled with NaN / -7 (or on ``outputs`` as they stand)."""
    from openseg3d_amd import _lib, ops
    table = ops.feature_map_table(maps, False, rows.device, channels)
    n = rows.shape[0]
    if outputs is None:
        outputs = (torch.full((n, table.channels), float("nan"), dtype=torch.float32, device=DEV),
                   torch.full((n,), -7, dtype=torch.int32, device=DEV), torch.full((1,), -7, dtype=torch.int32, device=DEV))
    out, cam, count = outputs
    _lib.call("seg3d_point_image_features", ctypes.byref(table), rows.data_ptr(), rows.element_size(), n, rows.stride(0),
              cp_col, out.data_ptr(), cam.data_ptr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), cam.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("map_dtype", [np.float32, np.float16])
@pytest.mark.parametrize("layout", ["chw", "hwc", "sliced"])
@pytest.mark.parametrize("form", ["stride15", "copy12", "cp_col3"])
@pytest.mark.parametrize("row_dtype", [np.float64, np.float32])
def test_device_equals_twin(row_dtype, form, layout, map_dtype):
    maps = make_maps(28, map_dtype, layout, present=(0, 2, 3))
    rows, cp_col = make_rows(1000, row_dtype, form, n_outside=9)
    twin = call_host(rows, maps, cp_col)
    assert twin[2] == 9
    same(call_dev(_t(rows), dev_maps(maps, layout), cp_col), twin)
    if form == "stride15":  # the [:, :12] view of the raw rows, through its stride
        same(call_dev(_t(rows)[:, :12], dev_maps(maps, layout), 6), twin)


@pytest.mark.parametrize("order", ["range", "shuffled"])
@pytest.mark.parametrize("layout,channels", [("chw", 28), ("hwc", 28), ("chw", 64), ("sliced", 1), ("hwc", 8), ("chw", 33)])
def test_sizes_and_workgroups(layout, channels, order):
    """n around the wave and the tile, and 20 011 rows: 79 workgroups with a ragged last tile, outside rows in many of
    them.  33 and 64 channels take two chunks of the row-per-lane path."""
    from openseg3d_amd import ops
    maps = make_maps(channels, layout=layout)
    dmaps = dev_maps(maps, layout)
    for n in (0, 1, 63, 64, 65, 1000, 20011):
        rows, _ = make_rows(n, order=order, n_outside=min(n, 50) if n >= 1000 else 0)
        if n == 0:
            d, c, k = ops.point_image_features(_t(rows), dmaps, check=False)
            assert d.shape == (0, channels) and c.shape == (0,) and int(k.item()) == 0
            continue
        twin = call_host(rows, maps)
        if n == 20011:
            assert twin[2] == 50
        same(call_dev(_t(rows), dmaps), twin)
    rows, _ = make_rows(1000, order=order)
    same(call_dev(_t(rows), dmaps), want(rows, maps, 6, channels))  # and the restatement itself


def test_wrapper_unaligned_rows_and_counter():
    from openseg3d_amd import ops
    maps = make_maps(28)
    dmaps = dev_maps(maps, "chw")
    # an unaligned base: float32 rows starting one element into their buffer
    rows, _ = make_rows(1000, np.float32, order="shuffled")
    buf = torch.zeros((rows.size + 1,), dtype=torch.float32, device=DEV)
    buf[1:] = _t(rows).reshape(-1)
    shifted = buf[1:].view(1000, 15)
    assert shifted.data_ptr() % 8 == 4
    twin = call_host(rows, maps)
    same(call_dev(shifted, dmaps), twin)
    d, c = ops.point_image_features(shifted, dmaps)
    assert d.dtype == torch.float32 and c.dtype == torch.int32
    assert np.array_equal(d.cpu().numpy(), twin[0]) and np.array_equal(c.cpu().numpy(), twin[1])
    # the counter: outside rows in several workgroups; a second call on the same outputs restarts it at zero
    bad, _ = make_rows(20011, n_outside=50)
    outputs = (torch.full((20011, 28), float("nan"), device=DEV), torch.full((20011,), -7, dtype=torch.int32, device=DEV),
               torch.full((1,), -7, dtype=torch.int32, device=DEV))
    first = call_dev(_t(bad), dmaps, outputs=outputs)
    same(first, call_host(bad, maps))
    assert first[2] == 50
    good, _ = make_rows(20011)
    same(call_dev(_t(good), dmaps, outputs=outputs), call_host(good, maps))
    assert int(outputs[2].item()) == 0
    d, c, count = ops.point_image_features(_t(bad), dmaps, check=False)
    assert int(count.item()) == 50 and np.array_equal(c.cpu().numpy(), first[1])
    with pytest.raises(ops.ImageFeatureIndexError):
        ops.point_image_features(_t(bad), dmaps)
    # all maps absent
    d, c = ops.point_image_features(_t(good), {}, channels=5)
    assert d.shape == (20011, 5) and not d.any().item() and (c == -1).all().item()


def test_offsets_past_2_31():
    """One float16 (2, 1, 2^30 + 64) map, 4.3 GB, never filled: a handful of pixels with x >= 2^30 are set in both
    channels and looked up.  Channel 1 of those pixels lies at element offsets past 2^31 and byte offsets past 2^32."""
    from openseg3d_amd import ops
    width = 2 ** 30 + 64
    big = torch.empty((2, 1, width), dtype=torch.float16, device=DEV)
    xs = [2 ** 30, 2 ** 30 + 1, 2 ** 30 + 63, 2 ** 30 - 1, 0, 12345]
    vals = torch.tensor([[1.5 + i, -100.25 - i] for i in range(len(xs))], dtype=torch.float16, device=DEV)
    idx = torch.tensor(xs, device=DEV)
    big[0, 0, idx] = vals[:, 0]
    big[1, 0, idx] = vals[:, 1]
    assert big.stride(0) + xs[2] > 2 ** 31
    rows = np.zeros((len(xs) + 2, 15))
    rows[:len(xs), 6], rows[:len(xs), 7] = 1, np.array(xs, np.float64) + 0.25
    rows[len(xs), 6:9] = (1, width, 0)  # one past the last column
    d, c, count = ops.point_image_features(_t(rows), [big], check=False)
    assert int(count.item()) == 1 and c.cpu().tolist() == [0] * len(xs) + [-1, -1]
    assert torch.equal(d[:len(xs)], vals.float()) and not d[len(xs):].any().item()
    del big
    torch.cuda.empty_cache()


def test_assemble_from_packed_file(tmp_path):
    """A fixture frame read from the packed file gives the same device batch as the same frame read from the dict file."""
    from openseg3d_amd import image_features as imf
    from openseg3d_amd.dataset import WaymoDataset
    root = str(tmp_path / "waymo")
    names = fx.write(root, 0)
    ds = WaymoDataset(fx.make_cfg(True, False, True), root, "validation", device=DEV)
    name = names[1]
    index = ds.filenames.index(name)
    before = ds.assemble([ds[index]])
    rows, feats = ds._raw_image_features(name)
    n = np.load(os.path.join(root, "lidar", name + ".npy")).shape[0]
    dense, camera = np.zeros((n, fx.DIM_IMAGE_FEATURE), np.float32), np.full((n,), -1, np.int32)
    dense[rows], camera[rows] = feats, 0
    imf.save_packed(os.path.join(root, "image_feature", name), dense, camera)
    os.remove(os.path.join(root, "image_feature", name + ".npy"))
    after = ds.assemble([ds[index]])
    assert before["point_image_features"].any().item()
    assert torch.equal(after["point_image_features"], before["point_image_features"])
    assert torch.equal(after["points"], before["points"])
