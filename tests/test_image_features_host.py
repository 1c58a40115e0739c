"""CPU checks of the per-point image-feature query: ``seg3d_point_image_features_host`` against the numpy restatement of
tools/extract_image_feature.py:84-100 (tests/image_feature_ref.py), the two file formats, and the dataset's packed
branch.  Everything is a copy, so every comparison is exact; the outputs handed to the entry are pre-filled with NaN /
-7 to show that it writes them in full.  The entry's offsets are ``int64_t`` by construction; an offset past 2^31 is
exercised on the device only (tests/test_gpu_image_features.py), not here."""
import ctypes
import os
import shutil

import numpy as np
import pytest

import dataset_fixture as fx
import image_feature_ref as ref

SHAPES = ((40, 64), (33, 50), (40, 64), (33, 50), (40, 64))  # (H, W) of cameras 0..4: a few kilobytes each


def make_maps(channels, dtype=np.float32, layout="chw", present=(0, 1, 2, 3, 4), seed=0):
    """dict camera id -> (C, H, W) array: 'chw' contiguous, 'hwc' a transposed [H, W, C] array, 'sliced' every second
    channel of a [2C, H, W] buffer."""
    rs = np.random.RandomState(seed)
    maps = {}
    for cam in present:
        h, w = SHAPES[cam]
        if layout == "chw":
            m = rs.randn(channels, h, w).astype(dtype)
        elif layout == "hwc":
            m = rs.randn(h, w, channels).astype(dtype).transpose(2, 0, 1)
        else:
            m = rs.randn(2 * channels, h, w).astype(dtype)[1::2]
        assert m.shape == (channels, h, w)
        maps[cam] = m
    return maps


def make_rows(n, dtype=np.float64, form="stride15", order="range", n_outside=0, seed=1):
    """Raw lidar rows whose projection columns look like the parser's: names 0 (no projection), 1..5 and 6 (a camera
    past the table), fractional pixel values inside the named camera's map, neighbouring rows on neighbouring pixels
    ('range') or the same rows shuffled.  ``n_outside`` rows, spread over the whole array, get a first projection that
    the library must refuse.  Returns (rows, cp_col)."""
    rs = np.random.RandomState(seed)
    lidar = rs.randn(n, 15)
    i = np.arange(n)
    for k, col in enumerate((6, 9)):
        name = (i // (97 + 30 * k) + 2 * k) % 7  # runs of one camera, as a lidar sweep crosses the images
        name = np.where(rs.rand(n) < 0.1, rs.randint(0, 7, n), name)
        h = np.array([SHAPES[(c - 1) % 5][0] for c in name])
        w = np.array([SHAPES[(c - 1) % 5][1] for c in name])
        lidar[:, col] = name
        lidar[:, col + 1] = (i + 13 * k) % w + rs.rand(n) * 0.99
        lidar[:, col + 2] = (i // w + 7 * k) % h + rs.rand(n) * 0.99
    if n_outside:
        bad = np.linspace(0, n - 1, n_outside).astype(int)
        kinds = [(64.0, 1.0), (1.0, 40.0), (-1.0, 2.0), (np.nan, 3.0), (3e9, 0.0), (5.0, -np.inf), (2.0, -1.5)]
        for j, r in enumerate(bad):
            lidar[r, 6] = 1  # camera 0: 40 x 64
            lidar[r, 7], lidar[r, 8] = kinds[j % len(kinds)]
    if order == "shuffled":
        lidar = lidar[rs.permutation(n)]
    cp_col = 6
    if form == "copy12":
        lidar = np.ascontiguousarray(lidar[:, :12])
    elif form == "cp_col3":
        lidar = np.ascontiguousarray(lidar[:, 3:13])
        cp_col = 3
    return np.ascontiguousarray(lidar.astype(dtype)), cp_col


def want(rows, maps, cp_col, channels):
    features, cameras, outside = ref.query(rows, maps, cp_col)
    return ref.dense(features, cameras, rows.shape[0], channels) + (outside,)


def call_host(rows, maps, cp_col=6, channels=None):
    """The host entry on outputs pre-filled with NaN / -7; -> (dense, camera, count)."""
    from openseg3d_amd import _lib, ops
    table = ops.feature_map_table(maps, True, None, channels)
    n = rows.shape[0]
    out = np.full((n, table.channels), np.nan, dtype=np.float32)
    cam = np.full((n,), -7, dtype=np.int32)
    count = np.full((1,), -7, dtype=np.int32)
    _lib.call("seg3d_point_image_features_host", ctypes.byref(table), rows.ctypes.data, rows.itemsize, n,
              rows.strides[0] // rows.itemsize, cp_col, out.ctypes.data, cam.ctypes.data, count.ctypes.data)
    return out, cam, int(count[0])


def same(got, exp):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert np.array_equal(got[1], exp[1])
    assert got[0].tobytes() == exp[0].tobytes()  # NaN left behind, or a flipped bit, would differ
    assert got[2] == exp[2]


@pytest.mark.parametrize("map_dtype", [np.float32, np.float16])
@pytest.mark.parametrize("layout", ["chw", "hwc", "sliced"])
@pytest.mark.parametrize("form", ["stride15", "copy12", "cp_col3"])
@pytest.mark.parametrize("row_dtype", [np.float64, np.float32])
def test_twin_against_restatement(row_dtype, form, layout, map_dtype):
    maps = make_maps(28, map_dtype, layout, present=(0, 2, 3))  # cameras 1 and 4 absent: the second projection is used
    rows, cp_col = make_rows(1000, row_dtype, form, n_outside=9)
    exp = want(rows, maps, cp_col, 28)
    assert exp[2] == 9 and (exp[1] >= 0).sum() > 300 and (exp[1] == -1).sum() > 100
    same(call_host(rows, maps, cp_col), exp)
    view, _ = make_rows(1000, row_dtype, "stride15", n_outside=9)
    if form == "stride15":  # a [:, :12] VIEW of the raw file keeps the file's stride
        same(call_host(view[:, :12], maps, 6), exp)


@pytest.mark.parametrize("channels", [1, 8, 28, 64])
@pytest.mark.parametrize("n", [0, 1, 257])
def test_sizes(n, channels):
    from openseg3d_amd import ops
    maps = make_maps(channels, layout="chw" if channels != 8 else "hwc")
    rows, _ = make_rows(n, order="shuffled")
    exp = want(rows, maps, 6, channels)
    if n:
        same(call_host(rows, maps), exp)
    d, c = ops.point_image_features_host(rows, maps)
    assert d.shape == (n, channels) and c.shape == (n,) and np.array_equal(d, exp[0]) and np.array_equal(c, exp[1])


def _row(*six):
    r = np.zeros((1, 15))
    r[0, 6:12] = six
    return r


def test_camera_choice():
    maps = make_maps(8, present=(0, 2))
    m0, m2 = maps[0], maps[2]
    cases = [
        (_row(2, 3, 4, 3, 5, 6), 2, m2[:, 6, 5], 0),      # first camera absent -> second used
        (_row(1, 3, 4, 3, 5, 6), 0, m0[:, 4, 3], 0),      # both present -> first used
        (_row(1, 64, 4, 3, 5, 6), -1, None, 1),           # first present, pixel outside -> counted, second NOT tried
        (_row(0, 3, 4, 0, 5, 6), -1, None, 0),            # name 0: no projection
        (_row(0, 3, 4, 1, 5, 6), 0, m0[:, 6, 5], 0),
        (_row(6, 3, 4, 9, 5, 6), -1, None, 0),            # names beyond the table
        (_row(4, 3, 4, 3, 5, 6), 2, m2[:, 6, 5], 0),      # inside the table but absent
        (_row(-3, 3, 4, 3, 5, 6), 2, m2[:, 6, 5], 0),     # a negative name is no camera
        (_row(1, 3, 4, np.nan, np.nan, np.nan), 0, m0[:, 4, 3], 0),  # the second projection is never read
        (_row(np.nan, 3, 4, 3, 5, 6), -1, None, 1),       # a name the decision reads is no integer
        (_row(2, 3, 4, np.inf, 5, 6), -1, None, 1),
    ]
    for rows, cam, feat, outside in cases:
        d, c, k = call_host(rows, maps)
        same((d, c, k), want(rows, maps, 6, 8))
        assert c[0] == cam and k == outside
        assert np.array_equal(d[0], np.zeros(8, np.float32) if feat is None else feat)
    # a table shorter than the names: camera 2 is "beyond n_maps" for a one-entry sequence
    from openseg3d_amd import ops
    d, c = ops.point_image_features_host(_row(3, 1, 1, 1, 2, 2), [m0])
    assert c[0] == 0 and np.array_equal(d[0], m0[:, 2, 2])
    d, c = ops.point_image_features_host(_row(3, 1, 1, 2, 2, 2), [None, m0[:, :33, :50], None])
    assert c[0] == 1 and np.array_equal(d[0], m0[:, 2, 2])
    # all maps absent: legal, every row misses
    rows, _ = make_rows(50)
    for empty in ({}, [None, None, None]):
        d, c = ops.point_image_features_host(rows, empty, channels=5)
        assert d.shape == (50, 5) and not d.any() and (c == -1).all()
    d, c, k = call_host(rows, {}, channels=5)
    assert not d.any() and (c == -1).all() and k == 0


def test_pixel_values():
    from openseg3d_amd import _lib, ops
    maps = make_maps(8)
    m0 = maps[0]  # 40 x 64
    inside = [((7.9, 2.2), (7, 2)), ((-0.5, 3.0), (0, 3)), ((63.999, 39.5), (63, 39)), ((0.0, -0.99), (0, 0))]
    for dtype in (np.float64, np.float32):
        for (x, y), (ix, iy) in inside:
            rows = _row(1, x, y, 0, 0, 0).astype(dtype)
            d, c, k = call_host(rows, maps)
            assert c[0] == 0 and k == 0 and np.array_equal(d[0], m0[:, iy, ix]), (x, y)
            same((d, c, k), want(rows, maps, 6, 8))
        bad = [(64, 0), (0, 40), (-1, 0), (0, -1), (np.nan, 0), (0, np.nan), (3e9, 0), (0, -3e9), (np.inf, 0),
               (2.0 ** 31, 0), (-2.0 ** 31, 0)]
        rows = np.concatenate([_row(1, x, y, 2, 1, 1) for x, y in bad] + [_row(1, 5, 5, 0, 0, 0)]).astype(dtype)
        d, c, k = call_host(rows, maps)
        same((d, c, k), want(rows, maps, 6, 8))
        assert k == len(bad) and (c[:-1] == -1).all() and not d[:-1].any() and c[-1] == 0
        d, c, count = ops.point_image_features_host(rows, maps, check=False)  # zero rows, -1, the exact count
        assert not d[:-1].any() and (c[:-1] == -1).all() and count.dtype == np.int32 and int(count[0]) == len(bad)
        with pytest.raises(ops.ImageFeatureIndexError) as err:
            ops.point_image_features_host(rows, maps)
        assert isinstance(err.value, IndexError) and isinstance(err.value, _lib.Seg3dError)
    # the counter restarts: a clean call after a counted one
    assert call_host(_row(1, 5, 5, 0, 0, 0), maps)[2] == 0


def _table(n_maps=1, channels=8, elem_bytes=4, data=256, height=4, width=4, strides=(16, 4, 1)):
    from openseg3d_amd import ops
    t = ops.FeatureMapTable()
    t.n_maps, t.channels, t.elem_bytes = n_maps, channels, elem_bytes
    e = t.maps[0]
    e.data, e.height, e.width = data, height, width
    e.channel_stride, e.row_stride, e.col_stride = strides
    return t


def test_einval_before_anything_is_read():
    """Every refusal of the contract, on null or fake addresses (never read, never launched), host and device entry."""
    from openseg3d_amd import _lib
    lib, fake = _lib.load(), ctypes.c_void_p(256)
    host = lambda t, rows=fake, pb=8, n=10, stride=15, cp=6, out=fake, cam=fake, cnt=fake: \
        lib.seg3d_point_image_features_host(ctypes.byref(t) if t is not None else None, rows, pb, n, stride, cp, out, cam, cnt)
    dev = lambda t, rows=fake, pb=8, n=10, stride=15, cp=6, out=fake, cam=fake, cnt=fake: \
        lib.seg3d_point_image_features(ctypes.byref(t) if t is not None else None, rows, pb, n, stride, cp, out, cam, cnt, None)
    for f in (host, dev):
        assert f(None) == _lib.EINVAL
        for ch in (0, -1, 65):
            assert f(_table(channels=ch)) == _lib.EINVAL, ch
        for nm in (0, -1, 9):
            assert f(_table(n_maps=nm)) == _lib.EINVAL, nm
        for eb in (0, 1, 3, 8):
            assert f(_table(elem_bytes=eb)) == _lib.EINVAL, eb
        for pb in (0, 2, 16):
            assert f(_table(), pb=pb) == _lib.EINVAL, pb
        assert f(_table(), cp=-1) == _lib.EINVAL
        assert f(_table(), cp=10) == _lib.EINVAL  # cp_col + 6 > stride
        assert f(_table(), stride=5, cp=0) == _lib.EINVAL
        assert f(_table(), n=-1) == _lib.EINVAL
        assert f(_table(), n=2 ** 31) == _lib.EINVAL
        assert f(_table(height=0)) == _lib.EINVAL
        assert f(_table(width=0)) == _lib.EINVAL
        for bad in ((0, 4, 1), (16, 0, 1), (16, 4, 0), (-16, 4, 1)):
            assert f(_table(strides=bad)) == _lib.EINVAL, bad
        assert f(_table(), rows=None) == _lib.EINVAL
        assert f(_table(), out=None) == _lib.EINVAL
        assert f(_table(), cam=None) == _lib.EINVAL
        assert f(_table(), cnt=None) == _lib.EINVAL
        # legal and empty: n == 0 returns 0 with nothing behind the pointers, an absent map's fields are not looked at
        assert f(_table(), rows=None, n=0, out=None, cam=None, cnt=None) == 0
        assert f(_table(data=None, height=0, width=0, strides=(0, 0, 0)), rows=None, n=0, out=None, cam=None, cnt=None) == 0


def test_wrapper_refuses_bad_inputs():
    from openseg3d_amd import _lib, ops
    rows, _ = make_rows(10)
    maps = make_maps(8)
    for bad_rows in (rows.astype(np.int32), rows[0], rows[:, :11]):
        with pytest.raises(_lib.Seg3dError):
            ops.point_image_features_host(bad_rows, maps)
    with pytest.raises(_lib.Seg3dError):
        ops.point_image_features_host(rows, maps, cp_col=10)
    with pytest.raises(_lib.Seg3dError):
        ops.point_image_features_host(rows, {0: maps[0], 1: make_maps(4)[1]})  # two values of C
    with pytest.raises(_lib.Seg3dError):
        ops.point_image_features_host(rows, {0: maps[0], 1: maps[1].astype(np.float16)})
    with pytest.raises(_lib.Seg3dError):
        ops.point_image_features_host(rows, {8: maps[0]})
    with pytest.raises(_lib.Seg3dError):
        ops.point_image_features_host(rows, {})  # C unknown
    with pytest.raises(_lib.Seg3dError):
        ops.point_image_features_host(rows, {0: maps[0][:, ::-1]})
    import torch
    with pytest.raises(_lib.Seg3dError):  # the device entry takes CUDA tensors only
        ops.point_image_features(torch.from_numpy(rows), maps)


# ------------------------------------------------------------------------------------------ files
def test_dict_and_packed_forms(tmp_path):
    from openseg3d_amd import image_features as imf, ops
    maps = make_maps(8, present=(0, 1, 3))
    rows, _ = make_rows(300)
    features, cameras, _ = ref.query(rows, maps)
    dense, camera = ops.point_image_features_host(rows, maps)
    d = imf.to_dict(dense, camera)
    assert list(d) == list(features) and all(type(k) is int for k in d) and 50 < len(d) < 300
    for k in d:
        assert d[k].dtype == np.float32 and d[k].shape == (8,) and np.array_equal(d[k], features[k])
    prow, pfeat = imf.to_packed(dense, camera)
    assert prow.dtype == np.int32 and pfeat.dtype == np.float32 and prow.tolist() == list(features)
    assert np.array_equal(pfeat, np.stack(list(features.values())))
    # packed file: exactly two plain arrays, read back without a pickle
    path = imf.save_packed(str(tmp_path / "frame"), dense, camera)
    assert path.endswith("frame.npz")
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["feats", "rows"]
    import zipfile
    assert all(i.compress_type == zipfile.ZIP_STORED for i in zipfile.ZipFile(path).infolist())
    lrow, lfeat = imf.load(str(tmp_path / "frame"))
    assert np.array_equal(lrow, prow) and np.array_equal(lfeat, pfeat) and lrow.dtype == np.int32 and lfeat.dtype == np.float32
    # dict file: what np.save(feature_file, point_image_features) stores
    dpath = imf.save_dict(str(tmp_path / "other"), dense, camera)
    back = np.load(dpath, allow_pickle=True).item()
    assert list(back) == list(features) and all(np.array_equal(back[k], features[k]) and back[k].dtype == np.float32 for k in back)
    lrow, lfeat = imf.load(str(tmp_path / "other"))
    assert np.array_equal(lrow, prow) and np.array_equal(lfeat, pfeat)
    # both files: the packed one wins
    imf.save_packed(str(tmp_path / "other"), dense[:10], camera[:10])
    assert len(imf.load(str(tmp_path / "other"))[0]) == int((camera[:10] >= 0).sum())
    # an empty frame keeps its width
    prow, pfeat = imf.to_packed(np.zeros((4, 8), np.float32), np.full(4, -1, np.int32))
    assert prow.shape == (0,) and pfeat.shape == (0, 8) and imf.to_dict(pfeat, prow) == {}


def test_dataset_reads_packed_file(tmp_path):
    """One frame's dict file replaced by a packed one: the same arrays come back, without np.load unpickling."""
    from openseg3d_amd import image_features as imf
    from openseg3d_amd.dataset import WaymoDataset
    root = str(tmp_path / "waymo")
    names = fx.write(root, 0)
    ds = WaymoDataset(fx.make_cfg(True, False, True), root, "validation")
    name, other = names[1], names[3]
    n = np.load(os.path.join(root, "lidar", name + ".npy")).shape[0]
    rows0, feats0 = ds._raw_image_features(name)
    full0 = ds.load_image_features(n, name)
    dict_file = os.path.join(root, "image_feature", name + ".npy")
    dense = np.zeros((n, fx.DIM_IMAGE_FEATURE), np.float32)
    camera = np.full((n,), -1, np.int32)
    dense[rows0], camera[rows0] = feats0, 0
    imf.save_packed(os.path.join(root, "image_feature", name), dense, camera)
    rows_both, _ = ds._raw_image_features(name)  # both files present
    os.remove(dict_file)
    real_load = np.load

    def no_pickle(path, *a, **kw):
        assert not kw.get("allow_pickle", False), path
        return real_load(path, *a, **kw)

    np.load = no_pickle
    try:
        rows1, feats1 = ds._raw_image_features(name)
        full1 = ds.load_image_features(n, name)
    finally:
        np.load = real_load
    assert rows1.dtype == rows0.dtype == np.int32 and feats1.dtype == feats0.dtype == np.float32
    assert np.array_equal(rows1, rows0) and np.array_equal(feats1, feats0) and np.array_equal(rows_both, rows0)
    assert full1.dtype == np.float32 and np.array_equal(full1, full0) and full0.any()
    # a frame with only the dict file goes through the old branch
    d = np.load(os.path.join(root, "image_feature", other + ".npy"), allow_pickle=True).item()
    rows2, feats2 = ds._raw_image_features(other)
    assert rows2.tolist() == list(d) and np.array_equal(feats2, np.stack(list(d.values())))
    # the whole sample is the same from either file
    a = ds[ds.filenames.index(name)]["point_image_features"]
    assert np.array_equal(a[:n], full0)
    shutil.rmtree(root)
