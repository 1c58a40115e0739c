"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol the header
declares, the product package never reaches into oracle/, and the ops refuse to run without a GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from openseg3d_amd import _lib
    declared = _lib.header_symbols()
    assert len(declared) >= 25
    assert sorted(_lib.SIGNATURES) == declared, "binding table and include/seg3d_hip.h disagree"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in seg3d_hip.h but not exported"
    assert _lib.load().seg3d_abi_version() == _lib.ABI_VERSION


def test_header_cites_reference_interfaces():
    text = open(os.path.join(ROOT, "include", "seg3d_hip.h")).read()
    for cite in ("voxel_generator.py:55-153", "ingroup_inds_cuda.cu:12-25", "spconv_utils.py:13-32",
                 "swformer_utils.py", "cosine_msa.py:115-177", "voxel_pooling_cuda.cu:10-79", "voxel_to_point.py:4-17"):
        assert cite in text, cite


def test_product_package_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "openseg3d_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                continue
            src = open(os.path.join(dirpath, f)).read()
            uses = re.findall(r"^\s*(?:from|import)\s+oracle\b.*$", src, flags=re.M)
            if f == "selfcheck.py":  # smoke()'s checker, allowed by the rules
                continue
            assert not uses, f"{f} imports the oracle: {uses}"
            assert "/root/reference" not in src, f"{f} reads the reference tree at run time"


def test_ops_fail_loudly_without_gpu():
    from openseg3d_amd import _lib, ops
    x = torch.zeros(4, 6)
    with pytest.raises(_lib.Seg3dError):
        ops.voxelize(x, [0.1, 0.1, 0.1], [-72, -72, -2, 72, 72, 4.4])
    with pytest.raises(_lib.Seg3dError):
        ops.voxel_to_point(torch.zeros(3, 4), torch.zeros(5, dtype=torch.long))
    with pytest.raises(_lib.Seg3dError):
        ops.get_inner_win_inds(torch.zeros(5, dtype=torch.long))


def test_host_only_entry_points():
    from openseg3d_amd import _lib, ops
    assert ops.grid_size([0.1, 0.1, 0.1], [-72, -72, -2, 72, 72, 4.4]) == [1440, 1440, 64]
    assert ops.grid_size([0.05, 0.012, 0.1], [0, -3.1415926, -2, 75.2, 3.1415926, 5.2]) == [1504, 524, 72]
    assert _lib.query("seg3d_voxelize_workspace_bytes", 180000) > 180000 * 12
    assert _lib.query("seg3d_coord_hash_bytes", 1000) == 2048 * 12
    # argument validation happens before anything is enqueued: a null call is rejected, not launched
    assert _lib.load().seg3d_spconv_fwd(None, None, 10, 10, None, 0, None, 48, 48, None, None, None) == _lib.EINVAL
    assert _lib.load().seg3d_spconv_fwd(None, None, 10, 10, None, 4, None, 50, 48, None, None, None) == _lib.EINVAL
    # the six-product Linear (csrc/linear_x6.hip) takes cin % 32 == 0 and cout % 64 == 0 and says so through its size query;
    # three planes of 8-element fragments per (32-channel step, 16-column tile)
    assert _lib.query("seg3d_linear_packed_bytes_x6", 128, 256) == (128 // 32) * (256 // 64) * 4 * 3 * 64 * 16 == 128 * 256 * 6
    assert _lib.query("seg3d_linear_packed_bytes_x6", 96, 256) == 96 * 256 * 6
    for cin, cout in ((48, 64), (64, 96), (6, 64), (64, 22), (0, 64)):
        assert _lib.query("seg3d_linear_packed_bytes_x6", cin, cout) == 0
    assert _lib.load().seg3d_linear_fwd_x6(None, 10, None, None, None, None, 0, 128, 256, None, None) == _lib.EINVAL
    assert _lib.load().seg3d_linear_fwd_x6(None, 0, None, None, None, None, 0, 128, 256, None, None) == 0  # nothing to do
    # the window-attention schedule query (host arithmetic of the launchers, no launch): null output, unsupported head
    # geometries, more chunks than tiles and a dropout rate outside [0, 1) are refused; an empty index has an empty grid
    sched = (ctypes.c_int32 * 6)(*([-7] * 6))
    lib = _lib.load()
    assert lib.seg3d_window_attn_schedule(59, 23, 8, 12, 0.0, None) == _lib.EINVAL
    for heads, dh in ((3, 12), (6, 6), (12, 6), (8, 32), (17, 24), (0, 24), (20, 6)):
        assert lib.seg3d_window_attn_schedule(59, 23, heads, dh, 0.0, sched) == _lib.EINVAL, (heads, dh)
    assert lib.seg3d_window_attn_schedule(23, 59, 8, 12, 0.0, sched) == _lib.EINVAL
    assert lib.seg3d_window_attn_schedule(-1, -1, 8, 12, 0.0, sched) == _lib.EINVAL
    assert lib.seg3d_window_attn_schedule(59, 23, 8, 12, 1.0, sched) == _lib.EINVAL
    assert list(sched) == [-7] * 6  # a refused call writes nothing
    assert lib.seg3d_window_attn_schedule(0, 0, 8, 24, 0.0, sched) == 0
    assert sched[0] == 0 and sched[1] > 0 and list(sched)[2:4] == [0, 0] and sched[5] == 0
    # 59 tiles x 2 groups of 4 heads: fewer units than any cap, grid = units rounded up to the 8 XCD groups (exact values: the
    # A/B switches SEG3D_ATTN_XCD, SEG3D_ATTN_XCD_BLOCK and SEG3D_ATTN_WGS_PER_CU must be unset, as in every test run)
    assert lib.seg3d_window_attn_schedule(59, 23, 8, 12, 0.0, sched) == 0
    cap = sched[1]
    assert cap >= 120 and list(sched) == [0, cap, 120, 2, 8, 128]
    # as many items as the cap, 8 heads each: eight rounds of the full grid
    assert lib.seg3d_window_attn_schedule(cap, cap, 8, 48, 0.0, sched) == 0 and sched[3] >= 8 and sched[2] == sched[1]
    # the weight-gradient kernel fits the workspace the query reports
    assert _lib.query("seg3d_linear_wgrad_workspace_bytes", 58453, 192, 192) >= 8 * (192 * 192 + 192) * 4
    # weight-gradient argument checks: every case below returns before a launch (the non-null addresses are never read)
    lib, fake, chunks = _lib.load(), ctypes.c_void_p(256), ctypes.c_int32(7)
    big = 1 << 40
    for name in ("seg3d_spconv_wgrad_partials", "seg3d_spconv_wgrad_partials_xbf16"):
        f = getattr(lib, name)
        for cin, cout in ((24, 32), (32, 40), (8, 16), (0, 16)):
            assert f(fake, fake, fake, 100, 100, cin, cout, fake, big, ctypes.byref(chunks), None) == _lib.EINVAL, (name, cin, cout)
        chunks.value = 7
        assert f(None, None, None, 0, 0, 32, 32, None, 0, ctypes.byref(chunks), None) == 0 and chunks.value == 0, name
        need = _lib.query("seg3d_spconv_wgrad_workspace_bytes", 1000, 32, 64)
        assert need >= 27 * 32 * 64 * 4
        assert f(fake, fake, fake, 1000, 1000, 32, 64, fake, need - 4, ctypes.byref(chunks), None) == _lib.EINVAL, name
        assert f(fake, fake, fake, 1000, 1000, 32, 64, None, need, ctypes.byref(chunks), None) == _lib.EINVAL, name
    assert lib.seg3d_spconv_wgrad(fake, fake, fake, 100, 100, 24, 32, 4, fake, fake, big, None) == _lib.EINVAL
    need = _lib.query("seg3d_spconv_wgrad_workspace_bytes", 1000, 48, 48)
    assert lib.seg3d_spconv_wgrad(fake, fake, fake, 1000, 1000, 48, 48, 4, fake, fake, need - 4, None) == _lib.EINVAL
    for name in ("seg3d_linear_wgrad_partials", "seg3d_linear_wgrad_partials_xbf16"):
        f = getattr(lib, name)
        for cin, cout in ((6, 64), (64, 22), (0, 16)):
            assert f(fake, fake, 100, cin, cout, 1, fake, big, ctypes.byref(chunks), None) == _lib.EINVAL, (name, cin, cout)
        chunks.value = 7
        need0 = _lib.query("seg3d_linear_wgrad_workspace_bytes", 0, 12, 40)
        assert f(None, None, 0, 12, 40, 1, None, need0, ctypes.byref(chunks), None) == 0 and chunks.value == 0, name
        need = _lib.query("seg3d_linear_wgrad_workspace_bytes", 70001, 12, 40)
        assert need >= 8 * (12 * 40 + 40) * 4
        assert f(fake, fake, 70001, 12, 40, 1, fake, need - 4, ctypes.byref(chunks), None) == _lib.EINVAL, name
    assert lib.seg3d_linear_wgrad(fake, fake, 100, 6, 64, fake, None, fake, big, None) == _lib.EINVAL


@pytest.mark.parametrize("tag,rng,vs", [("cart", [-72, -72, -2, 72, 72, 4.4], [0.1, 0.1, 0.1]),
                                        ("cyl", [0, -3.1415926, -2, 75.2, 3.1415926, 5.2], [0.05, 0.012, 0.1])])
@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_host_voxelizer_bit_exact_vs_reference(tag, rng, vs, dt):
    """VoxelGenerator.generate runs in DataLoader workers and TTA without a GPU context, so the CPU entry
    "must stay".  The library's own host entry (seg3d_voxelize_host_f32 / _f64, plain C++ in libseg3d_hip.so, no import of
    oracle/) against the outputs of the reference's points_to_voxel (tests/golden/voxelize.npz): coordinates in first-seen
    order and point -> voxel ids bit for bit, float32 and float64 rows, cartesian and cylinder grids."""
    import numpy as np
    from openseg3d_amd import batch, ops
    d = np.load(os.path.join(ROOT, "tests", "golden", "voxelize.npz"))
    k = f"{tag}_{dt}"
    pts = d[k + "_points"]
    gen = batch.VoxelGenerator(vs, rng)
    coors, ids = gen.generate(pts)  # numpy in -> the host entry, numpy out (voxel_generator.py:24-26)
    assert isinstance(coors, np.ndarray) and coors.dtype == np.int32 and ids.dtype == np.int32
    assert np.array_equal(coors, d[k + "_coors"]) and np.array_equal(ids, d[k + "_ids"])
    assert gen.grid_size.tolist() == d[tag + "_grid"].tolist()
    # collated form: a batch column in front, the same sample twice -> the second copy's voxels are new rows of batch 1
    rows = np.concatenate([np.pad(pts, ((0, 0), (1, 0)), constant_values=b) for b in (0.0, 1.0)])
    c4, i2 = ops.voxelize_host(rows, vs, rng, xyz_col=1, batch_col=0)
    m, n = coors.shape[0], pts.shape[0]
    assert np.array_equal(c4[:m, 1:], coors) and (c4[:m, 0] == 0).all() and np.array_equal(c4[m:, 1:], coors) and (c4[m:, 0] == 1).all()
    assert np.array_equal(i2[:n], ids) and np.array_equal(i2[n:], np.where(ids >= 0, ids + m, -1))


def test_host_voxelizer_edge_cases():
    import numpy as np
    from openseg3d_amd import _lib, ops
    vs, rng = [0.1, 0.1, 0.1], [-72, -72, -2, 72, 72, 4.4]
    c, i = ops.voxelize_host(np.zeros((0, 6), np.float32), vs, rng)
    assert c.shape == (0, 4) and i.shape == (0,)
    p = np.array([[0, 0, 0, 0, 0, 0], [1e6, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0.05, 0.05, 0.05, 0, 0, 0],
                  [np.nan, 0, 0, 0, 0, 0], [72.0, 0, 0, 0, 0, 0], [-72.0, -72.0, -2.0, 0, 0, 0]], np.float32)
    c, i = ops.voxelize_host(p, vs, rng)
    assert i.tolist() == [0, -1, 0, 0, -1, -1, 1] and c.tolist() == [[0, 20, 720, 720], [0, 0, 0, 0]]
    with pytest.raises(_lib.Seg3dError):
        ops.voxelize_host(np.zeros((4, 6), np.int32), vs, rng)
    with pytest.raises(_lib.Seg3dError):  # a workspace that is too small is refused, not overrun
        ws = np.empty((64,), np.uint8)
        cnt = np.zeros((1,), np.int32)
        out_c, out_i = np.empty((7, 4), np.int32), np.empty((7,), np.int32)
        F3, F6 = ctypes.c_float * 3, ctypes.c_float * 6
        _lib.call("seg3d_voxelize_host_f32", p.ctypes.data, 7, 6, 0, -1, F3(*vs), F6(*rng), out_c.ctypes.data, out_i.ctypes.data,
                  cnt.ctypes.data, ws.ctypes.data, ws.size)
