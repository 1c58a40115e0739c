"""The integer structures every kernel walks -- voxel list, coordinate hash, the three neighbour tables, chained coarse site
lists, window CSR and attention work items -- over their accepted range, on the device, against the oracle, the host
voxelizer and the plain references of tests/index_cases.py (which tests/test_index_range_host.py checks without a GPU).
Every comparison is exact but the positional embedding's.  All inputs are inside the documented contract."""
import numpy as np
import pytest
import torch

import index_cases as ic
import refcfg

pytestmark = pytest.mark.gpu

VOXEL_CASE_NAMES = list(ic.voxel_cases("float32"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from openseg3d_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------ A: voxelizer
@pytest.mark.parametrize("dt", ic.DTYPES)
@pytest.mark.parametrize("name", VOXEL_CASE_NAMES)
def test_voxelizer_device_equals_host_twin_and_reference(dev, name, dt):
    """Cell edges, non-finite coordinates (id -1, no voxel, the rest as if those rows were deleted), run and contention
    patterns of the wave-ballot head logic, row layouts and keys beyond 2^32: device == host twin == plain loop (== oracle
    where the case is one sample)."""
    from oracle import index_ops
    from openseg3d_amd import ops
    case = ic.voxel_cases(dt)[name]
    want_coords, want_ids = ic.voxel_expected(name, dt)
    coords, ids = ops.voxelize(torch.from_numpy(case["points"]).to(dev), case["voxel"], case["range"], case["xyz_col"],
                               case["batch_col"])
    host_coords, host_ids = ops.voxelize_host(case["points"], case["voxel"], case["range"], case["xyz_col"], case["batch_col"])
    assert coords.dtype == torch.int32 and ids.dtype == torch.int32
    assert np.array_equal(_np(ids), want_ids)
    assert np.array_equal(_np(coords), want_coords)
    assert np.array_equal(_np(ids), host_ids) and np.array_equal(_np(coords), host_coords)
    if ic.is_single_sample(case):
        oc, oi = index_ops.voxelize(case["points"], case["voxel"], case["range"])
        assert np.array_equal(_np(ids), oi) and np.array_equal(_np(coords)[:, 1:], oc)


# ------------------------------------------------------------------------------------------ B: site structures
def _check_tables(dev, coords, shape, batch):
    """Hash, submanifold table, coarse sites, strided and inverse tables and parity order of one site list vs the oracle."""
    from oracle import sparse_conv as sc
    from openseg3d_amd import ops
    m = coords.shape[0]
    ref = sc.Sites(coords, shape)
    c = torch.from_numpy(coords).to(dev)
    h = ops.CoordHash(c, shape)
    nbr = _np(ops.rulebook_subm(h))
    assert nbr.shape == (27, m) and np.array_equal(nbr, ref.subm())
    assert np.array_equal(_np(ops.parity_order(c)), ic.parity_ref(coords))
    rc, rf, ri = ref.down()
    co, shape_out = ops.downsample_coords(c, batch, shape)
    assert shape_out == rc.shape.tolist()
    assert np.array_equal(_np(co), rc.coords)
    fwd, inv = ops.rulebook_strided(h, co)
    fwd, inv = _np(fwd), _np(inv)
    assert fwd.shape == (27, rc.coords.shape[0]) and inv.shape == (27, m)
    assert np.array_equal(fwd, rf)
    assert np.array_equal(inv, ri)
    for k in range(27):  # the two tables are transposes of each other, at every offset
        o = np.nonzero(fwd[k] >= 0)[0]
        assert np.array_equal(inv[k][fwd[k][o]], o)
        i = np.nonzero(inv[k] >= 0)[0]
        assert np.array_equal(fwd[k][inv[k][i]], i)
    return nbr, _np(co)


@pytest.mark.parametrize("name", list(ic.site_cases()))
def test_site_tables_match_oracle(dev, name):
    """Odd and even dims, full occupancy and the eight corners, batch 3 with bitmap words that straddle samples, rows in
    random order, 0 / 1 / 255 / 256 / 257 / 2049 rows, and a block of 8191 sites (hash load 0.49994, longest probe chains)."""
    coords, shape, batch = ic.site_cases()[name]
    nbr, coarse = _check_tables(dev, coords, shape, batch)
    if name == "rows_0":
        assert nbr.shape == (27, 0) and coarse.shape == (0, 4)
    if name == "rows_1":
        assert nbr[13, 0] == 0 and (np.delete(nbr[:, 0], 13) == -1).all()


def test_hash_keys_beyond_2_32(dev):
    """128 x 8192 x 8192 sites whose keys exceed 2^32 and alias under 32-bit truncation: the submanifold table against a
    dict lookup (no downsampling at this shape: its bitmap is dense)."""
    from openseg3d_amd import ops
    coords, shape, _ = ic.big_key_sites()
    h = ops.CoordHash(torch.from_numpy(coords).to(dev), shape)
    assert np.array_equal(_np(ops.rulebook_subm(h)), ic.subm_dict(coords, shape))


@pytest.mark.parametrize("count", ic.STALE_COUNTS)
def test_downsample_ignores_rows_behind_the_device_count(dev, count):
    """downsample_launch(rows_dev=count): the buffer's rows behind `count` are valid sites that would add output sites."""
    from oracle import index_ops
    from openseg3d_amd import ops
    buf, shape, batch = ic.stale_tail_buffer()
    rows = torch.tensor([count], dtype=torch.int32, device=dev)
    out, n, shape_out = ops.downsample_launch(torch.from_numpy(buf).to(dev), batch, shape, rows_dev=rows)
    want, want_shape = index_ops.downsample_coords(buf[:count], shape)
    assert shape_out == want_shape.tolist() and int(n.item()) == want.shape[0]
    assert np.array_equal(_np(out)[:want.shape[0]], want)


@pytest.mark.parametrize("batch", [1, 3])
def test_downsample_chain_matches_three_oracle_levels(dev, batch):
    from oracle import sparse_conv as sc
    from openseg3d_amd import ops
    shape = [13, 22, 19]
    coords = ic.random_sites(shape, batch, 500 * batch, 50 + batch)
    ref = sc.Sites(coords, shape)
    levels = ops.downsample_chain(torch.from_numpy(coords).to(dev), batch, shape, 3)
    assert len(levels) == 3
    for got, got_shape in levels:
        ref = ref.down()[0]
        assert got_shape == ref.shape.tolist() and np.array_equal(_np(got), ref.coords)


# ------------------------------------------------------------------------------------------ C: window partition
def _partition(dev, coords, batch, window, nwin, shift, info):
    from openseg3d_amd import ops
    wi = ops.window_partition(torch.from_numpy(coords).to(dev), batch, window, nwin, shift, ic.levels_of(info), want_debug=True)
    wi.n_windows, wi.n_dropped, wi.n_tiles, wi.n_qgroups = (int(v) for v in wi.counts.tolist())
    return wi


def _check_partition(wi, win, in_win, info):
    """Ids, levels, slots vs the oracle; CSR, work items and counts vs the closed form; counts fit the buffers."""
    rank, level, slot = ic.levels_ref(win, info)
    m = win.shape[0]
    assert np.array_equal(_np(wi.win_id), win)
    if in_win is not None:
        assert np.array_equal(_np(wi.in_win), in_win)
    assert np.array_equal(_np(wi.rank), rank)
    assert np.array_equal(_np(wi.level), level)
    assert np.array_equal(_np(wi.slot), slot)
    want = ic.window_expect(win)
    assert (wi.n_windows, wi.n_dropped, wi.n_tiles, wi.n_qgroups) == (want["n_windows"], int((slot == -1).sum()),
                                                                      want["n_tiles"], want["n_qgroups"])
    assert wi.n_windows <= wi.win_start.shape[0] == wi.win_count.shape[0] == wi.win_tile0.shape[0]
    assert wi.n_tiles <= wi.tile_item.shape[0] and wi.n_qgroups <= wi.qg_item.shape[0] and m <= wi.tok.shape[0]
    assert np.array_equal(_np(wi.tok)[:m], want["tok"])
    for k in ("win_start", "win_count", "win_tile0"):
        assert np.array_equal(_np(getattr(wi, k))[:wi.n_windows], want[k]), k
    assert np.array_equal(_np(wi.tile_item)[:wi.n_tiles], want["tile_item"])
    assert np.array_equal(_np(wi.qg_item)[:wi.n_qgroups], want["qg_item"])


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("do_shift", [False, True])
@pytest.mark.parametrize("gi", [0, 1, 2], ids=["multiple", "ragged", "sz_eq_wz"])
@pytest.mark.parametrize("wi_", [0, 1, 2], ids=["win10x10x8", "win2x3x2", "win5x7x3"])
def test_window_geometry(dev, wi_, gi, do_shift, batch):
    """Even and odd window dims, both shifts, grids that are / are not multiples of the window, voxels at coordinate 0 and
    at the largest coordinate (the "+1" window when unshifted), and the sz == wz rule (no z shift)."""
    from openseg3d_amd.swformer import window_geometry
    window, grid = ic.WINDOW_SHAPES[wi_], ic.GEOMETRY_GRIDS[wi_][gi]
    coords = ic.geometry_coords(grid, batch, 100 * wi_ + gi)
    win, in_win = ic.window_ids_ref(coords, grid, window, do_shift)
    w, nwin, shift = window_geometry(grid, window, do_shift)
    info = refcfg.BATCHING_INFO[0]
    _check_partition(_partition(dev, coords, batch, w, nwin, shift, info), win, in_win, info)


def _occupancy_case(do_shift):
    from openseg3d_amd.swformer import window_geometry
    window = [10, 10, 8]
    coords, sparse = ic.occupancy_coords(window, do_shift, [ic.OCCUPANCIES, ic.OCCUPANCIES[::-1]])
    win, in_win = ic.window_ids_ref(coords, sparse, window, do_shift)
    return coords, win, in_win, window_geometry(sparse, window, do_shift)


LEVEL_CASES = [f"reference_stage{s}" for s in range(4)] + list(ic.LEVEL_TABLES)


@pytest.mark.parametrize("do_shift", [False, True])
@pytest.mark.parametrize("table", LEVEL_CASES)
def test_window_occupancies_and_levels(dev, table, do_shift):
    """Windows of exactly 1, 31, 32, 33, 127, 128, 129, 257 and 800 tokens, separated by empty and one-token windows, under
    the reference's four-level tables, one level, overlapping ranges (the later level wins), counts at a range's lo, hi - 1
    and hi, and at the op level an occupancy above max_tokens (ranks at or above the cap: slot -1, counted; other slots
    unchanged) and, with four levels, occupancies that match no range (level -1, slot -1; the level-3 windows' slots are
    rank_among_level3_windows * cap + rank)."""
    info = refcfg.BATCHING_INFO[int(table[-1])] if table.startswith("reference_stage") else ic.LEVEL_TABLES[table]
    coords, win, in_win, (w, nwin, shift) = _occupancy_case(do_shift)
    wi = _partition(dev, coords, 2, w, nwin, shift, info)
    _check_partition(wi, win, in_win, info)
    if table == "unmatched":
        level, slot, rank = _np(wi.level), _np(wi.slot), _np(wi.rank)
        l3 = np.unique(win[level == 3])
        assert l3.shape[0] == 4 and (slot[level == -1] == -1).all() and (level == -1).sum() == 2 * (128 + 129)
        assert np.array_equal(slot[level == 3], np.searchsorted(l3, win[level == 3]) * 800 + rank[level == 3])
    if table == "over_cap":
        assert wi.n_dropped == 2 * (27 + 28 + 29 + 157 + 700)


@pytest.mark.parametrize("n_canvas", ic.CANVAS_SIZES)
def test_window_canvas_sizes_around_the_scan_edges(dev, n_canvas):
    """The four-lane scan over 2047, 2048, 2049, 524289 and 526337 canvas entries (one chunk short by one, one chunk, one
    chunk plus one, 256 chunks plus one, 257 chunks plus one): voxels in the first and the last entry and on both sides
    of every 2048 boundary, 1 .. 4 per window so that every level lane and the tile lanes carry sums."""
    coords, entry = ic.canvas_coords(n_canvas)
    wi = _partition(dev, coords, 1, ic.CANVAS_WINDOW, [1, 1, n_canvas], [0, 0, 0], ic.CANVAS_INFO)
    _check_partition(wi, entry, None, ic.CANVAS_INFO)
    assert np.array_equal(_np(wi.in_win), np.stack([coords[:, 1] % 4, coords[:, 2], coords[:, 3]], axis=1))


@pytest.mark.parametrize("c", [48, 96, 192])
@pytest.mark.parametrize("window", ic.WINDOW_SHAPES, ids=["win10x10x8", "win2x3x2", "win5x7x3"])
def test_pos_embed_every_in_window_coordinate(dev, window, c):
    """sin/cos of libm vs device: <= 2 ulp of values in [-1, 1], the 5e-7 of test_window_partition_bit_exact_vs_reference."""
    from oracle import window as owin
    from openseg3d_amd import ops
    from openseg3d_amd.swformer import SparseWindowPartitionLayer
    in_win = ic.all_in_window(window)
    layer = SparseWindowPartitionLayer(refcfg.BATCHING_INFO[0], window, [40.0, 40.0, 16.0])
    pos = ops.pos_embed(torch.from_numpy(in_win).to(dev), window, layer.inv_freq(c, dev), c)
    want = owin.pos_embed_flat(torch.from_numpy(in_win).long(), window, c)
    assert pos.shape == want.shape and pos.dtype == torch.float32
    assert float((pos.cpu() - want).abs().max()) <= 5e-7


@pytest.mark.parametrize("c", [50, 64, 9, 45, 51])
def test_pos_embed_refuses_bad_channel_counts(dev, c):
    """c not divisible by 3, or c / 3 odd."""
    from openseg3d_amd import _lib, ops
    in_win = torch.from_numpy(ic.all_in_window([2, 3, 2])).to(dev)
    with pytest.raises(_lib.Seg3dError):
        ops.pos_embed(in_win, [2, 3, 2], torch.ones((64,), device=dev), c)
