"""The integer structures over their accepted range, the part that needs no GPU: the host voxelizer
(seg3d_voxelize_host_f32 / _f64) against the oracle and a plain first-seen loop on every case of tests/index_cases.py, and
the references that tests/test_gpu_index_range.py holds the device to -- the dict-lookup neighbour table, the parity order
and the closed form of the window CSR and work items -- against the oracle or a plain loop.  All comparisons are exact."""
import numpy as np
import pytest
import torch

import index_cases as ic
import refcfg

VOXEL_CASE_NAMES = list(ic.voxel_cases("float32"))


# ------------------------------------------------------------------------------------------ A: voxelizer
@pytest.mark.parametrize("dt", ic.DTYPES)
@pytest.mark.parametrize("name", VOXEL_CASE_NAMES)
def test_host_voxelizer_matches_loop_and_oracle(name, dt):
    from oracle import index_ops
    from openseg3d_amd import ops
    case = ic.voxel_cases(dt)[name]
    want_coords, want_ids = ic.voxel_expected(name, dt)
    coords, ids = ops.voxelize_host(case["points"], case["voxel"], case["range"], case["xyz_col"], case["batch_col"])
    assert coords.dtype == np.int32 and ids.dtype == np.int32
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(coords, want_coords)
    if ic.is_single_sample(case):
        oc, oi = index_ops.voxelize(case["points"], case["voxel"], case["range"])
        assert np.array_equal(oi, want_ids)
        assert np.array_equal(oc, want_coords[:, 1:]) and not want_coords[:, 0].any()


def test_edge_case_separates_float64_from_float32():
    """Some float64 edge points round, as float32, into another cell: the f64 entry must follow the f64 reference."""
    from openseg3d_amd import ops
    c64 = ic.voxel_cases("float64")["edges"]
    _, ids64 = ic.voxel_expected("edges", "float64")
    c32, ids32 = ic.voxelize_loop(c64["points"].astype(np.float32), c64["voxel"], c64["range"])
    coords64, _ = ic.voxel_expected("edges", "float64")
    cell64 = np.where(ids64[:, None] >= 0, coords64[np.maximum(ids64, 0)], -1)
    cell32 = np.where(ids32[:, None] >= 0, c32[np.maximum(ids32, 0)], -1)
    assert int((cell64 != cell32).any(axis=1).sum()) >= 20
    # both sides of every cell edge are hit: each cell of each axis is occupied and points fall outside at both ends
    assert set(coords64[:, 3]) == set(range(32)) and set(coords64[:, 2]) == set(range(16)) and set(coords64[:, 1]) == set(range(8))
    assert (ids64 == -1).sum() > 10
    assert np.array_equal(ops.voxelize_host(c64["points"], c64["voxel"], c64["range"])[1], ids64)


@pytest.mark.parametrize("dt", ic.DTYPES)
def test_nonfinite_case_expectation(dt):
    """Non-finite rows get -1 and leave the rest as if they were deleted (what voxel_expected states), whole rows too."""
    pts = ic.voxel_cases(dt)["nonfinite"]["points"]
    bad = ~np.isfinite(pts).all(axis=1)
    coords, ids = ic.voxel_expected("nonfinite", dt)
    assert bad.sum() == 12 and (ids[bad] == -1).all() and (ids[~bad] >= 0).all()
    assert all(np.isnan(pts[:, c]).any() and np.isposinf(pts[:, c]).any() and np.isneginf(pts[:, c]).any() for c in range(3))
    c2, i2 = ic.voxelize_loop(pts, ic.SMALL_VOXEL, ic.SMALL_RANGE)  # the loop itself rejects them: same answer
    assert np.array_equal(c2, coords) and np.array_equal(i2, ids)


def test_pattern_cases_are_what_they_claim():
    for n in ic.PATTERN_SIZES:
        assert ic.voxel_expected(f"one_cell_{n}", "float32")[0].shape[0] == 1
        assert ic.voxel_expected(f"own_cell_{n}", "float32")[0].shape[0] == n
        assert np.array_equal(ic.voxel_expected(f"alternating_{n}", "float32")[1], np.arange(n) % 2 if n > 1 else [0])
    coords, ids = ic.voxel_expected("runs_rejected", "float32")
    assert coords.shape[0] == 97 and (ids == -1).sum() == 129
    coords, ids = ic.voxel_expected("keys_beyond_2_32", "float32")
    assert coords.shape[0] == 72 and set(coords[:, 0]) == {0, 1, 2} and coords[:, 1].max() >= 64
    ids = ic.voxel_expected("layout_s4_x1_b0", "float64")
    assert set(ids[0][:, 0]) == {0, 2, 3}  # the sample in the middle is empty


# ------------------------------------------------------------------------------------------ B: site structures
@pytest.mark.parametrize("name", [n for n, c in ic.site_cases().items() if c[0].shape[0] <= 600])
def test_site_references_agree_with_oracle(name):
    from oracle import sparse_conv as sc
    coords, shape, batch = ic.site_cases()[name]
    m = coords.shape[0]
    assert np.unique(coords, axis=0).shape[0] == m  # distinct sites, inside the shape, batch ids in range
    assert m == 0 or ((coords >= 0).all() and (coords[:, 1:] < np.array(shape)).all() and coords[:, 0].max() < batch)
    ref = sc.Sites(coords, shape)
    assert np.array_equal(ic.subm_dict(coords, shape), ref.subm())
    coarse, fwd, inv = ref.down()
    assert coarse.shape.tolist() == [(s - 1) // 2 + 1 for s in shape]
    for k in range(27):  # the transpose identity the device tables are held to
        o = np.nonzero(fwd[k] >= 0)[0]
        assert np.array_equal(inv[k][fwd[k][o]], o)
        assert (fwd[k] >= 0).sum() == (inv[k] >= 0).sum()
    order = ic.parity_ref(coords)
    key = (coords[:, 1] & 1) * 4 + (coords[:, 2] & 1) * 2 + (coords[:, 3] & 1)
    assert np.array_equal(np.sort(order), np.arange(m)) and (np.diff(key[order]) >= 0).all()
    assert all((np.diff(order[key[order] == g]) > 0).all() for g in range(8))


def test_site_case_properties():
    from oracle import sparse_conv as sc
    cases = ic.site_cases()
    assert [cases[f"rows_{m}"][0].shape[0] for m in ic.ROW_COUNTS] == ic.ROW_COUNTS
    nbr = sc.Sites(*cases["rows_1"][:2]).subm()
    assert nbr[13, 0] == 0 and (np.delete(nbr[:, 0], 13) == -1).all()
    assert cases["corners_8x11x8"][0].shape[0] == 8 and cases["corners_1x1x2"][0].shape[0] == 2
    assert (4 * 3 * 3) % 32 != 0  # coarse cells per sample of [7, 6, 5]
    coords, shape, _ = ic.big_key_sites()
    table = ic.subm_dict(coords, shape)
    assert np.array_equal(table, sc.Sites(coords, shape).subm()) and (np.delete(table, 13, axis=0) >= 0).sum() >= 20


def test_stale_tail_rows_would_add_sites():
    from oracle import index_ops
    buf, shape, _ = ic.stale_tail_buffer()
    whole = index_ops.downsample_coords(buf, shape)[0].shape[0]
    for count in ic.STALE_COUNTS:
        assert index_ops.downsample_coords(buf[:count], shape)[0].shape[0] < whole


# ------------------------------------------------------------------------------------------ C: window partition
def _window_expect_loop(win):
    """window_expect by a plain loop over the windows."""
    ids = sorted(set(int(w) for w in win))
    out = dict(tok=[], win_start=[], win_count=[], win_tile0=[], tile_item=[], qg_item=[])
    for cw, w in enumerate(ids):
        rows = [i for i, v in enumerate(win) if v == w]
        start, n = len(out["tok"]), len(rows)
        out["tok"] += rows
        out["win_start"].append(start)
        out["win_count"].append(n)
        out["win_tile0"].append(len(out["tile_item"]))
        out["tile_item"] += [[cw, t, start, n] for t in range(-(-n // 32))]
        out["qg_item"] += [[cw, q, start, n] for q in range(-(-n // 128))]
    return out


@pytest.mark.parametrize("do_shift", [False, True])
def test_window_closed_form_matches_loop_and_oracle(do_shift):
    from oracle import window as owin
    coords, sparse = ic.occupancy_coords([10, 10, 8], do_shift, [ic.OCCUPANCIES, ic.OCCUPANCIES[::-1]])
    win, in_win = ic.window_ids_ref(coords, sparse, [10, 10, 8], do_shift)
    # the builder fills windows to exactly the occupancies it was given, one window per entry
    assert sorted(np.bincount(win)[np.unique(win)].tolist()) == sorted(2 * [o for o in ic.OCCUPANCIES if o])
    assert (in_win >= 0).all() and (in_win < np.array([8, 10, 10])).all()
    got, want = ic.window_expect(win), _window_expect_loop(win.tolist())
    for k, v in want.items():
        assert np.array_equal(got[k], np.array(v).reshape(got[k].shape)), k
    conti = owin.continuous_inds(torch.from_numpy(win)).numpy()  # make_continuous_inds: the compact window index
    assert np.array_equal(got["win_count"][conti], np.bincount(win)[win])
    assert np.array_equal(got["tile_item"][got["win_tile0"], 0], np.arange(got["n_windows"]))
    assert got["n_tiles"] == sum(-(-o // 32) for o in ic.OCCUPANCIES) * 2
    assert got["n_qgroups"] == sum(-(-o // 128) for o in ic.OCCUPANCIES) * 2


def test_level_references_on_the_level_tables():
    coords, sparse = ic.occupancy_coords([10, 10, 8], False, [ic.OCCUPANCIES, ic.OCCUPANCIES[::-1]])
    win, _ = ic.window_ids_ref(coords, sparse, [10, 10, 8], False)
    per_win = np.bincount(win)[win]
    for info in refcfg.BATCHING_INFO + [ic.LEVEL_TABLES[k] for k in ("one_level", "overlapping", "range_ends")]:
        rank, level, slot = ic.levels_ref(win, info)
        assert (level >= 0).all() and (slot >= 0).all()
        for bl in info:  # slots of a level: distinct, window-major
            s = slot[level == bl]
            assert np.unique(s).shape[0] == s.shape[0]
    _, level, _ = ic.levels_ref(win, ic.LEVEL_TABLES["overlapping"])
    # 1 is in range 0 only, 33 in ranges 0 and 1, 127 in all three, 257 in range 2 only: the last matching range wins
    assert [set(level[per_win == o]).pop() for o in (1, 33, 127, 257)] == [0, 1, 2, 2]
    _, level, _ = ic.levels_ref(win, ic.LEVEL_TABLES["range_ends"])
    assert [set(level[per_win == o]).pop() for o in (1, 31, 32, 127, 128, 257, 800)] == [0, 0, 1, 1, 2, 3, 3]
    rank, level, slot = ic.levels_ref(win, ic.LEVEL_TABLES["over_cap"])
    assert np.array_equal(slot == -1, rank >= 100) and (slot == -1).sum() == 2 * (27 + 28 + 29 + 157 + 700)
    rank, level, slot = ic.levels_ref(win, ic.LEVEL_TABLES["unmatched"])
    lost = (per_win == 128) | (per_win == 129)
    assert (level[lost] == -1).all() and (slot[lost] == -1).all() and (level[~lost] >= 0).all()
    l3 = np.unique(win[level == 3])  # the level's own windows only
    assert l3.shape[0] == 4 and np.array_equal(slot[level == 3], np.searchsorted(l3, win[level == 3]) * 800 + rank[level == 3])
    assert (np.unique(win[lost]).min() < l3.max())  # unmatched windows lie below level-3 windows in id


def test_geometry_and_canvas_cases():
    from openseg3d_amd.swformer import window_geometry
    for wi, window in enumerate(ic.WINDOW_SHAPES):
        for gi, grid in enumerate(ic.GEOMETRY_GRIDS[wi]):
            coords = ic.geometry_coords(grid, 3, 100 * wi + gi)
            assert np.unique(coords, axis=0).shape[0] == coords.shape[0] and coords[:, 0].max() == 2
            assert (coords[:, 1:] < np.array(grid[::-1])).all() and coords.min() == 0
            for do_shift in (False, True):
                _, nwin, shift = window_geometry(grid, window, do_shift)
                win, _ = ic.window_ids_ref(coords, grid, window, do_shift)
                assert win.min() >= 0 and win.max() < 3 * nwin[0] * nwin[1] * nwin[2]
                assert (shift[2] == 0) == (gi == 2)
                if gi == 0 and not do_shift:  # the largest coordinate lands in the "+1" window of every axis
                    assert win.max() == 3 * nwin[0] * nwin[1] * nwin[2] - 1
    for n in ic.CANVAS_SIZES:
        coords, entry = ic.canvas_coords(n)
        assert entry.min() == 0 and entry.max() == n - 1 and coords.shape[0] <= 1500
        assert {2047, 2048}.issubset(set(entry.tolist())) or n <= 2048
        _, level, slot = ic.levels_ref(entry, ic.CANVAS_INFO)
        assert np.array_equal(level, np.bincount(entry)[entry] - 1) and (slot >= 0).all()
        if n > 4096:
            assert set(level) == {0, 1, 2, 3}
