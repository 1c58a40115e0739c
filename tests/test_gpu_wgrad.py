"""Every weight-gradient kernel path against float64, called through the C ABI.

Sparse conv (dw [cout, 27, cin], dw[o, k, i] = sum over the valid pairs (r, nbr[k, r]) of dy[r, o] * x[nbr[k, r], i]):
  * split-bf16 path, seg3d_spconv_wgrad_partials (+ _xbf16, the SEG3D_TRAIN_STORAGE=bf16 copies) + seg3d_reduce_partials,
    which runs wgrad_sparse_kernel (narrow), wgrad_sparse_wide_kernel on 128 x 128 blocks where they add no padding
    ("fits128") and on the padded rectangular wide layers ("wide_padded");
  * seg3d_spconv_wgrad with flags = 4 (the same kernels and sum in one call: bit-identical to partials + reduce);
  * seg3d_spconv_wgrad with flags = 0, the exact-fp32 kernel spconv_wgrad_kernel<JA, JB> with float atomics.
Dense: seg3d_linear_wgrad_partials_xbf16 + seg3d_reduce_partials (wgrad_dense_kernel<true, false>).

Tables are real neighbour tables (submanifold, strided forward, inverse) of the golden scene and of 60 000 voxels of the
headline scene, plus edited copies: emptied offsets, an empty table, m_out of 1, 63, 64 and 65 rows.  Every call runs with
its workspace and outputs filled with NaN and followed by a 4 KiB guard of known bits: a partial block that is never
written shows up as NaN, a store past its slice as a changed guard or workspace tail.

Bars.  Split-bf16 products carry ~2^-16 relative error and the fp32 sums round-off that grows as a random walk, so the
elementwise bar is |dw - ref| <= C_SPLIT * 2^-16 * s with s = sqrt(sum over pairs of (x * dy)^2) of that entry, next to
the suite's usual max-norm bar 1e-4 * max(1, max|ref|).  A path that multiplied in plain bf16 (2^-9 per product) misses the
elementwise bar by two orders of magnitude.  For bf16 rows the reference takes bf16(x): exactly the operand the kernel gets.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import refcfg

pytestmark = pytest.mark.gpu

GUARD = 1024  # 4 KiB of known bits after every buffer a kernel writes
# Elementwise bar of the split paths in units of 2^-16 s.  Measured on the MI355X over every case of this file: worst 1.80
# with fp32 rows (sparse), 1.00 with bf16 rows (sparse), 0.72 (dense, bf16 rows): 2.2x headroom.  Multiplying the bf16
# rows by the high half of dy alone (the low-half MFMA of mfma2 dropped) measured 151 - 630 (sparse) and 200 - 453 (dense)
# in every case with a pair: 38x this bar and more.
C_SPLIT = 4.0
# exact-fp32 path (fp32 MFMA products, float atomics whose order varies run to run): max|dw - ref| / max|ref| measured at
# 6.9e-7 at worst over every case of this file; 5.8x headroom
FP32_BAR = 4e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from openseg3d_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables(dev):
    """name -> (nbr int32 [27, m_out] on the device, m_in)."""
    from oracle import index_ops, sparse_conv as sc
    from openseg3d_amd import scene
    shape = refcfg.GRID_CART[::-1].tolist()
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segformer_cart.npz"))
    g = sc.Sites(golden["voxel_coords"].astype(np.int32), shape)
    g_coarse, g_fwd, g_inv = g.down()
    # the first 60 000 voxels of the headline scene (as test_gpu_parity.py's headline_sites): SPNet's row counts
    hc, _ = index_ops.voxelize(scene.make_scene(0), refcfg.CART_VOXEL, refcfg.CART_RANGE)
    h = sc.Sites(np.pad(hc[:60000], ((0, 0), (1, 0))).astype(np.int32), shape)
    h_coarse, h_fwd, h_inv = h.down()
    mg, mgc, mh, mhc = g.coords.shape[0], g_coarse.coords.shape[0], h.coords.shape[0], h_coarse.coords.shape[0]
    assert mh >= 50000
    subm = g.subm()
    hole = subm.copy()
    hole[[5, 13]] = -1  # the centre offset (the units dispatched first) and one other offset without a single pair
    t = {"subm": (subm, mg), "down": (g_fwd, mg), "inv": (g_inv, mgc),
         "subm_hole": (hole, mg), "subm_none": (np.full_like(subm, -1), mg), "down_none": (np.full_like(g_fwd, -1), mg),
         "big_subm": (h.subm(), mh), "big_down": (h_fwd, mh), "big_inv": (h_inv, mhc)}
    for m in (1, 63, 64, 65):
        t[f"subm_m{m}"] = (subm[:, :m], mg)
    return {k: (torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev), m_in) for k, (v, m_in) in t.items()}


def _route(cin, cout):
    """The sparse split path's kernel choice (wgrad_split.hip, wgrad_split_sparse) with the A/B switches at their defaults."""
    fits128 = (cin + 127) // 128 * 2 == (cin + 63) // 64 and (cout + 127) // 128 * 2 == (cout + 63) // 64
    padded = cin != cout and min(cin, cout) >= 96 and max(cin, cout) >= 192
    return "fits128" if fits128 else "padded" if padded else "narrow"


def _operands(dev, nbr, m_in, cin, cout, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(m_in, cin, device=dev, generator=gen)
    dy = torch.randn(nbr.shape[1], cout, device=dev, generator=gen)
    return x, dy


def _reference(x, dy, nbr):
    """float64 dw [cout, 27, cin] and s = sqrt(sum of squared products) per entry, from the table itself."""
    x64, dy64 = x.double(), dy.double()
    ref = torch.zeros(dy.shape[1], 27, x.shape[1], dtype=torch.float64, device=x.device)
    s2 = torch.zeros_like(ref)
    for k in range(27):
        rows = torch.nonzero(nbr[k] >= 0).view(-1)
        if rows.numel() == 0:
            continue
        xs = x64.index_select(0, nbr[k, rows].long())
        ys = dy64.index_select(0, rows)
        ref[:, k, :] = ys.t() @ xs
        s2[:, k, :] = (ys * ys).t() @ (xs * xs)
    return ref, s2.sqrt()


def _guarded(n, dev):
    """float32 [n + GUARD]: NaN, then the guard bits."""
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    buf.view(torch.int32)[n:] = _pattern(dev)
    return buf


def _pattern(dev):
    return torch.arange(GUARD, dtype=torch.int32, device=dev) * 40503 + 0x3A5C0000


def _guard_intact(buf, n):
    return torch.equal(buf.view(torch.int32)[n:], _pattern(buf.device))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _split_once(x, dy, nbr, cin, cout):
    """seg3d_spconv_wgrad_partials(_xbf16) + seg3d_reduce_partials on NaN-filled, guarded buffers -> (dw, chunks)."""
    from openseg3d_amd import _lib
    dev = dy.device
    m_out, n = nbr.shape[1], 27 * cin * cout
    ws_bytes = _lib.query("seg3d_spconv_wgrad_workspace_bytes", m_out, cin, cout)
    assert ws_bytes % 4 == 0
    ws_n = ws_bytes // 4
    ws, dw = _guarded(ws_n, dev), _guarded(n, dev)
    chunks = ctypes.c_int32(-1)
    name = "seg3d_spconv_wgrad_partials_xbf16" if x.dtype == torch.bfloat16 else "seg3d_spconv_wgrad_partials"
    _lib.call(name, _ptr(x), _ptr(dy), _ptr(nbr), m_out, x.shape[0], cin, cout, _ptr(ws), ws_bytes, ctypes.byref(chunks),
              _stream())
    c = chunks.value
    assert 1 <= c and c * n <= ws_n
    _lib.call("seg3d_reduce_partials", _ptr(ws), c, n, n, _ptr(dw), None, _stream())
    torch.cuda.synchronize()
    assert _guard_intact(ws, ws_n) and _guard_intact(dw, n), "a store past the queried workspace or past dw"
    assert not torch.isnan(ws[:c * n]).any(), "a (chunk, offset, block) partial was never written"
    assert torch.isnan(ws[c * n:ws_n]).all(), "a store past the last chunk's cin x cout slice"
    assert not torch.isnan(dw[:n]).any()
    return dw[:n].view(cout, 27, cin), c


def _split(x, dy, nbr, cin, cout):
    dw, c = _split_once(x, dy, nbr, cin, cout)
    dw2, c2 = _split_once(x, dy, nbr, cin, cout)
    assert c2 == c and torch.equal(dw, dw2), "the split path is not bit-reproducible"
    return dw, c


def _fused(x, dy, nbr, cin, cout, flags):
    """seg3d_spconv_wgrad (flags 4: split-bf16, 0: exact fp32) on NaN-filled, guarded buffers."""
    from openseg3d_amd import _lib
    dev = dy.device
    m_out, n = nbr.shape[1], 27 * cin * cout
    ws_bytes = _lib.query("seg3d_spconv_wgrad_workspace_bytes", m_out, cin, cout)
    ws_n = ws_bytes // 4
    ws, dw = _guarded(ws_n, dev), _guarded(n, dev)
    _lib.call("seg3d_spconv_wgrad", _ptr(x), _ptr(dy), _ptr(nbr), m_out, x.shape[0], cin, cout, flags, _ptr(dw), _ptr(ws),
              ws_bytes, _stream())
    torch.cuda.synchronize()
    assert _guard_intact(ws, ws_n) and _guard_intact(dw, n), "a store past the queried workspace or past dw"
    assert not torch.isnan(dw[:n]).any()
    return dw[:n].view(cout, 27, cin)


def _check_split_bars(dw, ref, s, what):
    err = (dw.double() - ref).abs()
    scale = max(1.0, float(ref.abs().max()))
    worst = float((err / (2.0 ** -16 * s).clamp_min(1e-300)).max())  # (entries without a pair: s = 0, dw must be 0)
    print(f"{what}: max|dw - ref| / max(1, max|ref|) = {float(err.max()) / scale:.3g}, worst |dw - ref| / (2^-16 s) = {worst:.3g}")
    assert bool((err <= C_SPLIT * 2.0 ** -16 * s).all()), (what, worst, C_SPLIT)
    assert float(err.max()) <= 1e-4 * scale, (what, float(err.max()), scale)


def _check_sparse_split(dev, tables, table, cin, cout, seed, fused=False):
    """fp32 and bf16 rows through the split path of one (table, shape); returns the chunk count."""
    nbr, m_in = tables[table]
    x, dy = _operands(dev, nbr, m_in, cin, cout, seed)
    ref, s = _reference(x, dy, nbr)
    dw, chunks = _split(x, dy, nbr, cin, cout)
    _check_split_bars(dw, ref, s, f"{table} {cin}->{cout} fp32 rows")
    if fused:
        assert torch.equal(_fused(x, dy, nbr, cin, cout, 4), dw), "flags = 4 differs from partials + reduce"
    xb = x.to(torch.bfloat16)
    ref_b, s_b = _reference(xb, dy, nbr)
    dw_b, chunks_b = _split(xb, dy, nbr, cin, cout)
    assert chunks_b == chunks
    _check_split_bars(dw_b, ref_b, s_b, f"{table} {cin}->{cout} bf16 rows")
    if not (nbr >= 0).any():
        assert float(dw.abs().max()) == 0.0 and float(dw_b.abs().max()) == 0.0
    return chunks


NARROW = [(16, 16), (32, 32), (32, 64), (48, 48), (64, 64), (80, 48), (48, 80), (192, 192)]
FITS128 = [(128, 128), (256, 256), (128, 256), (256, 128), (384, 384), (768, 384), (112, 208), (80, 112), (96, 96)]
PADDED = [(96, 192), (192, 96), (384, 192), (112, 192)]
SHAPES = [(c, "narrow") for c in NARROW] + [(c, "fits128") for c in FITS128] + [(c, "padded") for c in PADDED]


@pytest.mark.parametrize("table", ["subm", "down", "inv"])
@pytest.mark.parametrize("shape,kernel", SHAPES, ids=[f"{a}-{b}" for (a, b), _ in SHAPES])
def test_sparse_split_wgrad_on_golden_tables(dev, tables, shape, kernel, table):
    """Submanifold, strided-forward and inverse tables of the golden scene, every kernel of the split path, widths that are
    and are not multiples of 64 (channel quads past cin / cout: only the store masks keep them out of dw)."""
    cin, cout = shape
    assert _route(cin, cout) == kernel
    _check_sparse_split(dev, tables, table, cin, cout, seed=cin * 1000 + cout, fused=table == "subm")


SPNET = [("big_subm", 32, 32), ("big_subm", 64, 64), ("big_subm", 128, 128), ("big_subm", 256, 256),
         ("big_down", 32, 64), ("big_down", 64, 128), ("big_down", 128, 256),
         ("big_inv", 256, 128), ("big_inv", 128, 64), ("big_inv", 64, 32)]


@pytest.mark.parametrize("table,cin,cout", SPNET)
def test_sparse_split_wgrad_at_spnet_widths_and_row_counts(dev, tables, table, cin, cout):
    """SPNet's 32 / 64 / 128 / 256 widths, its 128 <-> 256 strided and inverse layers, on >= 47 000-row tables."""
    chunks = _check_sparse_split(dev, tables, table, cin, cout, seed=cin + 7 * cout, fused=(cin, cout) == (256, 256))
    assert chunks > 1


EDITS = ["subm_hole", "subm_none", "down_none", "subm_m1", "subm_m63", "subm_m64", "subm_m65"]


@pytest.mark.parametrize("table", EDITS)
@pytest.mark.parametrize("cin,cout", [(16, 16), (48, 48), (128, 256), (96, 192)])
def test_sparse_split_wgrad_on_edited_tables(dev, tables, cin, cout, table):
    """Offsets without a single pair, a table without any (dw exactly 0), and m_out around one 64-row group."""
    _check_sparse_split(dev, tables, table, cin, cout, seed=cin + cout + len(table), fused=True)


def test_split_chunk_counts_reach_the_grid_padding_edges(dev, tables):
    """The XCD-aligned grid pads the (chunk, offset) units to a multiple of 8 and maps the centre units first: chunk
    counts of 1, 2, counts that are not multiples of 8 and >= 38 must all be hit (asserted from what the entry reports)."""
    seen = {}
    for table in ("subm_m1", "subm_m64", "subm_m65", "subm", "big_subm"):
        for cin, cout in ((16, 16), (48, 48)):
            seen[(table, cin, cout)] = _check_sparse_split(dev, tables, table, cin, cout, seed=3)
    counts = set(seen.values())
    assert {1, 2} <= counts, seen
    assert any(c % 8 for c in counts if c > 8), seen
    assert max(counts) >= 38, seen


EXACT = [(a, b) for a in (16, 32, 48, 64) for b in (16, 32, 48, 64)] + [(80, 112)]


@pytest.mark.parametrize("table", ["subm", "down", "inv"])
@pytest.mark.parametrize("cin,cout", EXACT)
def test_exact_fp32_sparse_wgrad(dev, tables, cin, cout, table):
    """seg3d_spconv_wgrad without the split flag: spconv_wgrad_kernel<JA, JB>, J = 4 / 3 / 2 / 1 for widths % 64 / % 48 /
    % 32 / other -- all 16 instantiations.  fp32 products and sums (float atomics: the order varies, not the grade)."""
    nbr, m_in = tables[table]
    x, dy = _operands(dev, nbr, m_in, cin, cout, seed=cin * 100 + cout)
    ref, _ = _reference(x, dy, nbr)
    dw = _fused(x, dy, nbr, cin, cout, 0)
    rel = float((dw.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"exact fp32 {table} {cin}->{cout}: max|dw - ref| / max|ref| = {rel:.3g}")
    assert rel <= FP32_BAR, rel


@pytest.mark.parametrize("table,cin,cout", [("big_subm", 64, 64), ("big_down", 32, 64), ("big_inv", 48, 16),
                                            ("subm_m1", 16, 16), ("subm_m65", 32, 48), ("subm_hole", 64, 32),
                                            ("subm_none", 48, 48)])
def test_exact_fp32_sparse_wgrad_at_row_count_edges(dev, tables, table, cin, cout):
    """The exact-fp32 kernel on >= 47 000-row tables, on m_out = 1 and 65, an emptied centre offset and an empty table."""
    nbr, m_in = tables[table]
    x, dy = _operands(dev, nbr, m_in, cin, cout, seed=5)
    ref, _ = _reference(x, dy, nbr)
    dw = _fused(x, dy, nbr, cin, cout, 0)
    if not (nbr >= 0).any():
        assert float(dw.abs().max()) == 0.0
        return
    rel = float((dw.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"exact fp32 {table} {cin}->{cout}: max|dw - ref| / max|ref| = {rel:.3g}")
    assert rel <= FP32_BAR, rel


@pytest.mark.parametrize("m", [1, 31, 32, 33, 70001])
@pytest.mark.parametrize("with_bias", [0, 1])
@pytest.mark.parametrize("cin,cout", [(12, 40), (20, 36), (104, 200)])
def test_dense_xbf16_wgrad_partials(dev, cin, cout, with_bias, m):
    """seg3d_linear_wgrad_partials_xbf16 + seg3d_reduce_partials (wgrad_dense_kernel<true, false>) at widths the Linear
    layers never route there yet (cin % 16 != 0, ragged 64-channel blocks), with the ragged last 32-row step."""
    from openseg3d_amd import _lib
    gen = torch.Generator(device=dev).manual_seed(m + cin + with_bias)
    xb = torch.randn(m, cin, device=dev, generator=gen).to(torch.bfloat16)
    dy = torch.randn(m, cout, device=dev, generator=gen)
    nw, n = cin * cout, cin * cout + cout
    ws_bytes = _lib.query("seg3d_linear_wgrad_workspace_bytes", m, cin, cout)
    ws_n = ws_bytes // 4
    outs = []
    for _ in range(2):
        ws, dw, db = _guarded(ws_n, dev), _guarded(nw, dev), _guarded(cout, dev)
        chunks = ctypes.c_int32(-1)
        _lib.call("seg3d_linear_wgrad_partials_xbf16", _ptr(xb), _ptr(dy), m, cin, cout, with_bias, _ptr(ws), ws_bytes,
                  ctypes.byref(chunks), _stream())
        c = chunks.value
        assert 1 <= c and c * n <= ws_n
        _lib.call("seg3d_reduce_partials", _ptr(ws), c, n, nw, _ptr(dw), _ptr(db) if with_bias else None, _stream())
        torch.cuda.synchronize()
        assert _guard_intact(ws, ws_n) and _guard_intact(dw, nw) and _guard_intact(db, cout)
        part = ws[:c * n].view(c, n)
        assert not torch.isnan(part[:, :nw]).any(), "a (chunk, block) partial was never written"
        if with_bias:
            assert not torch.isnan(part[:, nw:]).any()
        assert torch.isnan(ws[c * n:ws_n]).all(), "a store past the last chunk's partial"
        assert not torch.isnan(dw[:nw]).any()
        if with_bias:
            assert not torch.isnan(db[:cout]).any()
        else:
            assert torch.isnan(db[:cout]).all()  # no db asked for: none written
        outs.append((dw[:nw].clone(), db[:cout].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and (not with_bias or torch.equal(outs[0][1], outs[1][1]))
    x64, dy64 = xb.double(), dy.double()
    ref = dy64.t() @ x64
    s = ((dy64 * dy64).t() @ (x64 * x64)).sqrt()
    _check_split_bars(outs[0][0].view(cout, cin), ref, s, f"dense {m} {cin}->{cout} bf16 rows")
    if with_bias:
        ref_b = dy64.sum(0)
        err_b = (outs[0][1].double() - ref_b).abs()
        assert float(err_b.max()) <= 1e-4 * max(1.0, float(ref_b.abs().max()))
        assert bool((err_b <= C_SPLIT * 2.0 ** -16 * (dy64 * dy64).sum(0).sqrt()).all())
