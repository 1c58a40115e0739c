"""The small device ops over the whole range they accept, each against the plain fp64 composition of the reference
operation on the CPU: class_context (class_context.hip), knn_attention (knn_attention.hip), segment_reduce / scatter /
gather_rows (segment.hip), group_index and its scan (group.hip, scan.hip), span_mean / FlattenSELayer (rownorm.hip's
column sums) and the criterion kernels at 2 and 64 classes.  Forward and every gradient, with an upstream gradient that
is not all ones.  The shapes are the smallest that reach the code path each case names.

Tolerances: the forms the older tests of each op state (test_gpu_parity.py, test_gpu_losses.py), unchanged.  Where none
was stated (SUM, span_mean, FlattenSELayer) the bound is 4x the error of the fp32 torch evaluation of the same reference
composition on the CPU against its own fp64 value at that shape: the kernels sum in a different but fixed order, and 4x
covers a reordering, not a wrong term.  The measured values are written into the docstrings of the tests that use them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _maxerr(got, ref):
    return float((got.detach().cpu().double() - ref.detach()).abs().max()) if ref.numel() else 0.0


def _scale_of(ref):
    return max(1.0, float(ref.detach().abs().max())) if ref.numel() else 1.0


# ------------------------------------------------------------------------------------------ class_context
def _context_ref(feats, probs, offsets, scale, g):
    """ocr.py:22-33 per sample in fp64 autograd; rows behind the last offset are in no sample (zero gradients)."""
    fr, pr = feats.double().requires_grad_(), probs.double().requires_grad_()
    k = probs.shape[1]
    out, lo = [], 0
    for hi in offsets:
        prob = torch.softmax(scale * pr[lo:hi].t(), dim=1) if hi > lo else pr.new_zeros((k, 0))
        out.append(prob @ fr[lo:hi])
        lo = hi
    ref = torch.stack(out)
    ref.backward(g.double())
    return ref.detach(), fr.grad, pr.grad


def _context_check(dev, k, c, rows, tail, scale, prob_gain=3.0):
    from openseg3d_amd import ops
    gen = torch.Generator().manual_seed(1000 * k + c + sum(rows) + tail)
    m = sum(rows) + tail
    feats = torch.randn(m, c, generator=gen)
    probs = torch.randn(m, k, generator=gen) * prob_gain
    g = torch.randn(len(rows), k, c, generator=gen)
    offsets = np.cumsum(rows).tolist()
    ref, dfeats, dprobs = _context_ref(feats, probs, offsets, scale, g)
    assert ops.class_context_fits(k, c)
    fg, pg = feats.to(dev).requires_grad_(), probs.to(dev).requires_grad_()
    ctx = ops.class_context(fg, pg, offsets, scale)
    ctx.backward(g.to(dev))
    assert ctx.shape == ref.shape
    errs = (_maxerr(ctx, ref), _maxerr(fg.grad, dfeats), _maxerr(pg.grad, dprobs))
    print("class_context", k, c, rows, tail, scale, "errors", errs)
    assert errs[0] < 2e-5 * _scale_of(ref)
    assert errs[1] < 2e-5 * _scale_of(dfeats)
    assert errs[2] < 1e-4 * _scale_of(dprobs)
    if tail:  # exactly zero, not merely small
        assert float(fg.grad[m - tail:].abs().max()) == 0.0 and float(pg.grad[m - tail:].abs().max()) == 0.0
    first = (ctx.detach().clone(), fg.grad.clone(), pg.grad.clone())
    fg.grad = pg.grad = None
    again = ops.class_context(fg, pg, offsets, scale)
    again.backward(g.to(dev))
    assert torch.equal(first[0], again) and torch.equal(first[1], fg.grad) and torch.equal(first[2], pg.grad)
    return probs, dprobs


_CONTEXT_SHAPES = [(1, 4), (7, 36), (22, 260), (32, 384), (12, 1024), (32, 128)]
_CONTEXT_ROWS = [([1], 0), ([127, 128, 129], 0), ([0, 0, 5], 0), ([300, 0], 0), ([300], 40)]
_CONTEXT_SCALES = [0.125, 1.0, 4.0]


@pytest.mark.parametrize("rows,tail", _CONTEXT_ROWS)
@pytest.mark.parametrize("k,c", _CONTEXT_SHAPES)
def test_class_context_over_its_envelope(dev, k, c, rows, tail):
    """Every (classes, C) corner -- one class and 4 channels; neither a power of two; C = 260, the first that takes the
    256-channel loop twice; classes * C = 12288 twice, where the backward's dynamic LDS is exactly 64 KiB; all 32 class
    slots -- against the reference loop, with one row, rows around the 128-row chunk, empty samples first and last, and
    40 rows behind the last offset, which are in no sample and get exactly zero gradients.  The three scales rotate over
    the cases, so each shape meets each of them."""
    scale = _CONTEXT_SCALES[(_CONTEXT_SHAPES.index((k, c)) + [r for r, _ in _CONTEXT_ROWS].index(rows)) % 3]
    _context_check(dev, k, c, rows, tail, scale)


@pytest.mark.parametrize("scale", _CONTEXT_SCALES)
def test_class_context_scale_reaches_every_term(dev, scale):
    """scale multiplies the scores inside the softmax and d probs outside it: all three values at one shape, and the
    gradient w.r.t. probs differs between them (a dropped factor cannot hide behind the tolerance)."""
    _, dprobs = _context_check(dev, 22, 260, [127, 128, 129], 0, scale)
    assert float(dprobs.abs().max()) > 1e-3


def test_class_context_near_one_hot_softmax(dev):
    """probs * 30: per class nearly all the weight sits on one row and most weights underflow to 0 in float32."""
    probs, _ = _context_check(dev, 7, 36, [127, 128, 129], 0, 1.0, prob_gain=30.0)
    w = torch.softmax(probs[:127], dim=0)  # the first sample's weights, in float32 as the kernel holds them
    assert float(w.max(dim=0).values.median()) > 0.9 and int((w == 0).sum()) > 0


def test_class_context_fits_agrees_with_the_launch(dev):
    """class_context_fits is the wrapper's gate and bad_shape the library's: the same set of (classes, C).  Shapes on both
    sides of every bound; the library is asked directly (below the wrapper's gate) for the ones that do not fit."""
    from openseg3d_amd import _lib, ops
    fits = [(1, 4), (32, 384), (12, 1024), (3, 1024), (24, 512)]
    no_fit = [(33, 4), (0, 4), (4, 0), (4, 6), (4, 1028), (32, 388), (13, 1024), (25, 512)]
    for k, c in fits + no_fit:
        assert ops.class_context_fits(k, c) == ((k, c) in fits), (k, c)
    for k, c in fits:
        feats = torch.randn(5, c, device=dev, requires_grad=True)
        probs = torch.randn(5, k, device=dev, requires_grad=True)
        ops.class_context(feats, probs, [5]).sum().backward()
        assert bool(torch.isfinite(feats.grad).all()) and bool(torch.isfinite(probs.grad).all())
    for k, c in no_fit:
        if k < 1 or c < 1:
            continue
        feats, probs = torch.randn(5, c, device=dev), torch.randn(5, k, device=dev)
        with pytest.raises(_lib.Seg3dError):
            ops.class_context(feats, probs, [5])
        with pytest.raises(_lib.Seg3dError):  # the library's own gate
            ops._ClassContextFn.apply(feats, probs, ops.class_context_plan([5], dev), 1.0)


def test_class_context_refuses_bad_offsets(dev):
    from openseg3d_amd import _lib, ops
    feats, probs = torch.randn(10, 8, device=dev), torch.randn(10, 3, device=dev)
    for bad in ([6, 4], [4, 11], [-1, 5], [11]):
        with pytest.raises(_lib.Seg3dError):
            ops.class_context(feats, probs, bad)
    assert ops.class_context(feats, probs, [4, 4, 10]).shape == (3, 3, 8)


# ------------------------------------------------------------------------------------------ knn_attention
def _knn_ref(q, k, v, idx, invalid, keep, scale, g, need=(True, True, True)):
    """deep_fusion.py:31-43 in fp64 autograd."""
    qr, kr, vr = (t.double().requires_grad_(r) for t, r in zip((q, k, v), need))
    li = idx.long()
    attn = torch.einsum("nc,nkc->nk", qr, kr[li]) * (scale if scale is not None else q.shape[1] ** -0.5)
    if invalid is not None:
        attn = attn.masked_fill(invalid[li], float("-inf"))
    attn = torch.nan_to_num(torch.softmax(attn, dim=-1))
    if keep is not None:
        attn = attn * keep.double()
    ref = torch.einsum("nk,nkc->nc", attn, vr[li])
    ref.backward(g.double())
    return ref.detach(), [t.grad for t in (qr, kr, vr)]


def _knn_check(dev, q, k, v, idx, g, invalid=None, keep=None, scale=None, need=(True, True, True), reproducible=True):
    from openseg3d_amd import ops
    ref, grads = _knn_ref(q, k, v, idx, invalid, keep, scale, g, need)
    on = lambda t: None if t is None else t.to(dev)  # noqa: E731
    leaves = [t.to(dev).requires_grad_(r) for t, r in zip((q, k, v), need)]
    out = ops.knn_attention(*leaves, on(idx), on(invalid), on(keep), scale)
    out.backward(on(g))
    err = _maxerr(out, ref)
    gerrs = [None if w is None else (_maxerr(t.grad, w), _scale_of(w)) for t, w in zip(leaves, grads)]
    print("knn_attention", tuple(q.shape), tuple(idx.shape), k.shape[0], "out", err, "grads", gerrs)
    assert err < 2e-5
    for name, t, w in zip(("dq", "dk", "dv"), leaves, grads):
        if w is None:
            assert t.grad is None, name
        else:
            assert _maxerr(t.grad, w) < 1e-4 * _scale_of(w), name
    if reproducible:
        first = [out.detach().clone()] + [None if t.grad is None else t.grad.clone() for t in leaves]
        for t in leaves:
            t.grad = None
        again = ops.knn_attention(*leaves, on(idx), on(invalid), on(keep), scale)
        again.backward(on(g))
        assert torch.equal(first[0], again)
        assert all(a is None or torch.equal(a, t.grad) for a, t in zip(first[1:], leaves))
    return out.detach(), leaves, grads


def _knn_inputs(n, n_src, kk, seed, idx_hi=None):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(n, 32, generator=gen)
    k = torch.randn(n_src, 32, generator=gen)
    v = torch.randn(n_src, 32, generator=gen)
    idx = torch.randint(0, idx_hi or n_src, (n, kk), generator=gen, dtype=torch.int32)
    g = torch.randn(n, 32, generator=gen)
    return gen, q, k, v, idx, g


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099])
@pytest.mark.parametrize("kk", [1, 2, 15, 16])
def test_knn_attention_group_and_block_edges(dev, kk, n):
    """K at both ends of 1..16 and n around the 16-lane group (a 256-thread block holds 16 queries) and past sixteen
    blocks plus three queries, each with 1, 37 and 2500 source rows; a third of the sources masked, dropout factors on."""
    for n_src in (1, 37, 2500):
        gen, q, k, v, idx, g = _knn_inputs(n, n_src, kk, 100 * n + kk + n_src)
        invalid = torch.rand(n_src, generator=gen) < 0.3
        keep = (torch.rand(n, kk, generator=gen) >= 0.3).float() / 0.7
        _knn_check(dev, q, k, v, idx, g, invalid, keep, reproducible=(n_src == 37))


def test_knn_attention_without_a_mask_and_with_everything_masked(dev):
    """invalid=None takes the kernel's null-pointer branch; with every source invalid the output and all three gradients
    are exactly 0 (nan_to_num of a row of -inf)."""
    gen, q, k, v, idx, g = _knn_inputs(4099, 2500, 16, 1)
    _knn_check(dev, q, k, v, idx, g, invalid=None)
    out, leaves, _ = _knn_check(dev, q, k, v, idx, g, invalid=torch.ones(2500, dtype=torch.bool))
    assert float(out.abs().max()) == 0.0
    assert all(float(t.grad.abs().max()) == 0.0 for t in leaves)


def test_knn_attention_explicit_scale_and_sharp_softmax(dev):
    """scale=0.3 (not 32 ** -0.5) reaches the logits, dq and dk; q * 20 gives logits of +-60 and a near one-hot softmax."""
    gen, q, k, v, idx, g = _knn_inputs(4099, 2500, 15, 2)
    invalid = torch.rand(2500, generator=gen) < 0.3
    _knn_check(dev, q, k, v, idx, g, invalid, scale=0.3)
    _knn_check(dev, q * 20, k, v, idx, g, invalid)


def test_knn_attention_hub_and_unreferenced_sources(dev):
    """Every query's first neighbour is source row 0: one inverse list of 4099 pairs (plus the random hits), summed in a
    fixed order.  Only rows below 1000 are ever referenced: the other 1500 get exactly 0 in dk and dv."""
    gen, q, k, v, idx, g = _knn_inputs(4099, 2500, 16, 3, idx_hi=1000)
    idx[:, 0] = 0
    _, leaves, _ = _knn_check(dev, q, k, v, idx, g)
    assert float(leaves[1].grad[1000:].abs().max()) == 0.0 and float(leaves[2].grad[1000:].abs().max()) == 0.0
    assert float(leaves[1].grad[0].abs().max()) > 0.0


def test_knn_attention_dropped_row_only_v_and_column_slices(dev):
    """A query whose dropout factors are all 0 (output 0, no gradient through it); only v requiring a gradient; and q, k,
    v handed over as non-contiguous column slices of one wider tensor."""
    from openseg3d_amd import ops
    gen, q, k, v, idx, g = _knn_inputs(4099, 2500, 16, 4)
    invalid = torch.rand(2500, generator=gen) < 0.3
    keep = (torch.rand(4099, 16, generator=gen) >= 0.3).float() / 0.7
    keep[5] = 0.0
    out, leaves, _ = _knn_check(dev, q, k, v, idx, g, invalid, keep)
    assert float(out[5].abs().max()) == 0.0 and float(leaves[0].grad[5].abs().max()) == 0.0
    _knn_check(dev, q, k, v, idx, g, invalid, keep, need=(False, False, True))
    # column slices: [n, 96] rows, q = columns 0..31, k = 32..63, v = 64..95 (n == n_src here)
    wide = torch.randn(2500, 96, generator=gen)
    idx2, g2 = idx[:2500], g[:2500]
    ref, grads = _knn_ref(wide[:, :32], wide[:, 32:64], wide[:, 64:], idx2, invalid, None, None, g2)
    wg = wide.to(dev).requires_grad_()
    qs, ks, vs = wg[:, :32], wg[:, 32:64], wg[:, 64:]
    assert not qs.is_contiguous()
    out = ops.knn_attention(qs, ks, vs, idx2.to(dev), invalid.to(dev))
    out.backward(g2.to(dev))
    assert _maxerr(out, ref) < 2e-5
    want = torch.cat(grads, dim=1)
    assert _maxerr(wg.grad, want) < 1e-4 * _scale_of(want)


# ------------------------------------------------------------------------------------------ segment ops
def _segment_ref(x, ids, n_seg, mode, g):
    """torch_scatter.scatter(src, index, dim=0, reduce=mode, dim_size=n_seg) over the rows whose id is in [0, n_seg), in
    fp64; returns (out, d x).  MAX: empty segments give 0 and the gradient goes to the lowest-index row among the maxima
    (this build's rule: seg_reduce_kernel replaces its candidate on ``val > acc`` only)."""
    xr = x.double()
    n, c = xr.shape
    ok = (ids >= 0) & (ids < n_seg)
    rows = torch.nonzero(ok)[:, 0]
    idv = ids[ok].long()
    cnt = torch.bincount(idv, minlength=n_seg)
    if mode in ("sum", "mean"):
        xr.requires_grad_()
        out = torch.zeros((n_seg, c), dtype=xr.dtype).index_add(0, idv, xr[rows])
        if mode == "mean":
            out = out / cnt.clamp(min=1).to(xr.dtype)[:, None]
        out.backward(g.double())
        return out.detach(), xr.grad
    red = torch.full((n_seg, c), float("-inf"), dtype=xr.dtype).index_reduce(0, idv, xr[rows], "amax", include_self=True)
    out = torch.where(cnt[:, None] > 0, red, torch.zeros_like(red))
    big = float(n)
    cand = torch.where(xr[rows] == red[idv], rows.double()[:, None].expand(-1, c), torch.full((1, 1), big, dtype=xr.dtype))
    arg = torch.full((n_seg, c), big, dtype=xr.dtype).index_reduce(0, idv, cand, "amin", include_self=True).long()
    dx = torch.zeros((n, c), dtype=xr.dtype)
    s, ch = torch.nonzero(cnt[:, None].expand(-1, c) > 0, as_tuple=True)
    dx[arg[s, ch], ch] = g.double()[s, ch]
    return out, dx


def _skewed_ids(n_seg=3600):
    """One segment of 20 000 rows, 3 000 singletons, 100 segments of 7 rows, the rest empty; 10 % of the rows at -1;
    shuffled."""
    rs = np.random.RandomState(5)
    ids = np.concatenate([np.full(20000, 5), np.arange(10, 3010), np.repeat(np.arange(3100, 3200), 7)])
    rs.shuffle(ids)
    ids[rs.rand(ids.shape[0]) < 0.1] = -1
    assert n_seg > 3200
    return torch.from_numpy(ids.astype(np.int64)), n_seg


# 4 x the error of the fp32 CPU evaluation (index_add_ over float32 rows) against its fp64 value on _skewed_ids, x = randn
# with seed 40 + C: measured 1.0691e-03 (C = 4), 5.1796e-04 (6), 7.8341e-04 (64), 1.1464e-03 (260)
_SUM_BOUND = {4: 4 * 1.0691e-03, 6: 4 * 5.1796e-04, 64: 4 * 7.8341e-04, 260: 4 * 1.1464e-03}
_MODES = {"sum": 0, "mean": 1, "max": 2}


@pytest.mark.parametrize("c", [4, 6, 64, 260])
@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_segment_reduce_on_a_skewed_index(dev, mode, c):
    """SUM, MEAN and MAX, forward and backward, at C = 4 and 64 (float4 path), 6 (scalar path) and 260 (a row wider than a
    block's 256 threads / 65 quads), on an index with one 20 000-row segment, singletons, empty segments and skipped rows.
    MAX is exact; MEAN and every gradient are within 1e-6.  SUM had no stated bound: the fp32 index_add_ of the same
    rows on the CPU is off its fp64 value by 1.07e-03 / 5.2e-04 / 7.8e-04 / 1.15e-03 at C = 4 / 6 / 64 / 260 (18 000 additions
    in row order into a sum that reaches |190|..|450|, where one float32 ulp is 1.5e-05..3.1e-05); the bound is 4x that,
    _SUM_BOUND."""
    from openseg3d_amd import ops
    ids, n_seg = _skewed_ids()
    gen = torch.Generator().manual_seed(40 + c)
    x = torch.randn(ids.shape[0], c, generator=gen)
    g = torch.randn(n_seg, c, generator=gen)
    ref, dx = _segment_ref(x, ids, n_seg, mode, g)
    xg = x.to(dev).requires_grad_()
    out = ops.segment_reduce(xg, ops.SegmentIndex(ids.to(dev), n_seg), _MODES[mode])
    out.backward(g.to(dev))
    err = _maxerr(out, ref)
    print("segment_reduce", mode, c, "out", err, "dx", _maxerr(xg.grad, dx))
    assert err <= {"sum": _SUM_BOUND[c], "mean": 1e-6, "max": 0.0}[mode]
    assert _maxerr(xg.grad, dx) <= 1e-6
    # the torch_scatter-shaped entry gives the same bits
    again = ops.scatter(x.to(dev), ids.to(dev), dim=0, reduce=mode, dim_size=n_seg)
    assert torch.equal(again, out.detach())


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_scatter_ignores_ids_outside_the_segments(dev, mode):
    """Ids >= dim_size are skipped by the CSR build, so the forward ignores such rows; their gradient is exactly 0 (the
    SUM / MEAN backward used to read d out and the offsets behind their ends for them).  Then all ids at -1, no rows at
    all, and no segments at all."""
    from openseg3d_amd import ops
    gen = torch.Generator().manual_seed(7)
    n, c, n_seg = 5000, 6, 40
    x = torch.randn(n, c, generator=gen)
    ids = torch.randint(-1, 60, (n,), generator=gen)
    ids[:3] = torch.tensor([2 ** 31 - 1, n_seg, n_seg - 1])
    g = torch.randn(n_seg, c, generator=gen)
    ref, dx = _segment_ref(x, ids, n_seg, mode, g)
    xg = x.to(dev).requires_grad_()
    out = ops.scatter(xg, ids.to(dev), dim=0, reduce=mode, dim_size=n_seg)
    out.backward(g.to(dev))
    # (sums of ~80 rows, |sum| < 32: 4 x the measured fp32 CPU error of index_add_ at this shape, 5.0552e-06)
    assert _maxerr(out, ref) <= {"sum": 4 * 5.0552e-06, "mean": 1e-6, "max": 0.0}[mode]
    assert _maxerr(xg.grad, dx) <= 1e-6
    outside = (ids < 0) | (ids >= n_seg)
    assert int(outside.sum()) > 1000 and float(xg.grad[outside.to(dev)].abs().max()) == 0.0
    for idt, rows, segs in ((torch.full((n,), -1), n, n_seg), (ids[:0], 0, n_seg), (ids, n, 0)):
        xg = x[:rows].to(dev).requires_grad_()
        out = ops.scatter(xg, idt.to(dev), dim=0, reduce=mode, dim_size=segs)
        assert out.shape == (segs, c) and (segs == 0 or float(out.detach().abs().max()) == 0.0)
        out.backward(torch.ones_like(out))
        assert xg.grad.shape == (rows, c) and (rows == 0 or float(xg.grad.abs().max()) == 0.0)


def test_segment_max_with_infinities_and_ties(dev):
    """-inf inputs: a segment whose rows are all -inf in a channel reduces to -inf (only an EMPTY segment gives 0) and
    still routes its gradient to one row.  Duplicated rows tie in every channel: exactly one of the tied rows receives
    the gradient, it is the lowest-index one, and the tied rows' gradients sum to the upstream value."""
    from openseg3d_amd import ops
    gen = torch.Generator().manual_seed(11)
    n, c, n_seg = 4000, 6, 300
    x = torch.randn(n, c, generator=gen)
    ids = torch.randint(0, n_seg, (n,), generator=gen)
    ids[ids == 17] = 18
    x[torch.rand(n, c, generator=gen) < 0.2] = float("-inf")
    x[ids == 3] = float("-inf")
    x[ids == 4, 2] = float("-inf")
    dup = torch.nonzero(ids == 9)[:, 0]
    x[dup] = torch.randn(c, generator=gen)  # every row of segment 9 equal: a tie in all channels
    x[3000:] = x[1000:2000]                 # and a thousand duplicated rows spread over the segments
    ids[3000:] = ids[1000:2000]
    g = torch.randn(n_seg, c, generator=gen)
    ref, dx = _segment_ref(x, ids, n_seg, "max", g)
    xg = x.to(dev).requires_grad_()
    out = ops.segment_reduce(xg, ops.SegmentIndex(ids.to(dev), n_seg), ops.REDUCE_MAX)
    out.backward(g.to(dev))
    assert torch.equal(out.detach().cpu().double(), ref)
    assert bool((out[3] == float("-inf")).all()) and float(out[4, 2]) == float("-inf") and float(out[17].abs().max()) == 0.0
    assert torch.equal(xg.grad.cpu().double(), dx)
    got = xg.grad.cpu()
    dup = torch.nonzero(ids == 9)[:, 0]
    assert len(dup) > 2 and torch.equal(got[dup[0]], g[9]) and float(got[dup[1:]].abs().max()) == 0.0
    sums = torch.zeros(n_seg, c, dtype=torch.float64).index_add(0, ids, got.double())
    live = torch.bincount(ids, minlength=n_seg) > 0
    assert torch.equal(sums[live], g.double()[live])


@pytest.mark.parametrize("c", [6, 260])
def test_gather_rows_and_its_backward(dev, c):
    """out[i] = feats[ids[i]], zeros at -1: the scalar path (C = 6) and the float4 path at C = 260; exact.  The backward is
    the SUM reduce of d out over the rows that read each feature row (at most a handful here, |sum| < 16): within 1e-6
    like every gradient of these ops -- the float32 sum in ascending row order, evaluated on the CPU, is off by 5.7e-07
    (C = 6) and 8.3e-07 (C = 260).  A feature row nobody reads gets exactly 0.  Then no ids at all."""
    from openseg3d_amd import ops
    gen = torch.Generator().manual_seed(c)
    m, n = 3000, 5000
    feats = torch.randn(m, c, generator=gen)
    ids = torch.randint(-1, m - 500, (n,), generator=gen)
    g = torch.randn(n, c, generator=gen)
    fr = feats.double().requires_grad_()
    ok = ids >= 0
    ref = torch.zeros((n, c), dtype=torch.float64).index_add(0, torch.nonzero(ok)[:, 0], fr[ids[ok]])
    ref.backward(g.double())
    fg = feats.to(dev).requires_grad_()
    out = ops.gather_rows(fg, ids.to(dev))
    out.backward(g.to(dev))
    assert torch.equal(out.detach().cpu().double(), ref.detach())
    print("gather_rows", c, "dfeats", _maxerr(fg.grad, fr.grad))
    assert _maxerr(fg.grad, fr.grad) <= 1e-6
    assert float(fg.grad[m - 500:].abs().max()) == 0.0
    fg.grad = None
    out = ops.gather_rows(fg, ids[:0].to(dev))
    assert out.shape == (0, c)
    out.sum().backward()
    assert fg.grad.shape == (m, c) and float(fg.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ group_index and the scan
def _group_ref(ids, n_groups):
    """numpy: stable argsort of the ids in [0, n_groups) and the cumulative bincount."""
    ok = (ids >= 0) & (ids < n_groups)
    rows = np.nonzero(ok)[0]
    order = rows[np.argsort(ids[rows], kind="stable")]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(ids[rows], minlength=n_groups))]).astype(np.int64)
    rank = np.full(ids.shape[0], -1, dtype=np.int64)
    rank[order] = np.arange(order.shape[0]) - offsets[ids[order]]
    return rank, order, offsets


def _group_check(dev, ids, n_groups):
    from openseg3d_amd import ops
    rank, order, offsets = _group_ref(ids, n_groups)
    r, o, off = ops.group_index(torch.from_numpy(ids.astype(np.int32)).to(dev), n_groups)
    assert off.shape[0] == n_groups + 1 and r.shape[0] == o.shape[0] == ids.shape[0]
    assert np.array_equal(off.cpu().numpy(), offsets)
    assert np.array_equal(r.cpu().numpy(), rank)
    assert np.array_equal(o.cpu().numpy()[:order.shape[0]], order)


@pytest.mark.parametrize("n_groups", [1, 2047, 2048, 2049, 524289, 526337])
def test_group_index_and_scan_sizes(dev, n_groups):
    """The scan works on 2048-element chunks: one chunk short by one, exactly one, one plus an element; 524289 = 256 chunks
    plus an element, where the last workgroup's base is the sum of 256 chunk totals (one per thread); and 526337 = 257
    chunks plus an element, the first size at which a thread of the last workgroup adds a second chunk total (its base
    loop runs a second round).  About 600 000 ids, one in sixteen at -1 and as many at or above n_groups; for one group
    a third of the ids are in it (a 200 000-entry list ranked by counting)."""
    rs = np.random.RandomState(n_groups % 1000)
    n = 600011
    if n_groups == 1:
        ids = rs.randint(-1, 2, n)
    else:
        ids = rs.randint(0, n_groups, n)
        ids[rs.rand(n) < 1 / 16] = -1
        hi = rs.rand(n) < 1 / 16
        ids[hi] = n_groups + rs.randint(0, 3, int(hi.sum())) * 1000
        ids[:2] = (n_groups - 1, 0)  # both ends of the range are hit
    _group_check(dev, ids.astype(np.int64), n_groups)


def test_group_index_with_nothing_to_group(dev):
    """All ids at -1 (every rank -1, offsets all 0), and no ids at all with five groups (six zero offsets)."""
    from openseg3d_amd import ops
    _group_check(dev, np.full(5000, -1, dtype=np.int64), 300)
    r, o, off = ops.group_index(torch.zeros((0,), dtype=torch.int32, device=dev), 5)
    assert r.shape == o.shape == (0,) and off.cpu().tolist() == [0] * 6


# ------------------------------------------------------------------------------------------ span_mean, FlattenSELayer
def _span_ref(x, offsets, g, dtype):
    """mean of each span as first row + mean of (x - first row) -- se_layer.py:24-25 on contiguous samples -- in ``dtype``."""
    xr = x.detach().to(dtype).clone().requires_grad_()
    out, lo = [], 0
    for hi in offsets:
        out.append(xr[lo] + (xr[lo:hi] - xr[lo]).mean(dim=0) if hi > lo else xr.new_zeros(x.shape[1]))
        lo = hi
    ref = torch.stack(out)
    ref.backward(g.to(dtype))
    return ref.detach(), xr.grad


# 4 x the error of the fp32 CPU evaluation of _span_ref against its fp64 value, x = 1000 + randn (one float32 ulp at 1000
# is 6.1e-05: the last addition's rounding is all of it).  Measured per (C, case): see test_span_mean_matches_fp64
_SPAN_FWD_MEASURED = {(4, "one"): 0.0, (4, "three"): 2.1941e-05, (4, "tail"): 2.7466e-05,
                      (32, "one"): 0.0, (32, "three"): 3.0404e-05, (32, "tail"): 3.0518e-05,
                      (1024, "one"): 0.0, (1024, "three"): 3.0644e-05, (1024, "tail"): 3.0518e-05}
_SPAN_CASES = {"one": ([1], 0), "three": ([5, 0, 70001], 0), "tail": ([40, 300], 25)}


@pytest.mark.parametrize("case", ["one", "three", "tail"])
@pytest.mark.parametrize("c", [4, 32, 1024])
def test_span_mean_matches_fp64(dev, c, case):
    """Offsets [1]; [5, 5, 70006] (a short span, an empty one, and one long enough for every block of the column sum);
    [40, 340] with 25 rows behind the last offset.  x = 1000 + randn: summing x itself in float32 would lose the
    fraction, the shifted sums do not.  Forward bound: 4 x the fp32 CPU evaluation's error, _SPAN_FWD_MEASURED (0 for the
    one-row span, which is x[0] exactly on both sides; 2.2e-05 / 3.0e-05 / 3.1e-05 at [5, 5, 70006] and 2.7e-05 / 3.1e-05 /
    3.1e-05 with the tail at C = 4 / 32 / 1024: half a float32 ulp at 1000).  Backward: g[b] / rows is one float32 division of float32 operands, so at
    most two roundings (torch may multiply by the rounded reciprocal), 2 ** -24 relative each: 3 * 2 ** -24 covers both and
    their product term; exactly 0 behind the last offset."""
    from openseg3d_amd import ops
    rows, tail = _SPAN_CASES[case]
    offsets = np.cumsum(rows).tolist()
    gen = torch.Generator().manual_seed(c + len(rows))
    x = 1000.0 + torch.randn(offsets[-1] + tail, c, generator=gen)
    g = torch.randn(len(rows), c, generator=gen)
    ref, dx = _span_ref(x, offsets, g, torch.float64)
    xg = x.to(dev).requires_grad_()
    out = ops.span_mean(xg, offsets)
    out.backward(g.to(dev))
    err = _maxerr(out, ref)
    print("span_mean", c, case, "out", err, "dx", _maxerr(xg.grad, dx))
    assert err <= 4 * _SPAN_FWD_MEASURED[(c, case)]
    assert bool(((xg.grad.cpu().double() - dx).abs() <= 3 * 2.0 ** -24 * dx.abs()).all())
    if tail:
        assert float(xg.grad[offsets[-1]:].abs().max()) == 0.0


def test_span_mean_with_every_span_empty(dev):
    """A batch whose samples are all empty: zeros forward, and a backward that returns zeros of the input's shape."""
    from openseg3d_amd import ops
    for rows in (0, 3):
        x = torch.randn(rows, 32, device=dev, requires_grad=True)
        out = ops.span_mean(x, [0, 0])
        assert out.shape == (2, 32) and float(out.abs().max()) == 0.0
        out.backward(torch.randn(2, 32, device=dev))
        assert x.grad.shape == (rows, 32) and (rows == 0 or float(x.grad.abs().max()) == 0.0)


def _se_ref(x, w1, w2, rows, g, dtype, shifted=False):
    """se_layer.py:16-29 as torch in ``dtype``: mean per sample, fc (Linear, ReLU, Linear, Sigmoid), gate.  ``shifted``
    takes each mean as first row + mean of (x - first row), the form span_mean evaluates; in fp64 the two agree to 1e-14."""
    xr, a, b = (t.detach().to(dtype).clone().requires_grad_() for t in (x, w1, w2))
    idx = torch.repeat_interleave(torch.arange(len(rows)), torch.tensor(rows))
    if shifted:
        pooled, lo = [], 0
        for n in rows:
            pooled.append(xr[lo] + (xr[lo:lo + n] - xr[lo]).mean(dim=0) if n else xr.new_zeros(x.shape[1]))
            lo += n
        pooled = torch.stack(pooled)
    else:
        cnt = torch.tensor(rows, dtype=dtype).clamp(min=1)
        pooled = torch.zeros((len(rows), x.shape[1]), dtype=dtype).index_add(0, idx, xr) / cnt[:, None]
    gate = torch.sigmoid(torch.relu(pooled @ a.t()) @ b.t())
    out = xr * gate[idx]
    out.backward(g.to(dtype))
    return [out.detach(), xr.grad, a.grad, b.grad]


# fp32 CPU evaluation of _se_ref against its fp64 value at (C = 32, rows [257, 0, 1000]): output, d x, d fc[0].weight,
# d fc[2].weight, on one thread (torch's CPU index_put accumulates in thread order).  The row_offsets branch is measured
# in the form it evaluates (shifted=True).
_SE_MEASURED = {"index": (2.7896e-07, 2.7546e-07, 1.0196e-06, 1.3279e-06),
                "row_offsets": (2.8057e-07, 2.5674e-06, 2.0844e-06, 2.3965e-06)}


@pytest.mark.parametrize("branch", ["row_offsets", "index"])
def test_flatten_se_layer_matches_fp64(dev, branch):
    """FlattenSELayer over three samples of 257, 0 and 1000 rows (the index branch, whose segment count is the largest id
    + 1, sees the same batch): output, d x and both fc weight gradients against se_layer.py:16-29 in fp64.  Bounds: 4 x the
    fp32 CPU evaluation's error, _SE_MEASURED.  The row_offsets branch pools with span_mean, whose result is rounded at the
    size of the span's first row (|x| ~ 2), not of the mean (~0.1): the pooled rows are off by 4e-07 instead of 8e-08, and
    the weight gradients multiply that by |d z| ~ 18.  Held to the scatter-mean form's fp32 error (1.0e-06 and 1.3e-06 for
    the two weight gradients) that branch misses 4 x: it gave 5.46e-06 and 5.47e-06 on the device.  Its own form's fp32
    error is 2.1e-06 and 2.4e-06, and that is what it is held to."""
    from openseg3d_amd import segformer
    rows, c = [257, 0, 1000], 32
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(sum(rows), c, generator=gen)
    w1 = torch.randn(c // 4, c, generator=gen) * 0.3
    w2 = torch.randn(c, c // 4, generator=gen) * 0.3
    g = torch.randn(sum(rows), c, generator=gen)
    want = _se_ref(x, w1, w2, rows, g, torch.float64)
    se = segformer.FlattenSELayer(c).to(dev)
    with torch.no_grad():
        se.fc[0].weight.copy_(w1)
        se.fc[2].weight.copy_(w2)
    xg = x.to(dev).requires_grad_()
    idx = torch.repeat_interleave(torch.arange(len(rows)), torch.tensor(rows)).to(dev)
    out = se(xg, idx, np.cumsum(rows).tolist() if branch == "row_offsets" else None)
    out.backward(g.to(dev))
    got = [out, xg.grad, se.fc[0].weight.grad, se.fc[2].weight.grad]
    errs = [_maxerr(a, b) for a, b in zip(got, want)]
    print("FlattenSELayer", branch, "errors", errs)
    for name, err, measured in zip(("out", "dx", "dw1", "dw2"), errs, _SE_MEASURED[branch]):
        assert err <= 4 * measured, name


# ------------------------------------------------------------------------------------------ class counts of the losses
@pytest.mark.parametrize("c", [2, 64])
def test_criteria_at_the_class_count_limits(dev, c):
    """lovasz_softmax (classes='present' with classes missing from the labels, and 'all') and cross_entropy (OHEM threshold
    0.7, and plain) at 2 and 64 classes, 2049 rows (one past a chunk), against oracle.losses in fp64, with the assertions
    of test_criterion_matches_oracle_at_size; upstream gradient 0.4."""
    from oracle import losses as L
    from openseg3d_amd import ops
    n = 2049
    gen = torch.Generator().manual_seed(c)
    x = torch.randn(n, c, generator=gen) * 2.5
    present = 1 if c == 2 else 40  # labels use the first `present` classes only
    y = torch.randint(0, present, (n,), generator=gen)
    y[torch.rand(n, generator=gen) < 0.1] = 255
    cases = (("lovasz present", lambda t, lab: ops.lovasz_softmax(t, lab, 255, "present"),
              lambda t: L.lovasz_softmax(t, y, classes="present")),
             ("lovasz all", lambda t, lab: ops.lovasz_softmax(t, lab, 255, "all"), lambda t: L.lovasz_softmax(t, y, classes="all")),
             ("ohem 0.7", lambda t, lab: ops.cross_entropy(t, lab, 255, 0.7), lambda t: L.ohem_cross_entropy(t, y, 0.7)),
             ("plain ce", lambda t, lab: ops.cross_entropy(t, lab, 255), lambda t: L.ohem_cross_entropy(t, y, None)))
    for name, fn_dev, fn_ref in cases:
        xr = x.double().requires_grad_(True)
        lr = fn_ref(xr)
        (lr * 0.4).backward()
        assert bool(torch.isfinite(lr)), name
        xg = x.to(dev).requires_grad_(True)
        lg = fn_dev(xg, y.to(dev))
        (lg * 0.4).backward()
        err = _maxerr(xg.grad, xr.grad)
        print("criterion", c, name, float(lg), float(lr), "grad", err)
        assert abs(float(lg) - float(lr)) <= 1e-5 * max(abs(float(lr)), 1e-3), (name, float(lg), float(lr))
        assert err <= 1e-9 + 2e-4 * float(xr.grad.abs().max()), (name, err)
