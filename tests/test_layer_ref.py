"""The encoder-layer tests' own fp64 reference (layer_ref.py) is itself checked (no GPU): without dropout and DropPath it equals
oracle.window.encoder_layer, the padded-window restatement every golden file was made with, forward and every gradient; and
the training-mode extras obey their invariants (neutral factors change nothing, a dropped row passes through)."""
import types

import numpy as np
import pytest
import torch

import layer_ref
import refcfg
from oracle import params as oracle_params
from oracle import window as W

C, HEADS = 48, 8
PREFIX = "layers.0."


def _index_from(win):
    """The CSR of the non-empty windows of a per-voxel window id, shaped like ops.WindowIndex as far as the references read
    it (windows in ascending id, tokens in flat order)."""
    tok = torch.argsort(win, stable=True)
    _, counts = torch.unique(win, sorted=True, return_counts=True)
    starts = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)[:-1]])
    return types.SimpleNamespace(tok=tok, win_start=starts, win_count=counts, n_windows=int(counts.shape[0]))


@pytest.fixture(scope="module")
def case():
    rs = np.random.RandomState(0)
    # 160 voxels on a 30 x 30 x 12 corner of the canvas: a dozen windows of 1 .. ~40 tokens, plus one voxel on a cell of its own
    zyx = np.unique(np.stack([rs.randint(0, 12, 160), rs.randint(0, 30, 160), rs.randint(0, 30, 160)], 1), axis=0)
    zyx = np.concatenate([zyx, [[3, 55, 55]]], 0)[rs.permutation(zyx.shape[0] + 1)]
    coords = torch.from_numpy(np.concatenate([np.zeros((zyx.shape[0], 1), np.int64), zyx], 1))
    info = W.window_partition(coords, refcfg.BATCHING_INFO[0], refcfg.WINDOW_SHAPE, np.array([60.0, 60.0, 16.0]), C)
    wi = _index_from(info["batch_win_inds_shift0"])
    counts = wi.win_count.tolist()
    assert 1 in counts and max(counts) > 16 and len(counts) > 8
    m = coords.shape[0]
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(m, C, generator=gen, dtype=torch.float64)
    g = torch.randn(m, C, generator=gen, dtype=torch.float64)
    p = {k: v.double() for k, v in oracle_params.state_dict_for(refcfg.swformer_param_shapes(C, 1), 3).items()}
    return types.SimpleNamespace(info=info, wi=wi, m=m, x=x, g=g, p=p, pos=info["pos_flat_shift0"].double())


def _leaves(case):
    x = case.x.clone().requires_grad_()
    p = {k: v.clone().requires_grad_() for k, v in case.p.items()}
    return x, p


def _run(case, g=None, **kw):
    x, p = _leaves(case)
    y = layer_ref.encoder_layer(x, case.pos, p, PREFIX, HEADS, case.wi, **kw)
    y.backward(case.g if g is None else g)
    return y.detach(), x.grad, {k: v.grad for k, v in p.items()}


def _close(a, b, rel):
    return float((a - b).abs().max()) <= rel * max(1.0, float(b.abs().max()))


def test_plain_layer_equals_the_padded_window_oracle(case):
    y, dx, dp = _run(case)
    x, p = _leaves(case)
    info = case.info
    pos_dict = {k: v.double() for k, v in info["pos_dict_shift0"].items()}
    want = W.encoder_layer(x, pos_dict, info["flat2win_inds_shift0"], info["key_mask_shift0"], p, PREFIX, HEADS)
    want.backward(case.g)
    assert _close(y, want.detach(), 1e-10)
    assert _close(dx, x.grad, 1e-10)
    assert set(dp) == {PREFIX + n for n in layer_ref.PARAM_NAMES} == set(p)
    for k in p:
        assert float(p[k].grad.abs().max()) > 0.0, k
        assert _close(dp[k], p[k].grad, 1e-10), k


def test_neutral_mask_and_factors_change_nothing(case):
    y0, dx0, dp0 = _run(case)
    keep = {(w, h): torch.ones(n, n, dtype=torch.float64) for w, n in enumerate(case.wi.win_count.tolist()) for h in range(HEADS)}
    ones = torch.ones(case.m, dtype=torch.float64)
    y1, dx1, dp1 = _run(case, keep=keep, s1=ones, s2=ones)
    assert torch.equal(y0, y1)
    assert _close(dx1, dx0, 1e-12)
    for k in dp0:
        assert _close(dp1[k], dp0[k], 1e-12), k


def test_keep_factors_follow_the_window_order(case):
    keep = layer_ref.keep_factors(case.wi, HEADS, 0.1, 77)
    counts = case.wi.win_count.tolist()
    assert set(keep) == {(w, h) for w in range(len(counts)) for h in range(HEADS)}
    assert all(tuple(keep[(w, h)].shape) == (n, n) for w, n in enumerate(counts) for h in range(HEADS))
    vals = torch.cat([k.reshape(-1) for k in keep.values()])
    assert set(vals.unique().tolist()) == {0.0, 256.0 / 230.0}  # p = 0.1: 26 of 256 byte values drop
    assert 0.07 < float((vals == 0).double().mean()) < 0.13
    assert layer_ref.keep_factors(case.wi, HEADS, 0.0, 77) is None


def test_a_dropped_row_passes_through(case):
    """s1 = s2 = 0 on a row: its output is its input, and its input gradient is the upstream gradient plus only what reaches
    it as a key / value of the other rows of its window."""
    wi = case.wi
    counts, starts = wi.win_count.tolist(), wi.win_start.tolist()
    big = int(np.argmax(counts))
    r_multi = int(wi.tok[starts[big] + 2])            # a row among many in its window
    r_single = int(wi.tok[starts[counts.index(1)]])   # alone in its window
    keep = layer_ref.keep_factors(wi, HEADS, 0.1, 5)
    gen = torch.Generator().manual_seed(2)
    s1 = (torch.rand(case.m, generator=gen) < 0.8).double() / 0.8
    s2 = (torch.rand(case.m, generator=gen) < 0.8).double() / 0.8
    for r in (r_multi, r_single):
        s1[r] = s2[r] = 0.0
    y, dx, _ = _run(case, keep=keep, s1=s1, s2=s2)
    for r in (r_multi, r_single):
        assert torch.equal(y[r], case.x[r])
        # upstream gradient on that row alone: it comes back unchanged and reaches nothing else
        g_r = torch.zeros_like(case.g)
        g_r[r] = case.g[r]
        _, dx_r, dp_r = _run(case, g=g_r, keep=keep, s1=s1, s2=s2)
        assert torch.equal(dx_r, g_r)
        assert all(float(v.abs().max()) == 0.0 for v in dp_r.values())
        # upstream gradient on every other row: what they send to row r through the attention
        g_o = case.g.clone()
        g_o[r] = 0.0
        _, dx_o, _ = _run(case, g=g_o, keep=keep, s1=s1, s2=s2)
        assert _close(dx[r], case.g[r] + dx_o[r], 1e-12)
    assert float((dx[r_multi] - case.g[r_multi]).abs().max()) > 1e-6
    assert torch.equal(dx[r_single], case.g[r_single])


def test_block_threads_shift_mask_and_factors(case):
    """block() = the layers in sequence, layer i with shift 0 if i < depth // 2 else 1, keeps[i], scales[2 i], scales[2 i + 1]."""
    depth = 3
    p = {k: v.double() for k, v in oracle_params.state_dict_for(refcfg.swformer_param_shapes(C, depth), 4).items()}
    index = [case.wi, _index_from(case.info["batch_win_inds_shift1"])]
    pos = [case.pos, case.info["pos_flat_shift1"].double()]
    assert not torch.equal(index[0].tok, index[1].tok)
    # eval: the padded-window oracle's block
    y = layer_ref.block(case.x, pos, index, p, depth, HEADS, None, None)
    assert _close(y, W.swformer_block(case.x, case.info, p, "", depth, HEADS), 1e-10)
    # training: the same chain written out
    gen = torch.Generator().manual_seed(6)
    scales = [None, None] + [(torch.rand(case.m, generator=gen) < 0.7).double() / 0.7 for _ in range(4)]
    keeps = [layer_ref.keep_factors(index[0 if i < 1 else 1], HEADS, 0.1, 900 + i) for i in range(depth)]
    y = layer_ref.block(case.x, pos, index, p, depth, HEADS, keeps, scales)
    want = case.x
    for i, s in enumerate((0, 1, 1)):
        want = layer_ref.encoder_layer(want, pos[s], p, f"layers.{i}.", HEADS, index[s], keep=keeps[i], s1=scales[2 * i],
                                       s2=scales[2 * i + 1])
    assert torch.equal(y, want)
