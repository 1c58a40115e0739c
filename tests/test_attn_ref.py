"""The attention tests' own fp64 references agree with each other (no GPU): the batched-by-window-size form used for the
thousand-window base sets against the per-(window, head) loop every other attention test is held to."""
import types

import numpy as np
import torch

from attn_ref import reference, reference_grouped


def _fake_index(sizes, seed):
    """A window CSR over shuffled rows, shaped like ops.WindowIndex as far as the references read it."""
    rs = np.random.RandomState(seed)
    counts = np.asarray(sizes)[rs.permutation(len(sizes))]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return types.SimpleNamespace(tok=torch.from_numpy(rs.permutation(int(counts.sum()))), win_start=torch.from_numpy(starts),
                                 win_count=torch.from_numpy(counts), n_windows=len(sizes))


def test_grouped_reference_equals_the_loop():
    sizes = [1 + i % 5 for i in range(40)] + [33, 33, 64, 7]
    wi = _fake_index(sizes, 0)
    m, heads, dh = sum(sizes), 4, 6
    c = heads * dh
    gen = torch.Generator().manual_seed(0)
    qk = torch.randn(m, 2 * c, generator=gen, dtype=torch.float64)
    qk[3] *= 1e-3
    v = torch.randn(m, c, generator=gen, dtype=torch.float64)
    g = torch.randn(m, c, generator=gen, dtype=torch.float64)
    got = []
    for fn in (reference, reference_grouped):
        for tau in (0.2, 0.004):  # 0.004: below tau_min, clamped
            leaves = [qk.clone().requires_grad_(), v.clone().requires_grad_(), torch.full((1, 1, 1), tau, dtype=torch.float64, requires_grad=True)]
            out = fn(leaves[0], leaves[1], leaves[2], 0.01, heads, wi)
            out.backward(g)
            got.append([out.detach()] + [t.grad for t in leaves])
    for a, b in zip(got[:2], got[2:]):
        for x, y in zip(a, b):
            assert float((x - y).abs().max()) <= 1e-12 * max(1.0, float(x.abs().max()))
    assert float(got[0][3].abs().max()) > 0 and float(got[1][3].abs().max()) == 0.0
