"""fp64 restatements of the two attention modes beside the shared-tau cosine one (attn_ref.reference): per-head tau
(cosine_msa.py:156-160 with tau [1, H, 1, 1]) and scaled dot product (cosine_msa.py:163-165), evaluated per window and head
from the CSR as attn_ref.reference does, with the optional dropout factors of dropout_ref.dropout_factors.  Shared by
test_attn_modes_host.py (against the reference module's own numbers, tests/golden/attn_modes.npz) and
test_gpu_attention_modes.py (the yardstick of the kernels)."""
import collections
import math

import torch

# what the restatement reads of a window index: token rows in CSR order, first slot and token count per window
HostCSR = collections.namedtuple("HostCSR", "tok win_start win_count n_windows")


def host_csr(sizes, perm=None):
    """A CSR over sum(sizes) flat rows without a device: window w holds sizes[w] tokens; perm (optional) = the flat row of
    every token slot, i.e. any ragged layout (default: slot i is row i)."""
    total = int(sum(sizes))
    tok = torch.arange(total) if perm is None else torch.as_tensor(perm, dtype=torch.long)
    starts = torch.tensor([0] + list(sizes[:-1]), dtype=torch.long).cumsum(0)
    return HostCSR(tok, starts, torch.tensor(list(sizes), dtype=torch.long), len(sizes))


def _csr(wi):
    tok = wi.tok.cpu().long()
    return tok, wi.win_start[: wi.n_windows].cpu().tolist(), wi.win_count[: wi.n_windows].cpu().tolist()


def scores(qk, tau, tau_min, heads, rows, h):
    """[n, n] pre-softmax scores of head h on the flat rows of one window: cosine / max(tau_h, tau_min), or, with tau None,
    q.k / sqrt(dh)."""
    c = qk.shape[1] // 2
    dh = c // heads
    sl = slice(h * dh, (h + 1) * dh)
    qh, kh = qk[rows][:, sl], qk[rows][:, c + h * dh:c + (h + 1) * dh]
    if tau is None:
        return (qh / math.sqrt(dh)) @ kh.t()
    t = tau.reshape(-1)
    t_h = t[h] if t.numel() > 1 else t[0]
    qh = torch.nn.functional.normalize(qh, dim=-1, eps=1e-12)
    kh = torch.nn.functional.normalize(kh, dim=-1, eps=1e-12)
    return qh @ kh.t() / torch.clamp(t_h, min=tau_min)


def reference(qk, v, tau, tau_min, heads, wi, keep=None):
    """qk [m, 2C] (q | k), v [m, C]; tau: 1 element, `heads` elements, or None (dot product).  One (window, head) at a time in
    the dtype of the inputs; keep[(w, h)] = optional [n, n] dropout factors (0 or 1 / keep_prob).  Differentiable."""
    m, c = v.shape
    dh = c // heads
    tok, starts, counts = _csr(wi)
    out = torch.zeros(m, c, dtype=v.dtype)
    pieces = []
    for w, (s, n) in enumerate(zip(starts, counts)):
        rows = tok[s:s + n]
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            p = torch.softmax(scores(qk, tau, tau_min, heads, rows, h), dim=-1)
            if keep is not None:
                p = p * keep[(w, h)].to(p.dtype)
            pieces.append((rows, sl, p @ v[rows][:, sl]))
    for rows, sl, o in pieces:
        out[rows, sl] = out[rows, sl] + o  # index_put on disjoint (rows, head) blocks: differentiable
    return out


def score_extent(qk, heads, wi):
    """S_abs = max |q_i| |k_j| / sqrt(dh) over same-window pairs and heads (the dot mode's counterpart of 1 / tau)."""
    c = qk.shape[1] // 2
    dh = c // heads
    tok, starts, counts = _csr(wi)
    best = 0.0
    for s, n in zip(starts, counts):
        rows = tok[s:s + n]
        qn = qk[rows][:, :c].reshape(n, heads, dh).norm(dim=-1).max(dim=0).values
        kn = qk[rows][:, c:].reshape(n, heads, dh).norm(dim=-1).max(dim=0).values
        best = max(best, float((qn * kn).max()) / math.sqrt(dh))
    return best


def module_forward(x, pos, w_in, b_in, w_out, b_out, tau, tau_min, heads, wi):
    """CosineMultiheadAttention on flat rows: q = k = (x + pos) W_qk, v = x W_v (cosine_msa.py:58-63), the core above, the
    out-projection."""
    c = x.shape[1]
    qk = (x + pos) @ w_in[: 2 * c].t() + b_in[: 2 * c]
    v = x @ w_in[2 * c:].t() + b_in[2 * c:]
    return reference(qk, v, tau, tau_min, heads, wi) @ w_out.t() + b_out
