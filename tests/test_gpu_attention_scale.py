"""Window attention against fp64 where the persistent schedule really runs: forward workgroups that walk several and several
hundred work units (the persistent loop, the next-item prefetch, both refills of the descriptor ring), XCD blocks of 8 / 4 / 1
items with a partial last block, backward grids with padded last groups, and thousands of tau partials -- every case asserts
its regime through seg3d_window_attn_schedule, i.e. through the launchers' own arithmetic.

The item counts come from many small windows, not from many tokens.  Families A and B replicate a small base set of windows
onto other window cells; replica r is scaled by exact powers of two unique to it (v by a, q by b, k by c, the upstream gradient
by e, drawn from {1/2, 1, 2, 4}^3 x {1, 2}).  Cosine scores do not change, so out_r = a out_b, dv_r = e dv_b, dq_r = (a e / b)
dq_b, dk_r = (a e / c) dk_b and dtau = sum_r a_r e_r dtau_b, all exactly: ONE fp64 reference (forward and autograd) of the base
set serves every replica, and a replica computed from another replica's rows is wrong by O(100 %).  The large tensors are
gathered and scaled on the device and compared there in float64.  Family C is independent random data with dropout and a
direct reference with one tau leaf per replica.

Bars (all from test_gpu_attention.py, none new; f = max(1, 0.1 / max(tau, 0.01))): forward 2e-5 f max|v| (3e-5 max|v| with
dropout at tau 0.5), dv and dqk 3e-4 f max(1, max|want|) -- row-local, applied to every replica after un-scaling, so the size
does not enter -- and dtau, one number with 10^3 - 10^4-fold cancellation, the SUM over replicas of the bar each replica
would get alone: sum_r a_r e_r 2e-3 f max(1, |dtau_b|) (A / B), sum_r 2e-3 f max(1, |dtau_r|) (C).

Measured on an MI355X (256 CUs): see RESULTS at the end of this docstring.

RESULTS
  case                     windows / tiles / chunks   forward      J  blk  bwd wgs   fwd    dv     dqk    dtau     s
  A R=10 dh=24 tau=0.2        220 /    910 /    350   fused        4   1    2816   0.227  0.015  0.020  0.033    0.3
  A R=10 dh=48 tau=0.2        220 /    910 /    350   fused        6   1    2816   0.289  0.017  0.039  0.002    0.3
  A R=17 dh=6 tau=0.02        374 /   1547 /    595   fused        4   8    1547   0.917  0.083  0.112  0.003    0.1
  A R=17 dh=6 tau=0.2         374 /   1547 /    595   fused        4   8    1547   0.289  0.035  0.021  0.022    0.1
  A R=17 dh=12 tau=0.02       374 /   1547 /    595   fused        5   8    3200   0.732  0.040  0.014  0.226    0.2
  A R=17 dh=12 tau=0.2        374 /   1547 /    595   fused        5   8    3200   0.257  0.028  0.024  0.010    0.2
  A R=17 dh=24 tau=0.02       374 /   1547 /    595   fused        7   4    4864   0.531  0.027  0.017  0.008    0.2
  A R=17 dh=24 tau=0.2        374 /   1547 /    595   fused        7   4    4864   0.227  0.015  0.020  0.033    0.0
  A R=17 dh=48 tau=0.02       374 /   1547 /    595   fused       10   4    4864   0.363  0.023  0.020  0.005    0.3
  A R=17 dh=48 tau=0.2        374 /   1547 /    595   fused       10   4    4864   0.289  0.017  0.039  0.002    0.0
  B R=115 dh=12 tau=0.2    115000 / 115000 / 115000   fused      300   8  230016   0.483  0.030  0.038  0.011    0.1
  B R=39 dh=24 tau=0.2      39000 /  39000 /  39000   fused      407   4  312064   0.484  0.044  0.028  0.000    0.1
  C dh=6 p=0.1 tau=0.5        128 /    512 /    192   vector-ALU   1   1     512   0.002  0.001  0.002  0.000    0.8
  C dh=12 p=0.1 tau=0.5       128 /    512 /    192   fused        2   8    1024   0.041  0.018  0.040  0.001    0.9
  C dh=24 p=0.1 tau=0.5       128 /    512 /    192   fused        2   1    1536   0.032  0.020  0.012  0.001    1.3
  C dh=48 p=0.1 tau=0.5       128 /    512 /    192   fused        3   1    1536   0.025  0.015  0.008  0.001    1.6
(forward = kernel the query reports; J = most units one forward workgroup walks; blk = items per XCD block; bwd wgs = workgroups of
a backward pass, padding included; fwd / dv / dqk / dtau = worst error over its bar; s = wall time of the case, the first use of a
base reference included.  The 16 cases take 6.5 s together; this module, test_gpu_attention.py, test_gpu_layer.py and the whole-model
gradient test ran in 43 s, 68 passed.)
With the tau gradient accumulated as sum dS * S, as it was before this module, dtau stood at 2.64 (A R=17 dh=12 tau=0.02) and, on
another draw of the base set, at 1.15 (dh=6 tau=0.02) of its bar; it is now sum dS * (S - LSE + log2 n).
"""
import math
import time
import types

import numpy as np
import pytest
import torch

import attn_ref
from attn_ref import HALF_TILE_SIZES, WINDOW_SIZES, reference, reference_grouped, schedule, schedule_of, windows_of
from dropout_ref import dropout_factors

pytestmark = pytest.mark.gpu

HEADS, TAU_MIN = 8, 0.01
BASE_A = WINDOW_SIZES + HALF_TILE_SIZES            # 22 windows, 2 537 tokens, 91 tiles, 35 chunks
BASE_B = [1 + i % 5 for i in range(1000)]          # 1 000 windows, 3 000 tokens, one tile / chunk each


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _tiles(sizes):
    return sum(-(-n // 32) for n in sizes), sum(-(-n // 128) for n in sizes)


def _scalings(n_rep, seed):
    """[n_rep, 4] float64 (a, b, c, e): the 128 tuples of {1/2, 1, 2, 4}^3 x {1, 2} in a random order, unique per replica up to
    128 replicas (then cycling: replicas 128 apart share a tuple)."""
    vals = np.array([0.5, 1.0, 2.0, 4.0])
    idx = np.random.RandomState(seed).permutation(128)[np.arange(n_rep) % 128]
    return torch.from_numpy(np.stack([vals[idx % 4], vals[(idx // 4) % 4], vals[(idx // 16) % 4], 1.0 + (idx // 64)], axis=1))


_PLANS, _REFS = {}, {}


def _plan(dev, key, sizes, seed):
    if key not in _PLANS:
        _PLANS.clear()  # the large plans hold device buffers: keep one at a time (cases are ordered by plan)
        _PLANS[key] = windows_of(dev, sizes, seed=seed)
    return _PLANS[key]


def _base(dev, name, sizes, dh, tau):
    """Base windows, their fp64 inputs and the fp64 forward / autograd, computed once per (family, dh, tau)."""
    key = (name, dh, tau)
    if key not in _REFS:
        ws = windows_of(dev, sizes, seed=1)
        c = HEADS * dh
        gen = torch.Generator().manual_seed(7000 + dh * 10 + int(tau * 1000))
        qk = torch.randn(ws.m, 2 * c, generator=gen, dtype=torch.float64)
        qk[5] *= 1e-3   # short and long rows exercise the normalisation
        qk[7] *= 40.0
        v = torch.randn(ws.m, c, generator=gen, dtype=torch.float64) * 1.5
        g = torch.randn(ws.m, c, generator=gen, dtype=torch.float64)
        qk_r, v_r = qk.clone().requires_grad_(), v.clone().requires_grad_()
        tau_r = torch.full((1, 1, 1), tau, dtype=torch.float64, requires_grad=True)
        ref = (reference_grouped if len(sizes) > 100 else reference)(qk_r, v_r, tau_r, TAU_MIN, HEADS, ws.wi)
        ref.backward(g)
        _REFS[key] = (ws, qk, v, g, ref.detach(), qk_r.grad, v_r.grad, float(tau_r.grad))
    return _REFS[key]


def _replica_rows(ws_b, ws, n_base):
    """For every flat row of the replicated set: its replica and the base row it stands for (window i of the replicated list is
    base window i % n_base of replica i // n_base; within a window the CSR orders pair the rows up -- any pairing will do, the
    operation is symmetric in a window's tokens)."""
    counts, starts = torch.tensor(ws.counts), torch.tensor(ws.starts)
    win_of_slot = torch.repeat_interleave(torch.arange(len(ws.counts)), counts)
    pos = torch.arange(ws.m) - starts[win_of_slot]
    listed = ws.which[win_of_slot]
    start_b = torch.empty(n_base, dtype=torch.long)
    start_b[ws_b.which] = torch.tensor(ws_b.starts)
    rep, base_row = torch.empty(ws.m, dtype=torch.long), torch.empty(ws.m, dtype=torch.long)
    rep[ws.tok] = listed // n_base
    base_row[ws.tok] = ws_b.tok[start_b[listed % n_base] + pos]
    return rep, base_row, listed


def _ratio(err, bar):
    return float(err) / float(bar)


def _run_replicated(dev, name, sizes_b, n_rep, dh, tau, plan_seed):
    """One replicated case: returns the worst error / bar of (forward, dv, dqk, dtau) and the plan."""
    from openseg3d_amd import ops
    ws_b, qk_b, v_b, g_b, out_b, dqk_b, dv_b, dtau_b = _base(dev, name, sizes_b, dh, tau)
    n_base, c = len(sizes_b), HEADS * dh
    ws = _plan(dev, (name, n_rep), list(sizes_b) * n_rep, plan_seed)
    rep, base_row, listed = _replica_rows(ws_b, ws, n_base)
    s = _scalings(n_rep, seed=n_rep)
    # 128 distinct tuples: beyond that replicas would share one, and on random cells some neighbours of the item list would too.
    # A device whose cap needs more (the descriptor-ring case at dh 12 on more than about 280 CUs) needs a placement that keeps the
    # item list's neighbours apart before this test can speak for it
    assert n_rep <= 128, f"{n_rep} replicas: more than the 128 distinct scaling tuples"
    s_d, rep_d, row_d = s.to(dev), rep.to(dev), base_row.to(dev)
    a, b, cc, e = (s_d[:, i][rep_d][:, None] for i in range(4))
    qk_bd, v_bd, g_bd = qk_b.to(dev), v_b.to(dev), g_b.to(dev)
    # power-of-two factors commute with the rounding to float32: the GPU's inputs are exactly scaled copies of the base's
    qk_g = torch.cat([qk_bd[row_d, :c] * b, qk_bd[row_d, c:] * cc], dim=1).float().requires_grad_()
    v_g = (v_bd[row_d] * a).float().requires_grad_()
    g_g = (g_bd[row_d] * e).float()
    tau_g = torch.full((1, 1, 1), tau, device=dev, requires_grad=True)
    out = ops.window_attention_packed(qk_g, v_g, tau_g, TAU_MIN, HEADS, ws.wi)
    out.backward(g_g)
    f = max(1.0, 0.1 / max(tau, TAU_MIN))
    worst = {}
    worst["fwd"] = _ratio((out.detach().double() / a - out_b.to(dev)[row_d]).abs().max(), 2e-5 * f * float(v_b.abs().max()))
    worst["dv"] = _ratio((v_g.grad.double() / e - dv_b.to(dev)[row_d]).abs().max(), 3e-4 * f * max(1.0, float(dv_b.abs().max())))
    dqk = qk_g.grad.double()
    dqk = torch.cat([dqk[:, :c] * (b / (a * e)), dqk[:, c:] * (cc / (a * e))], dim=1)
    worst["dqk"] = _ratio((dqk - dqk_b.to(dev)[row_d]).abs().max(), 3e-4 * f * max(1.0, float(dqk_b.abs().max())))
    weight = float((s[:, 0] * s[:, 3]).sum())  # sum_r a_r e_r
    worst["dtau"] = _ratio(abs(float(tau_g.grad.double()) - weight * dtau_b), weight * 2e-3 * f * max(1.0, abs(dtau_b)))
    return worst, ws


def _record(case, ws, sch, worst, t0):
    line = (f"{case}: {len(ws.counts)} windows {ws.m} tokens {ws.wi.n_tiles} tiles {ws.wi.n_qgroups} chunks | kernel {sch.kernel} "
            f"cap {sch.cap} grid {sch.grid} J {sch.walked} block {sch.xcd_block} bwd {sch.bwd_blocks} | "
            + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" | {time.time() - t0:.1f} s")
    print("\n" + line)


def _replicas_for(base_sizes, dh, want_walked, start, fits=lambda r: True):
    """Fewest replicas >= start whose forward walks at least want_walked units per workgroup on THIS device (the query holds the
    device's CU count) and that `fits`."""
    tiles, chunks = _tiles(base_sizes)
    r = start
    while schedule(r * tiles, r * chunks, HEADS, dh).walked < want_walked or not fits(r):
        r += 1
        assert r * len(base_sizes) <= math.prod(attn_ref.n_cells()), "more windows than window cells"
    return r


# ------------------------------------------------------------------ A: persistent loop, blocked item order, ragged ends
# (R = 17: 1 547 tiles, 595 chunks -- wide heads on blocks of 4, 1 547 % 8 = 3 and 595 % 4 = 3: the last XCD block is partial;
#  R = 10: 350 chunks -- wide heads on single items, still over the cap, 350 % 8 = 6 pads the backward's last group)
A_CASES = [(17, dh, tau) for tau in (0.2, 0.02) for dh in (6, 12, 24, 48)] + [(10, 24, 0.2), (10, 48, 0.2)]


@pytest.mark.parametrize("n_rep,dh,tau", sorted(A_CASES))
def test_persistent_loop_and_blocked_order_vs_fp64(dev, n_rep, dh, tau):
    t0 = time.time()
    tiles, chunks = _tiles(BASE_A)
    assert (len(BASE_A), sum(BASE_A), tiles, chunks) == (22, 2537, 91, 35)
    narrow = dh <= 12
    if n_rep == 17:  # blocks of 8 tiles / 4 chunks, a partial last block, J >= 3; more replicas only where a device needs them
        n_rep = _replicas_for(BASE_A, dh, 3, 17, lambda r: r * chunks >= 512 and (r * tiles) % 8 and (r * chunks) % 4)
    worst, ws = _run_replicated(dev, "A", BASE_A, n_rep, dh, tau, plan_seed=2)
    sch = schedule_of(ws.wi, HEADS, dh)
    assert (ws.wi.n_tiles, ws.wi.n_qgroups) == (n_rep * tiles, n_rep * chunks)
    assert sch.kernel == attn_ref.FUSED and sch.walked >= 3 and sch.grid >= sch.cap
    assert sch.xcd_block == (8 if narrow else 4 if ws.wi.n_qgroups >= 512 else 1)
    if n_rep == 10:
        assert not narrow and sch.xcd_block == 1 and ws.wi.n_qgroups % 8 == 6
    else:
        assert ws.wi.n_qgroups >= 512 and (ws.wi.n_tiles if narrow else ws.wi.n_qgroups) % sch.xcd_block
    n_items = ws.wi.n_tiles if narrow else ws.wi.n_qgroups
    assert sch.bwd_blocks > n_items * (HEADS // (4 if narrow else 1)) or dh == 6   # the fused backward's last group is padded
    _record(f"A R={n_rep} dh={dh} tau={tau}", ws, sch, worst, t0)
    assert max(worst.values()) < 1.0, worst


# ------------------------------------------------------------------ B: descriptor ring
# kDescRing = 256 descriptors per workgroup; the j = 128 refill writes descriptors 256 .. 383 (consumed only when J > 256), the
# j = 256 refill writes 384 .. 511 into the ring's other half (consumed when J > 384)
@pytest.mark.parametrize("dh,want_walked", [(12, 300), (24, 400)])
def test_descriptor_ring_refills_vs_fp64(dev, dh, want_walked):
    t0 = time.time()
    assert _tiles(BASE_B) == (1000, 1000) and sum(BASE_B) == 3000
    n_rep = _replicas_for(BASE_B, dh, want_walked, 1)
    worst, ws = _run_replicated(dev, "B", BASE_B, n_rep, dh, 0.2, plan_seed=3)
    sch = schedule_of(ws.wi, HEADS, dh)
    assert ws.wi.n_dropped == 0 and ws.wi.n_tiles == ws.wi.n_qgroups == 1000 * n_rep
    assert sch.kernel == attn_ref.FUSED and sch.walked >= want_walked and sch.grid >= sch.cap
    _record(f"B R={n_rep} dh={dh} tau=0.2", ws, sch, worst, t0)
    assert max(worst.values()) < 1.0, worst


# ------------------------------------------------------------------ C: dropout on the persistent forward and at backward scale
C_REPLICAS, C_P, C_TAU, C_SEED = 16, 0.1, 0.5, 0x0BAD_5EED_1234_5678


@pytest.mark.parametrize("dh", [6, 12, 24, 48])
def test_dropout_at_scale_vs_fp64(dev, dh):
    from openseg3d_amd import ops
    t0 = time.time()
    n_base, c = len(HALF_TILE_SIZES), HEADS * dh
    ws = _plan(dev, ("C", C_REPLICAS), HALF_TILE_SIZES * C_REPLICAS, 4)
    wi, m = ws.wi, ws.m
    assert (len(ws.counts), m, wi.n_tiles, wi.n_qgroups) == (128, 14400, 512, 192)
    sch = schedule_of(wi, HEADS, dh, C_P)
    if dh == 6:
        assert sch.kernel == attn_ref.VECTOR_ALU and sch.bwd_blocks == 512   # tau_reduce_small over 512 partials
    else:
        assert sch.kernel == attn_ref.FUSED and sch.walked >= 2
    gen = torch.Generator().manual_seed(300 + dh)
    qk = torch.randn(m, 2 * c, generator=gen, dtype=torch.float64)
    v = torch.randn(m, c, generator=gen, dtype=torch.float64)
    g = torch.randn(m, c, generator=gen, dtype=torch.float64)
    # the direct reference, one replica at a time on that replica's rows (a window index of its own over local rows, the
    # masks of the windows' numbers in the FULL index): every replica has its own tau leaf, and the loop's index_puts stay small
    ref, dqk_w, dv_w, want_r = torch.zeros(m, c, dtype=torch.float64), torch.zeros(m, 2 * c, dtype=torch.float64), \
        torch.zeros(m, c, dtype=torch.float64), torch.zeros(C_REPLICAS, dtype=torch.float64)
    for r in range(C_REPLICAS):
        wins = [w for w in range(len(ws.counts)) if int(ws.which[w]) // n_base == r]
        rows = torch.cat([attn_ref.rows_of(ws, w) for w in wins])
        cnt = torch.tensor([ws.counts[w] for w in wins])
        sub = types.SimpleNamespace(tok=torch.arange(rows.shape[0]), win_start=torch.cumsum(cnt, 0) - cnt, win_count=cnt, n_windows=len(wins))
        keep = {(i, h): torch.from_numpy(dropout_factors(C_P, C_SEED, w, h, ws.counts[w])) for i, w in enumerate(wins) for h in range(HEADS)}
        qk_r, v_r = qk[rows].clone().requires_grad_(), v[rows].clone().requires_grad_()
        tau_r = torch.full((1, 1, 1), C_TAU, dtype=torch.float64, requires_grad=True)
        ref_r = reference(qk_r, v_r, tau_r, TAU_MIN, HEADS, sub, keep)
        ref_r.backward(g[rows])
        ref[rows], dqk_w[rows], dv_w[rows], want_r[r] = ref_r.detach(), qk_r.grad, v_r.grad, tau_r.grad.reshape(())
    assert len(set(torch.cat([attn_ref.rows_of(ws, w) for w in range(len(ws.counts))]).tolist())) == m  # every row in one window
    qk_g, v_g = qk.float().to(dev).requires_grad_(), v.float().to(dev).requires_grad_()
    tau_g = torch.full((1, 1, 1), C_TAU, device=dev, requires_grad=True)
    out = ops.window_attention_packed(qk_g, v_g, tau_g, TAU_MIN, HEADS, wi, C_P, C_SEED)
    out.backward(g.float().to(dev))
    f = max(1.0, 0.1 / max(C_TAU, TAU_MIN))
    worst = {"fwd": _ratio((out.detach().double() - ref.to(dev)).abs().max(), 3e-5 * float(v.abs().max()))}
    for name, got, want in (("dv", v_g.grad, dv_w), ("dqk", qk_g.grad, dqk_w)):
        worst[name] = _ratio((got.double() - want.to(dev)).abs().max(), 3e-4 * f * max(1.0, float(want.abs().max())))
    worst["dtau"] = _ratio(abs(float(tau_g.grad.double()) - float(want_r.sum())), float((2e-3 * f * want_r.abs().clamp(min=1.0)).sum()))
    _record(f"C dh={dh} p={C_P} tau={C_TAU}", ws, sch, worst, t0)
    assert max(worst.values()) < 1.0, worst
