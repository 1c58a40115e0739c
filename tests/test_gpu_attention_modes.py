"""The per-head-tau and scaled-dot-product modes of the window-attention core (seg3d_window_attn_fwd_modes / _bwd_modes;
cosine_msa.py:156-160 with tau [1, H, 1, 1], :163-165) against the fp64 restatements of attn_modes_ref.py: every head width,
window sizes around the 16 / 32 / 128-token edges, every tau regime on every head position, dot-product scores that need the
running maximum, dropout with the kernels' own mask, determinism, the module and the training layer.

Bars are the project's own (test_gpu_attention.py), applied per head with f_h = max(1, 0.1 / max(tau_h, 0.01)); in dot mode
1 / tau's counterpart is S_abs = max |q_i| |k_j| / sqrt(dh) over same-window pairs, f = max(1, 0.1 S_abs)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_modes_ref as amr  # noqa: E402
from attn_ref import HALF_TILE_SIZES, rows_of, windows_of  # noqa: E402
from dropout_ref import dropout_factors  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN_SIZES = [1, 2, 16, 17, 33, 64, 129, 257, 640]
FIXTURE_TAUS = [1.0, 0.5, 0.2, 0.1, 0.05, 0.02, 0.011, 0.004]  # tests/golden/attn_modes.npz; the last is below tau_min
HEADS, TAU_MIN, SEED = 8, 0.01, 0x0BAD_5EED_1234_5678
DHS = [6, 12, 24, 48]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def main_ws(dev):
    return windows_of(dev, MAIN_SIZES)


@pytest.fixture(scope="module")
def half_ws(dev):
    return windows_of(dev, HALF_TILE_SIZES)


@pytest.fixture(scope="module")
def refs():
    return {}  # fp64 forward / autograd of a case, computed once and shared by the tests that need it


def keep_of(wi, p, seed):
    counts = wi.win_count[: wi.n_windows].cpu().tolist()
    return {(w, h): torch.from_numpy(dropout_factors(p, seed, w, h, n)) for w, n in enumerate(counts) for h in range(HEADS)}


def fp64_case(refs, key, wi, qk, v, g, tau, p=0.0):
    """-> (out, dqk, dv, dtau or None) in fp64"""
    if key not in refs:
        qk_r, v_r = qk.clone().requires_grad_(), v.clone().requires_grad_()
        tau_r = None if tau is None else tau.clone().requires_grad_()
        out = amr.reference(qk_r, v_r, tau_r, TAU_MIN, HEADS, wi, keep_of(wi, p, SEED) if p else None)
        out.backward(g)
        refs[key] = (out.detach(), qk_r.grad, v_r.grad, None if tau is None else tau_r.grad)
    return refs[key]


def run_gpu(dev, wi, qk, v, g, tau, p=0.0):
    from openseg3d_amd import ops
    qk_g, v_g = qk.float().to(dev).requires_grad_(), v.float().to(dev).requires_grad_()
    tau_g = None if tau is None else tau.float().to(dev).requires_grad_()
    out = ops.window_attention_packed(qk_g, v_g, tau_g, TAU_MIN, HEADS, wi, p, SEED if p else 0)
    out.backward(g.float().to(dev))
    torch.cuda.synchronize()
    return out.detach(), qk_g.grad, v_g.grad, None if tau is None else tau_g.grad


def cosine_inputs(m, c, seed):
    """test_gpu_attention.py's inputs: randn, one row x 1e-3, one row x 40, v x 1.5"""
    gen = torch.Generator().manual_seed(seed)
    qk = torch.randn(m, 2 * c, generator=gen, dtype=torch.float64)
    qk[5] *= 1e-3
    qk[7] *= 40.0
    v = torch.randn(m, c, generator=gen, dtype=torch.float64) * 1.5
    g = torch.randn(m, c, generator=gen, dtype=torch.float64)
    return qk, v, g


def plain_inputs(m, c, seed):
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(m, w, generator=gen, dtype=torch.float64) for w in (2 * c, c, c))


def err(got, want):
    return float((got.detach().cpu().double() - want).abs().max())


def check_per_head(label, got, want, v, f_heads, dh, fwd_rel=2e-5, grad_rel=3e-4, tau_rel=2e-3):
    """The bars head by head: forward fwd_rel f_h max|v| on the head's columns, dqk / dv grad_rel f_h max(1, max|want|) on
    them, dtau[h] tau_rel f_h max(1, |want_h|).  Prints every figure, then asserts all of them."""
    out, dqk, dv, dtau = got
    out_w, dqk_w, dv_w, dtau_w = want
    c = HEADS * dh
    bad = []
    for h in range(HEADS):
        f = f_heads[h]
        cols = torch.arange(h * dh, (h + 1) * dh)
        qk_cols = torch.cat([cols, c + cols])
        rows = [("out", err(out[:, cols], out_w[:, cols]), fwd_rel * f * float(v[:, cols].abs().max())),
                ("dqk", err(dqk[:, qk_cols], dqk_w[:, qk_cols]), grad_rel * f * max(1.0, float(dqk_w[:, qk_cols].abs().max()))),
                ("dv", err(dv[:, cols], dv_w[:, cols]), grad_rel * f * max(1.0, float(dv_w[:, cols].abs().max())))]
        if dtau_w is not None:
            t_w = dtau_w.reshape(-1)[h]
            rows.append(("dtau", err(dtau.reshape(-1)[h], t_w), tau_rel * f * max(1.0, abs(float(t_w)))))
        for name, e, bar in rows:
            print(f"FIGURE {label} head {h} f={f:.2f} {name} err={e:.3e} bar={bar:.3e}")
            if not e < bar:
                bad.append((h, name, e, bar))
    assert not bad, (label, bad)


def f_of_tau(taus):
    return [max(1.0, 0.1 / max(float(t), 0.01)) for t in taus]


# ------------------------------------------------------------------------------------------ per-head tau
def per_head_taus(dh):
    """the fixture's eight regimes, rotated per head width: every head position (wave, head group) meets every regime"""
    r = DHS.index(dh) * 3 % HEADS
    return FIXTURE_TAUS[r:] + FIXTURE_TAUS[:r]


@pytest.mark.parametrize("dh", DHS)
def test_per_head_tau_forward_and_backward_vs_fp64(dev, main_ws, refs, dh):
    """Every tau regime on every head position, bars head by head.  (Closest figures on an MI355X: dtau of the tau = 0.1
    head at dh 24, 9.1e-3 against 1.09e-2 -- one head's sum over 1.3 M pairs that cancels to 5.4; forward of the tau = 0.011
    head at dh 12 / 24 / 48 at 66 / 46 / 25 % of its bar.  At dh 6 the forward is the exact-fp32 kernel: 2.4e-5 against 1.04e-3.)"""
    ws, c = main_ws, HEADS * dh
    taus = per_head_taus(dh)
    tau = torch.tensor(taus, dtype=torch.float64).reshape(1, HEADS, 1, 1)
    qk, v, g = cosine_inputs(ws.m, c, 500 + dh)
    want = fp64_case(refs, ("perhead", dh), ws.wi, qk, v, g, tau)
    got = run_gpu(dev, ws.wi, qk, v, g, tau)
    assert got[3].shape == (1, HEADS, 1, 1)
    check_per_head(f"perhead-{dh}", got, want, v, f_of_tau(taus), dh)
    clamped = taus.index(0.004)
    assert float(got[3].reshape(-1)[clamped]) == 0.0 and float(want[3].reshape(-1)[clamped]) == 0.0  # tau_h <= tau_min
    assert all(float(t) != 0.0 for i, t in enumerate(got[3].reshape(-1)) if i != clamped)


@pytest.mark.parametrize("dh", DHS)
def test_per_head_tau_with_dropout_vs_fp64(dev, main_ws, refs, dh):
    """p = 0.1 with the kernels' own mask restated on the host, tau_h alternating 0.5 / 0.3: the dropout tests' bars (3e-5 max|v|
    forward, 3e-4 dqk / dv, 2e-3 dtau on the quantity's scale)."""
    ws, c, p = main_ws, HEADS * dh, 0.1
    taus = [0.5, 0.3] * (HEADS // 2)
    tau = torch.tensor(taus, dtype=torch.float64).reshape(1, HEADS, 1, 1)
    qk, v, g = plain_inputs(ws.m, c, 600 + dh)
    want = fp64_case(refs, ("perhead-drop", dh), ws.wi, qk, v, g, tau, p)
    got = run_gpu(dev, ws.wi, qk, v, g, tau, p)
    figs = [("out", err(got[0], want[0]), 3e-5 * float(v.abs().max()))]
    figs += [(n, err(a, b), r * max(1.0, float(b.abs().max())))
             for n, a, b, r in (("dqk", got[1], want[1], 3e-4), ("dv", got[2], want[2], 3e-4), ("dtau", got[3], want[3], 2e-3))]
    for n, e, bar in figs:
        print(f"FIGURE perhead-drop-{dh} {n} err={e:.3e} bar={bar:.3e}")
    assert all(e < bar for _, e, bar in figs), figs


@pytest.mark.parametrize("tau_v", [0.2, 0.02])
@pytest.mark.parametrize("dh", DHS)
def test_equal_per_head_taus_match_the_shared_entry(dev, main_ws, dh, tau_v):
    """All heads on one tau against the shared-tau entry.  NOT compared with torch.equal: the per-head kernels are other
    instantiations of the kernel bodies, and not always of the same body -- at dh 6 per-head tau takes the exact-fp32
    vector-ALU forward where the shared tau takes the fused one (measured difference 4.8e-5 at tau 0.2; at dh 12 / 24 / 48
    out, dqk and dv come out bit-equal, which is not promised), and the per-head tau gradient uses another row constant.
    So out, dqk and dv are held to the bars above on their difference, and sum_h dtau[h] to the dtau bar against the
    shared dtau."""
    ws, c = main_ws, HEADS * dh
    qk, v, g = cosine_inputs(ws.m, c, 700 + dh)
    f = max(1.0, 0.1 / tau_v)
    shared = run_gpu(dev, ws.wi, qk, v, g, torch.full((1, 1, 1), tau_v, dtype=torch.float64))
    heads = run_gpu(dev, ws.wi, qk, v, g, torch.full((1, HEADS, 1, 1), tau_v, dtype=torch.float64))
    s64 = [t.cpu().double() for t in shared]
    figs = [("out", err(heads[0], s64[0]), 2e-5 * f * float(v.abs().max())),
            ("dqk", err(heads[1], s64[1]), 3e-4 * f * max(1.0, float(s64[1].abs().max()))),
            ("dv", err(heads[2], s64[2]), 3e-4 * f * max(1.0, float(s64[2].abs().max()))),
            ("dtau", abs(float(heads[3].double().sum()) - float(s64[3].sum())), 2e-3 * f * max(1.0, abs(float(s64[3].sum()))))]
    for n, e, bar in figs:
        print(f"FIGURE equal-taus-{dh}-{tau_v} {n} diff={e:.3e} bar={bar:.3e}")
    assert all(e < bar for _, e, bar in figs), figs


def test_one_element_tau_still_takes_the_shared_entry(dev, main_ws, monkeypatch):
    from openseg3d_amd import _lib
    names, call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    qk, v, g = plain_inputs(main_ws.m, 96, 1)
    run_gpu(dev, main_ws.wi, qk, v, g, torch.ones(1, 1, 1, dtype=torch.float64))
    assert [n for n in names if "attn" in n] == ["seg3d_window_attn_fwd", "seg3d_window_attn_bwd"]
    del names[:]
    run_gpu(dev, main_ws.wi, qk, v, g, torch.ones(1, HEADS, 1, 1, dtype=torch.float64))
    run_gpu(dev, main_ws.wi, qk, v, g, None)
    assert [n for n in names if "attn" in n] == ["seg3d_window_attn_fwd_modes", "seg3d_window_attn_bwd_modes"] * 2


# ------------------------------------------------------------------------------------------ dot product
def check_dot(label, got, want, v, f, fwd_rel=2e-5, grad_rel=3e-4):
    figs = [("out", err(got[0], want[0]), fwd_rel * f * float(v.abs().max())),
            ("dqk", err(got[1], want[1]), grad_rel * f * max(1.0, float(want[1].abs().max()))),
            ("dv", err(got[2], want[2]), grad_rel * f * max(1.0, float(want[2].abs().max())))]
    for n, e, bar in figs:
        print(f"FIGURE {label} f={f:.2f} {n} err={e:.3e} bar={bar:.3e}")
    assert all(e < bar for _, e, bar in figs), (label, figs)


@pytest.mark.parametrize("dh", DHS)
def test_dot_mode_moderate_scores_vs_fp64(dev, main_ws, refs, dh):
    ws, c = main_ws, HEADS * dh
    qk, v, g = plain_inputs(ws.m, c, 800 + dh)
    s_abs = amr.score_extent(qk, HEADS, ws.wi)
    f = max(1.0, 0.1 * s_abs)
    assert s_abs < 25.0  # randn rows: |q| |k| / sqrt(dh) ~ sqrt(dh)
    want = fp64_case(refs, ("dot", dh), ws.wi, qk, v, g, None)
    got = run_gpu(dev, ws.wi, qk, v, g, None)
    assert got[3] is None
    check_dot(f"dot-{dh}", got, want, v, f)


def sharp_dot_inputs(ws, dh, seed):
    """Keys with a common component u (the first channel of every head) and, in every window of >= 64 tokens, two query rows
    +beta u and -beta u, beta such that S_abs = 50: the score scale of cosine tau = 0.02."""
    c = HEADS * dh
    qk, v, g = plain_inputs(ws.m, c, seed)
    k = qk[:, c:]
    k *= 0.15
    k[:, ::dh] += 4.0
    k_len = k.reshape(ws.m, HEADS, dh).norm(dim=-1).max()
    beta = 50.0 * dh ** 0.5 / float(k_len)
    marked = []
    for w, n in enumerate(ws.counts):
        if n >= 64:
            rows = rows_of(ws, w)
            for r, sign in ((int(rows[0]), 1.0), (int(rows[1]), -1.0)):
                qk[r, :c] = 0.0
                qk[r, :c:dh] = sign * beta
                marked.append((w, r, sign))
    return qk, v, g, marked


@pytest.mark.parametrize("dh", DHS)
def test_dot_mode_scores_that_need_the_running_maximum(dev, main_ws, refs, dh):
    """Scores of +-40 .. 60 (natural units): a kernel that took a fixed bound for the maximum, or 0, gets the -beta u rows
    (every score <= -30) and the +beta u rows (scores >= +30) wrong by O(1).  Bars: the formula of the moderate case with
    f = max(1, 0.1 S_abs) ~ 5, the bars cosine tau = 0.02 is held to."""
    ws, c = main_ws, HEADS * dh
    qk, v, g, marked = sharp_dot_inputs(ws, dh, 900 + dh)
    s_abs = amr.score_extent(qk, HEADS, ws.wi)
    assert 40.0 <= s_abs <= 60.0, s_abs
    low = high = False
    for w, r, sign in marked:
        rows = rows_of(ws, w)
        i = int((rows == r).nonzero()[0])
        for h in range(HEADS):
            s = amr.scores(qk, None, TAU_MIN, HEADS, rows, h)[i]
            low |= bool((s <= -30.0).all())
            high |= bool((s >= 30.0).any())
    assert low and high
    want = fp64_case(refs, ("dot-sharp", dh), ws.wi, qk, v, g, None)
    got = run_gpu(dev, ws.wi, qk, v, g, None)
    # the float32 CPU evaluation of the same restatement on the same inputs, for the record beside the kernel's figures
    o32 = amr.reference(qk.float(), v.float(), None, TAU_MIN, HEADS, ws.wi)
    print(f"FIGURE dot-sharp-{dh} S_abs={s_abs:.2f} float32-restatement out err={float((o32.double() - want[0]).abs().max()):.3e}")
    check_dot(f"dot-sharp-{dh}", got, want, v, max(1.0, 0.1 * s_abs))


@pytest.mark.parametrize("which", ["half", "main"])
@pytest.mark.parametrize("dh", DHS)
def test_dot_mode_with_dropout_vs_fp64(dev, main_ws, half_ws, refs, dh, which):
    """p = 0.1 against fp64 with the same mask, on windows whose last tile is half empty and on the main set."""
    ws, c, p = (half_ws if which == "half" else main_ws), HEADS * dh, 0.1
    qk, v, g = plain_inputs(ws.m, c, 1000 + dh)
    f = max(1.0, 0.1 * amr.score_extent(qk, HEADS, ws.wi))
    want = fp64_case(refs, ("dot-drop", which, dh), ws.wi, qk, v, g, None, p)
    got = run_gpu(dev, ws.wi, qk, v, g, None, p)
    check_dot(f"dot-drop-{which}-{dh}", got, want, v, f, fwd_rel=3e-5)


# ------------------------------------------------------------------------------------------ determinism, refusals
@pytest.mark.parametrize("mode", ["perhead", "dot"])
@pytest.mark.parametrize("dh", DHS)
def test_backward_is_deterministic(dev, main_ws, dh, mode):
    ws, c = main_ws, HEADS * dh
    qk, v, g = cosine_inputs(ws.m, c, 1100 + dh)
    tau = None if mode == "dot" else torch.tensor(per_head_taus(dh), dtype=torch.float64).reshape(1, HEADS, 1, 1)
    a, b = run_gpu(dev, ws.wi, qk, v, g, tau, 0.1), run_gpu(dev, ws.wi, qk, v, g, tau, 0.1)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)


def test_other_tau_forms_are_refused_by_name(dev, main_ws):
    from openseg3d_amd import _lib, ops
    ws = main_ws
    qk, v = torch.randn(ws.m, 192, device=dev), torch.randn(ws.m, 96, device=dev)
    with pytest.raises(_lib.Seg3dError, match=r"1 element.*\[1, H, 1, 1\].*None"):
        ops.window_attention_packed(qk, v, torch.ones(3, device=dev), TAU_MIN, HEADS, ws.wi)
    with pytest.raises(_lib.Seg3dError, match=r"together with dot-product mode.*1 element.*\[1, H, 1, 1\].*None"):
        ops.window_attention_packed(qk, v, torch.ones(1, HEADS, 1, 1, device=dev), TAU_MIN, HEADS, ws.wi, cosine=False)
    with pytest.raises(_lib.Seg3dError, match=r"\[1, H, 1, 1\]"):
        ops.window_attention(qk[:, :96], qk[:, 96:], v, torch.ones(3, device=dev), TAU_MIN, HEADS, ws.wi)


# ------------------------------------------------------------------------------------------ module level
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "attn_modes.npz"))


@pytest.mark.parametrize("case", ["perhead", "dot"])
def test_module_matches_the_reference_fixture(dev, golden, case):
    """swformer.CosineMultiheadAttention in eval mode on a plan whose windows hold the fixture's 1, 5, 17 and 33 tokens.
    Bar per quantity: 4 x the fixture's own float32-against-float64 deviation, floored by the kernel bars (2e-5 forward, 3e-4
    gradients, 2e-3 dtau, times f and the quantity's scale; f = 10 for the per-head case, whose sharpest heads sit at
    tau_min, max(1, 0.1 S_abs) for the dot case)."""
    from openseg3d_amd import swformer
    d = golden
    e, heads, _ = (int(x) for x in d["meta"])
    sizes = [int(s) for s in d["sizes"]]
    ws = windows_of(dev, sizes)
    # fixture token t of window i -> flat row of the t-th token of the plan's window built for size i
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    row_of = torch.empty(sum(sizes), dtype=torch.long)
    for w in range(len(sizes)):
        i = int(ws.which[w])
        row_of[first[i]:first[i] + sizes[i]] = rows_of(ws, w)
    place = lambda a: torch.zeros(ws.m, e).index_copy(0, row_of, torch.from_numpy(a).float())  # noqa: E731
    mod = swformer.CosineMultiheadAttention(e, heads, dropout=0.1, tau_min=float(d["tau_min"]), cosine=case != "dot",
                                            non_shared_tau=case == "perhead")
    sd = {k: torch.from_numpy(d["param_" + k.replace(".", "_")]) for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")}
    if case == "perhead":
        sd["tau"] = torch.from_numpy(d["tau"]).float().reshape(1, heads, 1, 1)
    mod.load_state_dict(sd, strict=True)
    mod = mod.to(dev).eval()
    x = place(d["x"]).to(dev).requires_grad_()
    y = mod(x, place(d["pos"]).to(dev), ws.wi)
    y.backward(place(d["g"]).to(dev))
    got = {"out": y.detach().cpu()[row_of], "g_x": x.grad.cpu()[row_of], "g_in_w": mod.in_proj_weight.grad,
           "g_in_b": mod.in_proj_bias.grad, "g_out_w": mod.out_proj.weight.grad}
    if case == "perhead":
        got["g_tau"] = mod.tau.grad
        f = 10.0
        assert float(mod.tau.grad.reshape(-1)[-1]) == 0.0
    else:
        c = e
        xw, pw = torch.from_numpy(d["x"]).double(), torch.from_numpy(d["pos"]).double()
        w_in, b_in = sd["in_proj_weight"].double(), sd["in_proj_bias"].double()
        qk = (xw + pw) @ w_in[: 2 * c].t() + b_in[: 2 * c]
        f = max(1.0, 0.1 * amr.score_extent(qk, heads, amr.host_csr(sizes)))
    bad = []
    for k, have in got.items():
        want = torch.from_numpy(d[f"{case}_{k}"])
        floor = (2e-5 if k == "out" else 2e-3 if k == "g_tau" else 3e-4) * f * max(1.0, float(want.abs().max()))
        bar = max(4.0 * float(d[f"{case}_f32_err_{k}"]), floor)
        e_k = err(have, want)
        print(f"FIGURE module-{case} {k} err={e_k:.3e} bar={bar:.3e} f32dev={float(d[f'{case}_f32_err_{k}']):.3e}")
        if not e_k < bar:
            bad.append((k, e_k, bar))
    assert not bad, bad


# ------------------------------------------------------------------------------------------ layer level
@pytest.mark.parametrize("cosine,non_shared", [(True, True), (False, False)])
def test_training_layer_single_node_matches_the_composed_modules(dev, main_ws, monkeypatch, cosine, non_shared):
    """EncoderLayer(96, 8, 192) in training mode with either option: the single autograd node (ops._EncoderLayerFn) against
    the layer composed from its modules -- same parameters, same attention-dropout seed, same DropPath factors.  Both sides
    run the same kernels; the bars are the gradients' (3e-4 on the quantity's scale, 2e-3 for tau, 2e-5 for the output)."""
    from openseg3d_amd import swformer
    ws, c = main_ws, 96
    torch.manual_seed(5)
    layer = swformer.EncoderLayer(c, HEADS, 192, attn_drop=0.1, drop_path_rate=0.2, cosine=cosine, non_shared_tau=non_shared).to(dev).train()
    at = layer.win_attn.self_attn
    if cosine:
        with torch.no_grad():
            at.tau.copy_(torch.tensor([1.0, 0.5, 0.2, 0.1] * 2, device=dev).reshape(1, HEADS, 1, 1))
    else:
        assert at.tau is None
    gen = torch.Generator().manual_seed(77)
    x, pos, g = (torch.randn(ws.m, c, generator=gen).to(dev) for _ in range(3))
    s1, s2 = ((torch.rand(ws.m, generator=gen) < 0.8).float().div(0.8).to(dev) for _ in range(2))
    runs = {}
    for fused in (True, False):
        monkeypatch.setattr(swformer, "FUSED_LAYER", fused)
        layer.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_()
        y = layer(xg, pos, ws.wi, scales=(s1, s2), seed=1234)
        assert ("EncoderLayerFn" in type(y.grad_fn).__name__) == fused  # exactly one node for the whole layer
        y.backward(g)
        runs[fused] = (y.detach(), xg.grad, {k: v.grad.clone() for k, v in layer.named_parameters()})
    (y_f, dx_f, gr_f), (y_c, dx_c, gr_c) = runs[True], runs[False]
    assert set(gr_f) == set(gr_c) and ("win_attn.self_attn.tau" in gr_f) == cosine
    figs = [("y", y_f, y_c, 2e-5), ("dx", dx_f, dx_c, 3e-4)] + [(k, gr_f[k], gr_c[k], 2e-3 if k.endswith(".tau") else 3e-4) for k in gr_c]
    bad = []
    for name, a, b, rel in figs:
        e_k, bar = err(a, b.cpu().double()), rel * max(1.0, float(b.abs().max()))
        print(f"FIGURE layer-{'cos' if cosine else 'dot'} {name} diff={e_k:.3e} bar={bar:.3e}")
        if not e_k < bar:
            bad.append((name, e_k, bar))
    assert not bad, bad
    if cosine:
        assert gr_f["win_attn.self_attn.tau"].shape == (1, HEADS, 1, 1)
