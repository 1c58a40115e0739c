"""Window-attention core (a19-a21) on ragged windows against an fp64 restatement of _scaled_cosine_attention
(cosine_msa.py:115-177) evaluated per window and head from the CSR: every head width of the model (dh 6 / 12 / 24 / 48),
window sizes around the 16 / 32 / 128-token tile edges, tau in the fixed-maximum regime, in the online-maximum regime
(tau < 0.036) and below tau_min (clamped), forward and backward; plus the dropout mask's statistics and determinism."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from attn_ref import HALF_TILE_SIZES, WINDOW_SIZES, reference, windows_of  # noqa: E402,F401  (shared with test_gpu_attention_scale.py)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def windows(dev):
    """Voxel coordinates whose shift-0 windows hold exactly WINDOW_SIZES tokens, rows shuffled."""
    ws = windows_of(dev, WINDOW_SIZES)
    return ws.wi, ws.m


@pytest.fixture(scope="module")
def half_tile_windows(dev):
    ws = windows_of(dev, HALF_TILE_SIZES)
    return ws.wi, ws.m


@pytest.mark.parametrize("tau", [1.0, 0.2, 0.02, 0.004])
@pytest.mark.parametrize("dh", [6, 12, 24, 48])
def test_attention_forward_and_backward_vs_fp64(dev, windows, dh, tau):
    from openseg3d_amd import ops
    wi, m = windows
    heads, c = 8, 8 * dh
    gen = torch.Generator().manual_seed(dh * 10 + int(tau * 1000))
    qk = torch.randn(m, 2 * c, generator=gen, dtype=torch.float64)
    qk[5] *= 1e-3   # short rows exercise the normalisation
    qk[7] *= 40.0
    v = torch.randn(m, c, generator=gen, dtype=torch.float64) * 1.5
    tau_t = torch.full((1, 1, 1), tau, dtype=torch.float64)
    g = torch.randn(m, c, generator=gen, dtype=torch.float64)

    qk_r, v_r, tau_r = qk.clone().requires_grad_(), v.clone().requires_grad_(), tau_t.clone().requires_grad_()
    ref = reference(qk_r, v_r, tau_r, 0.01, heads, wi)
    ref.backward(g)

    qk_g, v_g = qk.float().to(dev).requires_grad_(), v.float().to(dev).requires_grad_()
    tau_g = tau_t.float().to(dev).requires_grad_()
    out = ops.window_attention_packed(qk_g, v_g, tau_g, 0.01, heads, wi)
    # split-bf16 products (~2^-16 relative each); sharp softmax (tau 0.02: scores up to 72 in log2 units) amplifies the
    # score error by the score scale
    sharp = 1.0 / max(tau, 0.01)
    tol = 2e-5 * max(1.0, 0.1 * sharp) * float(v.abs().max())
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) < tol
    out.backward(g.float().to(dev))
    for got, want, name in ((v_g.grad, v_r.grad, "dv"), (qk_g.grad, qk_r.grad, "dqk"), (tau_g.grad, tau_r.grad, "dtau")):
        scale = max(1.0, float(want.abs().max()))
        # dtau is ONE number summed over every (query, key, head) triple with heavy cancellation: 2e-3 relative
        rel = 2e-3 if name == "dtau" else 3e-4
        assert float((got.cpu().double() - want).abs().max()) < rel * max(1.0, 0.1 * sharp) * scale, name
    if tau < 0.01:
        assert float(tau_g.grad.abs().max()) == 0.0  # clamped: no gradient (torch.clamp)


# ------------------------------------------------------------------------------------------ attention dropout
from dropout_ref import dropout_factors  # noqa: E402  (csrc/attn_dropout.hpp restated with numpy)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dh", [12, 24, 48])
def test_half_empty_last_tiles(dev, half_tile_windows, dh, p):
    """The fused backward skips the second 16-token half of a window's last streamed tile when it holds no token, and both
    directions switch tokens past the window's end off inside the score product (spare K channel) or by their LSE: windows
    whose last tile holds exactly 16 and 17 tokens, at the tile and at the 128-token chunk edge, with and without dropout."""
    from openseg3d_amd import ops
    wi, m = half_tile_windows
    heads, c, seed = 8, 8 * dh, 0x0123_4567_89AB_CDEF
    gen = torch.Generator().manual_seed(100 + dh)
    qk = torch.randn(m, 2 * c, generator=gen, dtype=torch.float64)
    v = torch.randn(m, c, generator=gen, dtype=torch.float64)
    g = torch.randn(m, c, generator=gen, dtype=torch.float64)
    tau_t = torch.full((1, 1, 1), 0.5, dtype=torch.float64)
    keep = None
    if p > 0:
        counts = wi.win_count[: wi.n_windows].cpu().tolist()
        keep = {(w, h): torch.from_numpy(dropout_factors(p, seed, w, h, n)) for w, n in enumerate(counts) for h in range(heads)}
    qk_r, v_r, tau_r = qk.clone().requires_grad_(), v.clone().requires_grad_(), tau_t.clone().requires_grad_()
    ref = reference(qk_r, v_r, tau_r, 0.01, heads, wi, keep)
    ref.backward(g)
    qk_g, v_g = qk.float().to(dev).requires_grad_(), v.float().to(dev).requires_grad_()
    tau_g = tau_t.float().to(dev).requires_grad_()
    out = ops.window_attention_packed(qk_g, v_g, tau_g, 0.01, heads, wi, p, seed)
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) < 3e-5 * float(v.abs().max())
    out.backward(g.float().to(dev))
    for got, want, name in ((v_g.grad, v_r.grad, "dv"), (qk_g.grad, qk_r.grad, "dqk"), (tau_g.grad, tau_r.grad, "dtau")):
        scale = max(1.0, float(want.abs().max()))
        assert float((got.cpu().double() - want).abs().max()) < (2e-3 if name == "dtau" else 3e-4) * scale, name


@pytest.mark.parametrize("dh", [6, 12, 24, 48])
def test_attention_dropout_forward_and_backward_vs_fp64(dev, windows, dh):
    """Training-mode attention (cosine_msa.py:172-174: dropout on the softmax output) with the kernels' counter-based mask
    restated on the host: forward and every gradient against fp64 autograd with the SAME mask -- which also proves that the
    forward and the two backward passes regenerate one and the same mask."""
    from openseg3d_amd import ops
    wi, m = windows
    heads, c, p, seed = 8, 8 * dh, 0.1, 0x1234_5678_9ABC_DEF
    gen = torch.Generator().manual_seed(dh)
    qk = torch.randn(m, 2 * c, generator=gen, dtype=torch.float64)
    v = torch.randn(m, c, generator=gen, dtype=torch.float64)
    g = torch.randn(m, c, generator=gen, dtype=torch.float64)
    tau_t = torch.full((1, 1, 1), 0.5, dtype=torch.float64)
    counts = wi.win_count[: wi.n_windows].cpu().tolist()
    keep = {(w, h): torch.from_numpy(dropout_factors(p, seed, w, h, n)) for w, n in enumerate(counts) for h in range(heads)}
    qk_r, v_r, tau_r = qk.clone().requires_grad_(), v.clone().requires_grad_(), tau_t.clone().requires_grad_()
    ref = reference(qk_r, v_r, tau_r, 0.01, heads, wi, keep)
    ref.backward(g)
    qk_g, v_g = qk.float().to(dev).requires_grad_(), v.float().to(dev).requires_grad_()
    tau_g = tau_t.float().to(dev).requires_grad_()
    out = ops.window_attention_packed(qk_g, v_g, tau_g, 0.01, heads, wi, p, seed)
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) < 3e-5 * float(v.abs().max())
    out.backward(g.float().to(dev))
    for got, want, name in ((v_g.grad, v_r.grad, "dv"), (qk_g.grad, qk_r.grad, "dqk"), (tau_g.grad, tau_r.grad, "dtau")):
        scale = max(1.0, float(want.abs().max()))
        assert float((got.cpu().double() - want).abs().max()) < (2e-3 if name == "dtau" else 3e-4) * scale, name


def test_attention_dropout_statistics(dev, windows):
    """Uniform attention (q = 0 -> every score 0 -> p = 1 / n) over v = 1: out = kept / (n * keep_prob).  The kept mass has
    mean 1; the drop rate is the 8-bit threshold's 26 / 256; a new seed gives a new mask, the same seed the same mask; eval
    (p = 0) is untouched."""
    from openseg3d_amd import ops
    wi, m = windows
    heads, c = 8, 192
    qk = torch.zeros(m, 2 * c, device=dev)
    v = torch.ones(m, c, device=dev)
    tau = torch.ones(1, 1, 1, device=dev)
    with torch.no_grad():
        base = ops.window_attention_packed(qk, v, tau, 0.01, heads, wi)
        a = ops.window_attention_packed(qk, v, tau, 0.01, heads, wi, 0.1, 11)
        a2 = ops.window_attention_packed(qk, v, tau, 0.01, heads, wi, 0.1, 11)
        b = ops.window_attention_packed(qk, v, tau, 0.01, heads, wi, 0.1, 12)
    assert float((base - 1.0).abs().max()) < 1e-5
    assert torch.equal(a, a2) and not torch.equal(a, b)
    # per (token, head) kept fraction, weighted by the window size n: pool over every (query, key, head) triple
    tok = wi.tok.cpu().long()
    counts = wi.win_count[: wi.n_windows].cpu().tolist()
    starts = wi.win_start[: wi.n_windows].cpu().tolist()
    n_of = torch.zeros(m)
    for s, n in zip(starts, counts):
        n_of[tok[s:s + n]] = float(n)
    keep_prob = 230.0 / 256.0
    kept = (a.cpu()[:, ::24] * keep_prob * n_of[:, None]).round()  # one channel per head: kept keys of that (query, head)
    total = float(n_of.sum()) * heads
    drop_rate = 1.0 - float(kept.sum()) / total
    sigma = (0.1 * 0.9 / total) ** 0.5
    assert abs(drop_rate - 26.0 / 256.0) < 5 * sigma, (drop_rate, sigma)
    # the mean of the kept mass is 1 (F.dropout's 1 / keep_prob scaling, with the threshold's own keep probability)
    mean = float((a.cpu()[:, ::24] * n_of[:, None]).sum()) / total
    assert abs(mean - 1.0) < 5 * sigma / keep_prob
    # bytes of one hash word are not correlated: the two keys of a 2 x 2 block drop independently
    big = max(range(len(counts)), key=lambda w: counts[w])
    f = dropout_factors(0.1, 11, big, 0, counts[big]) == 0.0
    both = float((f[:, 0::2][:, : f.shape[1] // 2] & f[:, 1::2][:, : f.shape[1] // 2]).mean())
    assert abs(both - (26.0 / 256.0) ** 2) < 0.004


def test_unsupported_head_geometry_is_refused_with_a_clear_error(dev, windows):
    """The kernels take the reference's head geometries (8 heads of 6 / 12 / 24 / 48 channels, pointtransformer.py:143-155)
    and their obvious relatives; anything else is refused up front -- by name, not by a bare SEG3D_EINVAL from the launch
    -- and seg3d_window_attn_supported tells a caller beforehand."""
    from openseg3d_amd import _lib, ops
    lib = _lib.load()
    for heads, dh, ok in ((8, 6, 1), (8, 12, 1), (8, 24, 1), (8, 48, 1), (4, 12, 1), (16, 24, 1), (3, 12, 0), (6, 6, 0),
                          (8, 32, 0), (12, 6, 0), (17, 24, 0), (16, 6, 1), (20, 6, 0), (20, 12, 0), (0, 24, 0)):
        assert lib.seg3d_window_attn_supported(heads, dh) == ok, (heads, dh)
    wi, m = windows
    qk, v = torch.randn(m, 72, device=dev), torch.randn(m, 36, device=dev)
    with pytest.raises(_lib.Seg3dError, match="head geometry"):
        ops.window_attention_packed(qk, v, torch.ones(1, 1, 1, device=dev), 0.01, 3, wi)


def _fp64_case(windows, heads, dh, tau, p, seed):
    """Inputs and the fp64 forward / autograd of one head geometry on a window fixture."""
    wi, m = windows
    c = heads * dh
    gen = torch.Generator().manual_seed(1000 * heads + dh + (7 if p else 0))
    qk = torch.randn(m, 2 * c, generator=gen, dtype=torch.float64)
    v = torch.randn(m, c, generator=gen, dtype=torch.float64) * 1.5
    g = torch.randn(m, c, generator=gen, dtype=torch.float64)
    tau_t = torch.full((1, 1, 1), tau, dtype=torch.float64)
    keep = None
    if p > 0:
        counts = wi.win_count[: wi.n_windows].cpu().tolist()
        keep = {(w, h): torch.from_numpy(dropout_factors(p, seed, w, h, n)) for w, n in enumerate(counts) for h in range(heads)}
    qk_r, v_r, tau_r = qk.clone().requires_grad_(), v.clone().requires_grad_(), tau_t.clone().requires_grad_()
    ref = reference(qk_r, v_r, tau_r, 0.01, heads, wi, keep)
    ref.backward(g)
    return qk, v, g, tau_t, ref.detach(), qk_r.grad, v_r.grad, tau_r.grad


def _assert_vs_fp64(out, grads, ref, wants, v, tau, p):
    """The bars of the 8-head cases above: forward 2e-5 f max|v| (3e-5 max|v| with dropout at tau 0.5), dv / dqk 3e-4 f
    max(1, max|want|), dtau 2e-3 f max(1, |want|), f = max(1, 0.1 / max(tau, 0.01))."""
    f = max(1.0, 0.1 / max(tau, 0.01))
    tol = (3e-5 if p else 2e-5 * f) * float(v.abs().max())
    assert float((out.detach().cpu().double() - ref).abs().max()) < tol
    for got, want, name in zip(grads, wants, ("dqk", "dv", "dtau")):
        scale = max(1.0, float(want.abs().max()))
        assert float((got.cpu().double() - want).abs().max()) < (2e-3 if name == "dtau" else 3e-4) * f * scale, name


# every relative of the reference's geometry seg3d_window_attn_supported accepts: 4 / 12 / 16 narrow heads (dh 6: 4 / 16; 1, 3 and 4 groups of
# four), 1 .. 16 wide heads (the backward's 8-item groups x heads, odd head counts)
@pytest.mark.parametrize("heads,dh,tau,p", [(4, 6, 0.2, 0.0), (16, 6, 0.2, 0.0), (4, 12, 0.2, 0.0),
                                            (12, 12, 0.2, 0.0), (1, 24, 0.2, 0.0), (5, 24, 0.2, 0.0), (16, 24, 0.2, 0.0),
                                            (1, 48, 0.2, 0.0), (3, 48, 0.2, 0.0), (16, 48, 0.2, 0.0),
                                            (4, 12, 0.5, 0.1), (16, 24, 0.5, 0.1), (16, 6, 0.5, 0.1)])
def test_head_geometries_vs_fp64(dev, windows, heads, dh, tau, p):
    from openseg3d_amd import _lib, ops
    wi, m = windows
    assert _lib.load().seg3d_window_attn_supported(heads, dh) == 1
    seed = 0x0F1E_2D3C_4B5A_6978
    qk, v, g, tau_t, ref, dqk_w, dv_w, dtau_w = _fp64_case(windows, heads, dh, tau, p, seed)
    qk_g, v_g = qk.float().to(dev).requires_grad_(), v.float().to(dev).requires_grad_()
    tau_g = tau_t.float().to(dev).requires_grad_()
    out = ops.window_attention_packed(qk_g, v_g, tau_g, 0.01, heads, wi, p, seed)
    out.backward(g.float().to(dev))
    _assert_vs_fp64(out, (qk_g.grad, v_g.grad, tau_g.grad), ref, (dqk_w, dv_w, dtau_w), v, tau, p)


@pytest.mark.parametrize("dh", [12, 48])
def test_row_strided_entry_vs_fp64_and_packed(dev, windows, dh):
    """ops.window_attention: q, k, v as the three column blocks of ONE [m, 3C] tensor (row stride 3C, what a fused in-projection
    would hand over): forward and dq / dk / dv / dtau against fp64, and bit for bit what the packed entry returns for the same
    values (same kernels, other strides)."""
    from openseg3d_amd import ops
    wi, m = windows
    heads, c, tau = 8, 8 * dh, 0.2
    qk, v, g, tau_t, ref, dqk_w, dv_w, dtau_w = _fp64_case(windows, heads, dh, tau, 0.0, 0)
    qkv = torch.cat([qk, v], dim=1).float().to(dev).requires_grad_()
    assert qkv.stride(0) == 3 * c
    tau_g = tau_t.float().to(dev).requires_grad_()
    out = ops.window_attention(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], tau_g, 0.01, heads, wi)
    out.backward(g.float().to(dev))
    dqkv = qkv.grad
    _assert_vs_fp64(out, (dqkv[:, :2 * c], dqkv[:, 2 * c:], tau_g.grad), ref, (dqk_w, dv_w, dtau_w), v, tau, 0.0)
    qk_p, v_p = qk.float().to(dev).requires_grad_(), v.float().to(dev).requires_grad_()
    tau_p = tau_t.float().to(dev).requires_grad_()
    out_p = ops.window_attention_packed(qk_p, v_p, tau_p, 0.01, heads, wi)
    out_p.backward(g.float().to(dev))
    assert torch.equal(out, out_p)
    assert torch.equal(dqkv[:, :2 * c], qk_p.grad) and torch.equal(dqkv[:, 2 * c:], v_p.grad) and torch.equal(tau_g.grad, tau_p.grad)


def test_row_strided_entry_refusals(dev, windows):
    """The documented refusals of ops.window_attention: anything but float32, and a last dimension that is not contiguous."""
    from openseg3d_amd import _lib, ops
    wi, m = windows
    c = 96
    tau = torch.ones(1, 1, 1, device=dev)
    q, k, v = (torch.randn(m, c, device=dev) for _ in range(3))
    for bad in (torch.float64, torch.float16, torch.bfloat16):
        for i in range(3):
            args = [q, k, v]
            args[i] = args[i].to(bad)
            with pytest.raises(_lib.Seg3dError, match="float32 with a contiguous last dimension"):
                ops.window_attention(*args, tau, 0.01, 8, wi)
    wide = torch.randn(m, 2 * c, device=dev)
    t = torch.randn(c, m, device=dev).t()  # [m, c] with stride (1, m)
    for i, view in ((0, wide[:, ::2]), (1, t), (2, wide[:, 1::2])):
        assert view.shape == (m, c) and view.stride(1) != 1
        args = [q, k, v]
        args[i] = view
        with pytest.raises(_lib.Seg3dError, match="float32 with a contiguous last dimension"):
            ops.window_attention(*args, tau, 0.01, 8, wi)


def test_attention_time_does_not_depend_on_tau(dev):
    """The forward has two softmax forms: the fixed-maximum one (every cosine score is bounded by log2e / tau) and, below
    tau ~ 0.036 where that bound could underflow, the online-maximum one -- a wave-uniform branch on the device scalar.
    A learnt temperature must not move a layer onto a slow path: on the headline scene's stage 1 (narrow heads) and
    stage 3 (wide heads) the layer at tau = 0.02 takes at most 2x its time at tau = 1 (measured 1.1-1.2x; the round-2
    record that read 11 ms for these layers was the instrumented pass allocating gigabytes of unused workspace)."""
    from openseg3d_amd import batch as B, config, ops, scene, spconv, swformer
    cfg = config.default_cfg()
    ds = config.DatasetSpec(cfg)
    b = B.make_batch([scene.make_scene(0)], ds.voxel_size, ds.point_cloud_range)
    level = spconv.SiteLevel(b["voxel_coords"].int(), [int(g) for g in ds.grid_size][::-1], 1)
    info = [{int(k): v for k, v in lvl.items()} for lvl in cfg.MODEL.BATCHING_INFO]
    for stage, c in enumerate((48, 96, 192)):
        if stage != 1:
            part = swformer.SparseWindowPartitionLayer(info[stage], cfg.MODEL.WINDOW_SHAPE, [float(g) / 2 ** stage for g in ds.grid_size])
            wi = part.plan(level.coords, 1, c).index[0]
            m = level.coords.shape[0]
            qk, v = torch.randn(m, 2 * c, device=dev), torch.randn(m, c, device=dev)
            times = {}
            for tau_v in (1.0, 0.02):
                tau = torch.full((1, 1, 1), tau_v, device=dev)
                for _ in range(3):
                    ops.window_attention_packed(qk, v, tau, 0.01, 8, wi)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                # The window is ten launches, under a millisecond.  The scene and the plan built above leave Python's collector
                # about due for a full pass (50 ms with torch's objects in the heap), and when that pass fell between two of
                # these launches the device sat idle inside the window: collect now, so that none falls due in it.
                gc.collect()
                torch.cuda.synchronize()
                e0.record()
                for _ in range(10):
                    ops.window_attention_packed(qk, v, tau, 0.01, 8, wi)
                e1.record()
                torch.cuda.synchronize()
                times[tau_v] = e0.elapsed_time(e1) / 10
            assert times[0.02] <= 2.0 * times[1.0], (stage, times)
        level = level.down()[0]
