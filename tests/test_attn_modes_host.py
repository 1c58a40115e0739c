"""CPU-side checks of the per-head-tau and dot-product attention modes: the fp64 restatement the GPU tests measure the
kernels with (attn_modes_ref.py) against the reference module's own numbers (tests/golden/attn_modes.npz), the modules'
constructor options / state dicts / checkpoint loading, and every refusal of the seg3d_window_attn_*_modes entries."""
import ctypes
import os

import numpy as np
import pytest
import torch

import attn_modes_ref as amr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "attn_modes.npz"))


def fixture_case(d, case, dtype=torch.float64):
    """(x, pos, g, params, tau) of a fixture case as leaf tensors of `dtype`"""
    x, pos, g = (torch.from_numpy(d[k]).to(dtype) for k in ("x", "pos", "g"))
    par = {k: torch.from_numpy(d["param_" + k]).to(dtype) for k in ("in_proj_weight", "in_proj_bias", "out_proj_weight", "out_proj_bias")}
    tau = torch.from_numpy(d["tau"]).to(dtype).reshape(1, -1, 1, 1) if case == "perhead" else None
    return x, pos, g, par, tau


@pytest.mark.parametrize("case", ["perhead", "dot"])
def test_fp64_restatement_reproduces_the_reference_module(golden, case):
    """The fixture's padded [T, W, E] run of the reference module against the restatement on a RAGGED layout: the 56 valid
    tokens scattered over the flat rows by a fixed permutation, windows found through the CSR.  Outputs and every gradient
    agree to 1e-12 of the quantity's scale (max(1, max|want|): fp64 rounding is relative, and the per-head tau gradient of
    the tau = 0.011 head is O(10^2))."""
    d = golden
    e, heads, _ = (int(v) for v in d["meta"])
    sizes = [int(s) for s in d["sizes"]]
    x, pos, g, par, tau = fixture_case(d, case)
    n = x.shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))  # token slot s lives on flat row perm[s]
    csr = amr.host_csr(sizes, perm)
    scatter = lambda t: torch.zeros_like(t).index_copy(0, perm, t)  # noqa: E731  (slot order -> flat row order)
    xf, pf, gf = scatter(x).requires_grad_(), scatter(pos), scatter(g)
    leaves = {k: v.clone().requires_grad_() for k, v in par.items()}
    tau_l = None if tau is None else tau.clone().requires_grad_()
    out = amr.module_forward(xf, pf, leaves["in_proj_weight"], leaves["in_proj_bias"], leaves["out_proj_weight"],
                             leaves["out_proj_bias"], tau_l, float(d["tau_min"]), heads, csr)
    (out * gf).sum().backward()
    got = {"out": out.detach()[perm], "g_x": xf.grad[perm], "g_in_w": leaves["in_proj_weight"].grad,
           "g_in_b": leaves["in_proj_bias"].grad, "g_out_w": leaves["out_proj_weight"].grad}
    if tau is not None:
        got["g_tau"] = tau_l.grad
        assert float(tau_l.grad.reshape(-1)[-1]) == 0.0  # tau 0.004 <= tau_min: clamped
    for k, have in got.items():
        want = torch.from_numpy(d[f"{case}_{k}"])
        assert have.shape == want.shape, k
        err = float((have - want).abs().max())
        print(f"{case} {k}: err {err:.3e} scale {float(want.abs().max()):.3e}")
        assert err <= 1e-12 * max(1.0, float(want.abs().max())), (k, err)


REF_SHAPES = {"in_proj_weight": (144, 48), "in_proj_bias": (144,), "out_proj.weight": (48, 48), "out_proj.bias": (48,)}


@pytest.mark.parametrize("cosine,non_shared,tau_shape", [(True, False, (1, 1, 1)), (True, True, (1, 8, 1, 1)),
                                                          (False, False, None), (False, True, None)])
def test_constructor_options_state_dict_and_checkpoint(cosine, non_shared, tau_shape):
    """The four option combinations build the reference's keys and shapes (cosine_msa.py:413-432: cosine=False has no tau
    whatever non_shared_tau says), a state dict shaped like the reference's loads strictly, and a shared-tau dict is
    refused by a per-head module and the reverse."""
    from openseg3d_amd import checkpoint, swformer
    m = swformer.CosineMultiheadAttention(48, 8, dropout=0.1, tau_min=0.01, cosine=cosine, non_shared_tau=non_shared)
    want = dict(REF_SHAPES)
    if tau_shape is not None:
        want["tau"] = tau_shape
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert (m.tau is None) == (tau_shape is None)
    if tau_shape is not None:
        assert isinstance(m.tau, torch.nn.Parameter) and torch.equal(m.tau.detach(), torch.ones(tau_shape))
    ref_sd = {k: torch.full(s, 0.25) for k, s in want.items()}
    res = checkpoint.load_reference_checkpoint(m, {"model": ref_sd}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, ref_sd[k]) for k, v in m.state_dict().items())
    # the wrong temperature form for this module
    for other in ((1, 1, 1), (1, 8, 1, 1)):
        if other != tau_shape:
            bad = dict(ref_sd, tau=torch.ones(other))
            with pytest.raises(RuntimeError):
                checkpoint.load_reference_checkpoint(m, bad, strict=True)
    if tau_shape is not None:
        with pytest.raises(RuntimeError):
            checkpoint.load_reference_checkpoint(m, {k: v for k, v in ref_sd.items() if k != "tau"}, strict=True)
    # the enclosing modules hand the options down; the defaults build today's modules
    layer = swformer.EncoderLayer(96, 8, 192, cosine=cosine, non_shared_tau=non_shared)
    at = layer.win_attn.self_attn
    assert (at.cosine, at.non_shared_tau) == (cosine, non_shared)
    assert ("win_attn.self_attn.tau" in layer.state_dict()) == (tau_shape is not None)
    block = swformer.SWFormerBlock(96, 8, depth=2, cosine=cosine, non_shared_tau=non_shared)
    taus = [tuple(v.shape) for k, v in block.state_dict().items() if k.endswith(".tau")]
    assert taus == ([] if tau_shape is None else [tau_shape] * 2)
    wa = swformer.WindowAttention(96, 8, 0.1, cosine, 0.02)  # the reference's positional order (point_transformer_layer.py:222-231)
    assert wa.self_attn.cosine == cosine and wa.self_attn.tau_min == 0.02


def test_defaults_build_todays_modules():
    from openseg3d_amd import swformer
    torch.manual_seed(0)
    a = swformer.SWFormerBlock(48, 8, depth=2)
    torch.manual_seed(0)
    b = swformer.SWFormerBlock(48, 8, depth=2, cosine=True, non_shared_tau=False)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert tuple(sa["layers.0.win_attn.self_attn.tau"].shape) == (1, 1, 1)


def test_ops_refuse_other_tau_forms_by_name():
    """(The tau forms are checked before the device: a CPU run reaches these messages too.)"""
    from openseg3d_amd import _lib, ops
    qk, v = torch.zeros(4, 192), torch.zeros(4, 96)
    with pytest.raises(_lib.Seg3dError, match=r"\[1, H, 1, 1\].*None"):
        ops.window_attention_packed(qk, v, torch.ones(3), 0.01, 8, None)
    with pytest.raises(_lib.Seg3dError, match="together with dot-product mode"):
        ops.window_attention_packed(qk, v, torch.ones(1, 8, 1, 1), 0.01, 8, None, cosine=False)
    with pytest.raises(_lib.Seg3dError, match="cosine mode needs a tau"):
        ops.window_attention(qk[:, :96], qk[:, 96:], v, None, 0.01, 8, None, cosine=True)


# ------------------------------------------------------------------------------------------ the C entries, fake pointers
COS, DOT = 0, 1


def _fwd(lib, **kw):
    fake = ctypes.c_void_p(4096)
    a = dict(q=fake, k=fake, v=fake, ldq=96, ldk=96, ldv=96, tok=fake, ws=fake, wc=fake, ti=fake, n_tiles=7, qg=fake, n_qg=3,
             m=100, n_win=5, heads=8, dh=12, mode=COS, tau=fake, n_tau=8, tau_min=0.01, p=0.0, seed=0, out=fake, lse=fake)
    a.update(kw)
    return lib.seg3d_window_attn_fwd_modes(a["q"], a["k"], a["v"], a["ldq"], a["ldk"], a["ldv"], a["tok"], a["ws"], a["wc"],
                                           a["ti"], a["n_tiles"], a["qg"], a["n_qg"], a["m"], a["n_win"], a["heads"], a["dh"],
                                           a["mode"], a["tau"], a["n_tau"], a["tau_min"], a["p"], a["seed"], a["out"], a["lse"],
                                           None, 0, None)


def _bwd(lib, **kw):
    fake = ctypes.c_void_p(4096)
    a = dict(q=fake, k=fake, v=fake, ldq=96, ldk=96, ldv=96, out=fake, dout=fake, lse=fake, tok=fake, ws=fake, wc=fake, ti=fake,
             n_tiles=7, qg=fake, n_qg=3, m=100, n_win=5, heads=8, dh=12, mode=COS, tau=fake, n_tau=8, tau_min=0.01, p=0.0, seed=0,
             dq=fake, dk=fake, dv=fake, lddq=96, lddk=96, lddv=96, dtau=fake, work=fake, work_bytes=1 << 40)
    a.update(kw)
    return lib.seg3d_window_attn_bwd_modes(a["q"], a["k"], a["v"], a["ldq"], a["ldk"], a["ldv"], a["out"], a["dout"], a["lse"],
                                           a["tok"], a["ws"], a["wc"], a["ti"], a["n_tiles"], a["qg"], a["n_qg"], a["m"],
                                           a["n_win"], a["heads"], a["dh"], a["mode"], a["tau"], a["n_tau"], a["tau_min"], a["p"],
                                           a["seed"], a["dq"], a["dk"], a["dv"], a["lddq"], a["lddk"], a["lddv"], a["dtau"],
                                           a["work"], a["work_bytes"], None)


def test_mode_entries_refuse_before_any_launch():
    """Every SEG3D_EINVAL / SEG3D_EWORKSPACE of the new entries with addresses that are never read (a refused call returns
    before a launch), and the zero-size calls."""
    from openseg3d_amd import _lib
    lib = _lib.load()
    EINVAL, EWS = _lib.EINVAL, _lib.EWORKSPACE
    odd = ctypes.c_void_p(4096 + 4)
    for call in (_fwd, _bwd):
        # tau counts: neither 1 nor heads (cosine); anything but 0 (dot); an unknown mode
        for n_tau in (0, 2, 3, 7, 9, 16, -1):
            assert call(lib, n_tau=n_tau) == EINVAL, (call.__name__, n_tau)
        for n_tau in (1, 8):
            assert call(lib, mode=DOT, tau=None, n_tau=n_tau, dtau=None) == EINVAL
        assert call(lib, mode=2) == EINVAL and call(lib, mode=-1) == EINVAL
        # tau given in dot mode, missing in cosine mode
        assert call(lib, mode=DOT, n_tau=0, dtau=None) == EINVAL
        assert call(lib, tau=None) == EINVAL and call(lib, tau=None, n_tau=1) == EINVAL
        # rows that are not 16-byte aligned / strides that are no multiple of 4 floats
        assert call(lib, q=odd) == EINVAL and call(lib, ldk=98) == EINVAL
        # head geometries seg3d_window_attn_supported refuses
        for heads, dh in ((3, 12), (6, 6), (8, 32), (17, 24)):
            n_tau = heads
            assert lib.seg3d_window_attn_supported(heads, dh) == 0
            assert call(lib, heads=heads, dh=dh, n_tau=n_tau) == EINVAL, (heads, dh)
            assert call(lib, heads=heads, dh=dh, mode=DOT, tau=None, n_tau=0, dtau=None) == EINVAL, (heads, dh)
        assert call(lib, p=1.0) == EINVAL
        # null operands
        assert call(lib, v=None) == EINVAL and call(lib, ti=None) == EINVAL
        # zero-size calls return OK without touching anything (no dtau to zero: nothing is enqueued)
        for empty in (dict(m=0), dict(n_win=0), dict(n_tiles=0), dict(n_qg=0)):
            assert call(lib, mode=DOT, tau=None, n_tau=0, dtau=None, q=None, k=None, v=None, **empty) == 0, empty
    # a dtau that does not match the mode
    assert _bwd(lib, dtau=None) == EINVAL
    assert _bwd(lib, mode=DOT, tau=None, n_tau=0) == EINVAL  # (dtau given)
    assert _bwd(lib, dq=odd) == EINVAL and _bwd(lib, lddv=50) == EINVAL
    assert _bwd(lib, work=None) == EINVAL
    # the workspace: the query's answer is enough, anything less than the kernels' share of it is refused
    for heads, dh in ((8, 6), (8, 12), (8, 24), (8, 48)):
        for mode, n_tau in ((COS, 8), (COS, 1), (DOT, 0)):
            need = _lib.query("seg3d_window_attn_workspace_bytes_modes", 100, 7, heads, dh, mode, n_tau)
            assert need > 256
            kw = dict(heads=heads, dh=dh, mode=mode, n_tau=n_tau, ldq=heads * dh, ldk=heads * dh, ldv=heads * dh,
                      lddq=heads * dh, lddk=heads * dh, lddv=heads * dh)
            if mode == DOT:
                kw.update(tau=None, dtau=None)
            small = 7 * n_tau * 4 - 4 if dh == 6 and n_tau > 1 else (7 * 4 - 4 if dh == 6 else 64)
            assert _bwd(lib, work_bytes=small, **kw) == EWS, (heads, dh, mode)
        # per-head partials of the vector-ALU path: one per (tile, head), eight times the shared-tau demand
        if dh == 6:
            assert _lib.query("seg3d_window_attn_workspace_bytes_modes", 100, 7, 8, 6, COS, 8) == 7 * 8 * 4 + 256
            assert _lib.query("seg3d_window_attn_workspace_bytes_modes", 100, 7, 8, 6, COS, 1) == \
                _lib.query("seg3d_window_attn_workspace_bytes", 100, 7, 8, 6)
    # the size query refuses what the entries refuse
    for mode, n_tau in ((COS, 3), (DOT, 1), (2, 0)):
        assert _lib.query("seg3d_window_attn_workspace_bytes_modes", 100, 7, 8, 12, mode, n_tau) == 0
    assert _lib.query("seg3d_window_attn_workspace_bytes_modes", 100, 7, 3, 12, COS, 3) == 0


def test_binding_table_header_and_version_agree():
    from openseg3d_amd import _lib
    names = [n for n in _lib.header_symbols() if n.endswith("_modes")]
    assert names == ["seg3d_window_attn_bwd_modes", "seg3d_window_attn_fwd_modes", "seg3d_window_attn_workspace_bytes_modes"]
    assert all(n in _lib.SIGNATURES for n in names)
    text = open(_lib.HEADER_PATH).read()
    for cite in ("cosine_msa.py:413-432", ":156-160", ":163-165", "point_transformer_layer.py:222-231"):
        assert cite in text, cite
    assert f"#define SEG3D_ATTN_COSINE {_lib.ATTN_COSINE}" in text and f"#define SEG3D_ATTN_DOT {_lib.ATTN_DOT}" in text
    assert _lib.ABI_VERSION >= 56 and _lib.load().seg3d_abi_version() == _lib.ABI_VERSION
