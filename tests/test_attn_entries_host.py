"""Every refusal of the shared-tau attention entries (seg3d_window_attn_fwd / _bwd / _workspace_bytes) with addresses that
are never read: a refused or empty call returns before a launch or a memset, so the table runs without a GPU.  The codes
were recorded from the library as it stood before the entries were folded onto one path with the _modes entries
(test_attn_modes_host.py tables those); they are what each call has always returned, not what it ought to."""
import ctypes

import pytest

FAKE, ODD = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
OK, EINVAL, EWS = 0, -1, -2
EMPTY = (dict(m=0), dict(n_win=0), dict(n_tiles=0), dict(n_qg=0))
FWD_PTRS = ("q", "k", "v", "tok", "ws", "wc", "ti", "qg", "out")
BWD_PTRS = ("q", "k", "v", "out", "dout", "lse", "tok", "ws", "wc", "ti", "qg", "dq", "dk", "dv")


def _fwd(lib, **kw):
    a = dict(q=FAKE, k=FAKE, v=FAKE, ldq=96, ldk=96, ldv=96, tok=FAKE, ws=FAKE, wc=FAKE, wt0=FAKE, ti=FAKE, n_tiles=7, qg=FAKE,
             n_qg=3, m=100, n_win=5, heads=8, dh=12, tau=FAKE, tau_min=0.01, p=0.0, seed=0, out=FAKE, lse=FAKE)
    a.update(kw)
    return lib.seg3d_window_attn_fwd(a["q"], a["k"], a["v"], a["ldq"], a["ldk"], a["ldv"], a["tok"], a["ws"], a["wc"], a["wt0"],
                                     a["ti"], a["n_tiles"], a["qg"], a["n_qg"], a["m"], a["n_win"], a["heads"], a["dh"], a["tau"],
                                     a["tau_min"], a["p"], a["seed"], a["out"], a["lse"], None, 0, None)


def _bwd(lib, **kw):
    a = dict(q=FAKE, k=FAKE, v=FAKE, ldq=96, ldk=96, ldv=96, out=FAKE, dout=FAKE, lse=FAKE, tok=FAKE, ws=FAKE, wc=FAKE, wt0=FAKE,
             ti=FAKE, n_tiles=7, qg=FAKE, n_qg=3, m=100, n_win=5, heads=8, dh=12, tau=FAKE, tau_min=0.01, p=0.0, seed=0, dq=FAKE,
             dk=FAKE, dv=FAKE, lddq=96, lddk=96, lddv=96, dtau=FAKE, work=FAKE, work_bytes=1 << 40)
    a.update(kw)
    return lib.seg3d_window_attn_bwd(a["q"], a["k"], a["v"], a["ldq"], a["ldk"], a["ldv"], a["out"], a["dout"], a["lse"], a["tok"],
                                     a["ws"], a["wc"], a["wt0"], a["ti"], a["n_tiles"], a["qg"], a["n_qg"], a["m"], a["n_win"],
                                     a["heads"], a["dh"], a["tau"], a["tau_min"], a["p"], a["seed"], a["dq"], a["dk"], a["dv"],
                                     a["lddq"], a["lddk"], a["lddv"], a["dtau"], a["work"], a["work_bytes"], None)


def _rows():
    """(entry, arguments that differ from a valid call, recorded return code)"""
    rows = []
    for call, ptrs in ((_fwd, FWD_PTRS), (_bwd, BWD_PTRS)):
        rows += [(call, {p: None}, EINVAL) for p in ptrs]  # null operands, one at a time
        rows += [(call, dict(tau=None), EINVAL)]
        rows += [(call, dict(heads=0), EINVAL), (call, dict(heads=17, dh=24), EINVAL), (call, dict(heads=17, dh=12), EINVAL)]
        rows += [(call, dict(heads=h, dh=d, ldq=h * d, ldk=h * d, ldv=h * d, lddq=h * d, lddk=h * d, lddv=h * d)
                  if call is _bwd else dict(heads=h, dh=d, ldq=h * d, ldk=h * d, ldv=h * d), EINVAL)
                 for h, d in ((3, 12), (6, 6), (8, 32))]
        rows += [(call, dict(p=1.0), EINVAL), (call, dict(p=-0.25), EINVAL), (call, dict(p=float("nan")), EINVAL)]
        rows += [(call, {p: ODD}, EINVAL) for p in ("q", "k", "v")]  # rows are moved in 16-byte pieces
        rows += [(call, {ld: 98}, EINVAL) for ld in ("ldq", "ldk", "ldv")]
        rows += [(call, dict(m=-1), EINVAL), (call, dict(n_win=-1), EINVAL), (call, dict(n_tiles=-1), EINVAL),
                 (call, dict(n_qg=-1), EINVAL)]
        # the empty problem comes first: null operands, a null tau, even a refused head count return OK (no dtau: no memset)
        nulls = {p: None for p in ptrs}
        for empty in EMPTY:
            rows += [(call, dict(nulls, dtau=None, work=None, **empty), OK),
                     (call, dict(nulls, dtau=None, work=None, tau=None, **empty), OK),
                     (call, dict(dtau=None, tau=None, **empty), OK),
                     (call, dict(dtau=None, heads=17, dh=5, **empty), OK)]
    # the forward alone: an empty problem is OK whatever the dropout probability, the backward looks at p first
    rows += [(_fwd, dict(p=1.0, m=0), OK), (_bwd, dict(p=1.0, m=0, dtau=None), EINVAL), (_bwd, dict(p=-0.25, n_tiles=0, dtau=None), EINVAL)]
    # the forward takes no lse-less call to the vector-ALU kernel and needs no workspace; nothing of that is a refusal.
    # the backward's own operands
    rows += [(_bwd, {p: ODD}, EINVAL) for p in ("dq", "dk", "dv")]
    rows += [(_bwd, {ld: 50}, EINVAL) for ld in ("lddq", "lddk", "lddv")]
    rows += [(_bwd, dict(dtau=None), EINVAL), (_bwd, dict(work=None), EINVAL)]
    # 12 heads of 6 channels: a forward exists (not in this table: it would launch), no backward
    rows += [(_bwd, dict(heads=12, dh=6, ldq=72, ldk=72, ldv=72, lddq=72, lddk=72, lddv=72), EINVAL)]
    return rows


def _label(row):
    call, kw, _ = row
    return call.__name__ + ":" + ",".join(f"{k}={'odd' if v is ODD else v}" for k, v in kw.items())


@pytest.fixture(scope="module")
def lib():
    from openseg3d_amd import _lib
    assert (_lib.EINVAL, _lib.EWORKSPACE) == (EINVAL, EWS)
    return _lib.load()


def test_shared_entries_refuse_before_any_launch(lib):
    rows = _rows()
    assert len(rows) > 100
    got = [(_label(r), r[0](lib, **r[1])) for r in rows]
    want = [(_label(r), r[2]) for r in rows]
    assert got == want, [(g, w[1]) for g, w in zip(got, want) if g != w]


# seg3d_window_attn_workspace_bytes(m=100, n_tiles=7, heads, dh), recorded
# (the query does not look at the 16-head limit of the entries: 17 heads of 24 get a size)
WORKSPACE = {(8, 6): 284, (8, 12): 5888, (8, 24): 4864, (8, 48): 4864, (4, 6): 284, (16, 6): 284, (4, 12): 3328, (16, 12): 11008,
             (1, 24): 1280, (16, 48): 8960, (12, 6): 0, (3, 12): 0, (6, 6): 0, (8, 32): 0, (17, 24): 9728, (0, 12): 0, (-1, 12): 0}


def test_shared_workspace_query_and_the_backward_one_unit_short(lib):
    from openseg3d_amd import _lib
    got = {g: _lib.query("seg3d_window_attn_workspace_bytes", 100, 7, *g) for g in WORKSPACE}
    assert got == WORKSPACE
    assert _lib.query("seg3d_window_attn_workspace_bytes", -1, 7, 8, 12) == 0
    assert _lib.query("seg3d_window_attn_workspace_bytes", 100, -1, 8, 12) == 0
    assert _lib.query("seg3d_window_attn_workspace_bytes", 0, 0, 8, 6) == 256
    # The query sizes the fused backward for as many chunks as tiles and adds 256 bytes of slack: with n_qgroups = n_tiles
    # the kernels' own demand is the answer less 256, and one byte less than that is refused.
    for dh in (6, 12, 24, 48):
        c = 8 * dh
        need = WORKSPACE[(8, dh)] - 256
        kw = dict(heads=8, dh=dh, n_qg=7, ldq=c, ldk=c, ldv=c, lddq=c, lddk=c, lddv=c)
        assert _bwd(lib, work_bytes=need - 1, **kw) == EWS, dh
        assert _bwd(lib, work_bytes=0, **kw) == EWS, dh
        # the refusals in front of the workspace check keep their code when the workspace is short as well
        assert _bwd(lib, work_bytes=need - 1, **dict(kw, dq=ODD)) == EINVAL, dh
        assert _bwd(lib, work_bytes=need - 1, **dict(kw, dtau=None)) == EINVAL, dh
    # the vector-ALU backward (dh 6) counts tiles, not chunks; the fused one counts the chunks it is given
    assert _bwd(lib, work_bytes=27, heads=8, dh=6, n_qg=3, ldq=48, ldk=48, ldv=48, lddq=48, lddk=48, lddv=48) == EWS
    assert _bwd(lib, work_bytes=64, heads=8, dh=24, n_qg=3, ldq=192, ldk=192, ldv=192, lddq=192, lddk=192, lddv=192) == EWS
