"""Argument validation of the fused criterion entries (seg3d_criterion_workspace_bytes / _fwd / _bwd): bad arguments and a
short workspace are refused before anything is enqueued, so these run without a GPU (the pointers are never read)."""
import ctypes


def _table(sizes, ptr=0x1000):
    from openseg3d_amd import ops
    t = ops.CriterionTable()
    t.n_heads = len(sizes)
    for i, n in enumerate(sizes[:ops.CRITERION_MAX_HEADS]):
        t.heads[i].logits, t.heads[i].labels, t.heads[i].n, t.heads[i].weight = ptr, ptr, n, 1.0
    return t


def _fwd(lib, tab, c, terms=3, ws_bytes=1 << 40):
    fake = ctypes.c_void_p(0x1000)
    return lib.seg3d_criterion_fwd(ctypes.byref(tab) if tab is not None else None, c, terms, 255, 0.7, 1.0, 1.0, fake, fake,
                                   fake, fake, fake, ws_bytes, None)


def _bwd(lib, tab, c, terms=3):
    fake = ctypes.c_void_p(0x1000)
    out = (ctypes.c_void_p * 4)(0x1000, 0x1000, 0x1000, 0x1000)
    return lib.seg3d_criterion_bwd(ctypes.byref(tab) if tab is not None else None, c, terms, 1.0, 1.0, fake, fake, fake, fake,
                                   out, None)


def test_fused_criterion_refuses_bad_arguments_before_any_launch():
    from openseg3d_amd import _lib
    lib = _lib.load()
    good = _table([100, 50, 7])
    cases = [(None, 22, 3),                          # null table
             (_table([10, 10, 10, 10, 10]), 22, 3),  # more than four heads
             (_table([]), 22, 3),                    # no head
             (good, 0, 3), (good, 65, 3),            # c outside 1..64
             (good, 22, 0), (good, 22, 4),           # no term / unknown term bit
             (_table([100, -1]), 22, 3),             # negative row count
             (_table([100, 50], ptr=None), 22, 3),   # rows without logits / labels
             (_table([1 << 25, 1 << 25]), 32, 3),    # sum n * c == 2^31
             (_table([(1 << 31) // 22 + 1]), 22, 3)]
    for tab, c, terms in cases:
        assert _fwd(lib, tab, c, terms) == _lib.EINVAL, (c, terms)
        assert _bwd(lib, tab, c, terms) == _lib.EINVAL, (c, terms)
        assert lib.seg3d_criterion_workspace_bytes(ctypes.byref(tab) if tab is not None else None, c, terms) == 0
    # output pointers
    fake = ctypes.c_void_p(0x1000)
    assert lib.seg3d_criterion_fwd(ctypes.byref(good), 22, 3, 255, 0.7, 1.0, 1.0, fake, fake, None, fake, fake, 1 << 40,
                                   None) == _lib.EINVAL
    assert lib.seg3d_criterion_bwd(ctypes.byref(good), 22, 3, 1.0, 1.0, fake, fake, fake, fake, None, None) == _lib.EINVAL


def test_fused_criterion_refuses_a_short_workspace():
    """The call's own buffers (sort keys and values, chunk tables, partials) alone exceed these sizes: refused before the
    sort's scratch size is even asked for."""
    from openseg3d_amd import _lib
    lib = _lib.load()
    tab = _table([4101, 2049, 1])
    rows = 4101 + 2049 + 1
    for ws_bytes in (0, 256, rows * 22 * 24 - 1):  # two 8-byte key and two 4-byte value buffers of rows * c elements
        assert _fwd(lib, tab, 22, 3, ws_bytes) == _lib.EWORKSPACE, ws_bytes
    assert _fwd(lib, tab, 22, 1, 0) == _lib.EWORKSPACE  # ce only: the per-workgroup partials
    assert lib.seg3d_criterion_fwd(ctypes.byref(tab), 22, 3, 255, 0.7, 1.0, 1.0, None, None, ctypes.c_void_p(0x1000),
                                   ctypes.c_void_p(0x1000), None, 1 << 40, None) == _lib.EINVAL  # lse / coef missing
