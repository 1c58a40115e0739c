"""query_and_group / knn_interpolate on the host: the _host entries of csrc/pointops.hip (reached through CPU tensors and
numpy arrays) against the restatements of tests/pointops_ref.py -- bit for bit against the float32 one, within bounds
derived from the case (u = 2^-24, list lengths, K) against the float64 one.  Runs without a GPU."""
import numpy as np
import pytest
import torch

import pointops_ref as ref
from pointops_ref import SHAPES, make_case


@pytest.fixture(scope="module")
def ops():
    from openseg3d_amd import ops
    return ops


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else a
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def within(got, want, bound, what):
    got = got.detach().numpy() if isinstance(got, torch.Tensor) else got
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max error / bound = {worst:.3f}")
    assert (err <= bound).all(), f"{what}: error {err.max():.3e} exceeds its bound (ratio {worst:.3f})"


def run_group(ops, case, use_xyz=True, grads=(True, True, True), new_xyz=True):
    """-> (out, dxyz, dnew_xyz, dfeat) through the public call on CPU tensors."""
    t = {k: torch.from_numpy(case[k]) for k in ("xyz", "new_xyz", "feat", "idx")}
    for name, g in zip(("xyz", "new_xyz", "feat"), grads):
        t[name].requires_grad_(g)
    out = ops.query_and_group(case["k"], t["xyz"], t["new_xyz"] if new_xyz else None, t["feat"], t["idx"], None, None,
                              use_xyz=use_xyz)
    if out.requires_grad:
        dout = case["dout_g"] if use_xyz else np.ascontiguousarray(case["dout_g"][:, :, 3:])
        out.backward(torch.from_numpy(dout))
    return out.detach(), t["xyz"].grad, t["new_xyz"].grad, t["feat"].grad


def run_interp(ops, case, grad=True):
    feat = torch.from_numpy(case["feat"]).requires_grad_(grad)
    out = ops.knn_interpolate(feat, torch.from_numpy(case["idx"]), torch.from_numpy(case["dist"]))
    if grad:
        out.backward(torch.from_numpy(case["dout_i"]))
    return out.detach(), feat.grad


CASES = [dict(zip("nmkc", s), seed=i, outside=i % 2 == 1, scale=10.0 ** (i % 7 - 3)) for i, s in enumerate(SHAPES)]


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "n{n}-m{m}-k{k}-c{c}".format(**s))
def test_grouping_equals_restatements(ops, spec):
    case = make_case(**spec)
    n = case["n"]
    for use_xyz in (True, False):
        out, dxyz, dnew, dfeat = run_group(ops, case, use_xyz)
        dout = case["dout_g"] if use_xyz else np.ascontiguousarray(case["dout_g"][:, :, 3:])
        # forward: exact (a copy and one float32 subtraction)
        assert same_bits(out, ref.group_f32(case["xyz"], case["new_xyz"], case["feat"], case["idx"], use_xyz))
        wx, wq, wf = ref.group_bwd_f32(dout, case["idx"], n, use_xyz)
        assert same_bits(dfeat, wf)
        f64 = ref.group_bwd_f64(case["xyz"], case["new_xyz"], case["feat"], case["idx"], dout, use_xyz)
        within(dfeat, f64["dfeat"], f64["dfeat_bound"], "dfeat")
        if use_xyz:
            assert same_bits(dxyz, wx) and same_bits(dnew, wq)
            within(dxyz, f64["dxyz"], f64["dxyz_bound"], "dxyz")
            within(dnew, f64["dnew_xyz"], f64["dnew_xyz_bound"], "dnew_xyz")
        else:
            assert dxyz is None and dnew is None


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "n{n}-m{m}-k{k}-c{c}".format(**s))
def test_interpolation_equals_restatements(ops, spec):
    case = make_case(**spec)
    out, dfeat = run_interp(ops, case)
    want, w = ref.interp_f32(case["feat"], case["idx"], case["dist"])
    assert same_bits(out, want)
    assert same_bits(dfeat, ref.interp_bwd_f32(case["dout_i"], w, case["idx"], case["n"]))
    w64, bound = ref.interp_f64(case["feat"], case["idx"], case["dist"])
    within(out, w64, bound, "out")
    g64, gbound = ref.interp_bwd_f64(case["feat"], case["idx"], case["dist"], case["dout_i"])
    within(dfeat, g64, gbound, "dfeat")
    # numpy in, numpy out: the same host entry
    got = ops.knn_interpolate(case["feat"], case["idx"], case["dist"])
    assert isinstance(got, np.ndarray) and same_bits(got, want)


@pytest.mark.parametrize("k", [1, 3, 16, 64])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_interpolation_bound_with_zero_distances_and_far_slots(ops, k, scale):
    case = make_case(200, 300, k, 5, seed=k, scale=scale)
    case["dist"][::3, 0] = 0       # a query on top of a source row
    case["dist"][1::3, -1] = 1e5   # a slot beyond a short segment
    out, _ = run_interp(ops, case, grad=False)
    want, bound = ref.interp_f64(case["feat"], case["idx"], case["dist"])
    within(out, want, bound, f"out k={k} scale={scale}")
    w = ref.interp_weights_f32(case["dist"])
    if k > 1:
        # a 1e5 slot beside real neighbours: weight 1e-5 / norm <= 1e-5 * (the nearest neighbour's distance + 1e-8)
        far = w[1::3, -1]
        assert (far <= 1e-5 * (case["dist"][1::3, :-1].min(1).astype(np.float64) + 1e-8) * 1.001).all()
        # a zero distance (reciprocal 1e8) where the row's other slots are farther than 1e-3: norm <= 1e8 + (K - 1) 1e3, so
        # the weight is 1 to within (K - 1) 1e-5, plus (K + 4) u of float32 rounding
        d = case["dist"][::3]
        rows = (d[:, 1:] > 1e-3).all(1)
        assert rows.any()
        assert (np.abs(1.0 - w[::3][rows, 0].astype(np.float64)) <= (k - 1) * 1e-5 + (k + 4) * ref.U).all()
    else:
        assert (w == 1).all()


def test_hub_row_is_summed_in_chunks(ops):
    """Every query lists source row 7 first: L_7 = m = 3 CHUNK + 5, cut into 4 chunks; a list of exactly CHUNK and one of
    CHUNK + 1 entries sit on both sides of the chunk length."""
    m = 3 * ref.CHUNK + 5
    case = make_case(40, m, 3, 6, seed=3, hub=7)
    case["idx"][:, 1] = np.where(np.arange(m) < ref.CHUNK, 8, 9)
    case["idx"][:, 2] = np.where(np.arange(m) <= ref.CHUNK, 10, 11 + np.arange(m) % 5)
    lengths = np.bincount(case["idx"].reshape(-1), minlength=40)
    assert lengths[7] == m and lengths[8] == ref.CHUNK and lengths[10] == ref.CHUNK + 1
    out, dxyz, dnew, dfeat = run_group(ops, case)
    wx, wq, wf = ref.group_bwd_f32(case["dout_g"], case["idx"], 40)
    assert same_bits(dxyz, wx) and same_bits(dnew, wq) and same_bits(dfeat, wf)
    f64 = ref.group_bwd_f64(case["xyz"], case["new_xyz"], case["feat"], case["idx"], case["dout_g"])
    within(dfeat, f64["dfeat"], f64["dfeat_bound"], "hub dfeat")
    out, g = run_interp(ops, case)
    _, w = ref.interp_f32(case["feat"], case["idx"], case["dist"])
    assert same_bits(g, ref.interp_bwd_f32(case["dout_i"], w, case["idx"], 40))
    g64, gbound = ref.interp_bwd_f64(case["feat"], case["idx"], case["dist"], case["dout_i"])
    within(g, g64, gbound, "hub interpolation dfeat")


def test_rows_read_by_nobody_get_exact_zero(ops):
    case = make_case(50, 30, 4, 7, seed=4, n_read=20)
    _, dxyz, _, dfeat = run_group(ops, case)
    assert not bits(dxyz[20:]).any() and not bits(dfeat[20:]).any() and bits(dfeat[:20]).any()
    _, g = run_interp(ops, case)
    assert not bits(g[20:]).any() and bits(g[:20]).any()


def test_outside_indices_are_defined(ops):
    case = make_case(9, 6, 4, 5, seed=5)
    case["idx"][:] = np.array([[0, -1, 9, 3], [ref.INT32_MAX, ref.INT32_MIN, 8, 8], [-1, -1, -1, -1], [1, 2, 3, 4],
                               [10, 0, 0, -5], [8, 9, 8, 9]], np.int32)
    ok = ref.inside(case["idx"], 9)
    out, dxyz, dnew, dfeat = run_group(ops, case)
    assert not bits(out[torch.from_numpy(~ok)]).any()  # the whole slot of 3 + c values is zero
    assert not (dnew[2] != 0).any()  # no slot inside: no gradient (the entry returns -0.0)
    listed = np.bincount(case["idx"][ok], minlength=9) > 0
    assert not bits(dfeat[torch.from_numpy(~listed)]).any()
    # interpolation: the slot adds nothing, its reciprocal stays in the norm -> the weights of a row still sum to 1 over
    # all K slots, and a row with no slot inside is zero
    out, g = run_interp(ops, case)
    want, w = ref.interp_f32(case["feat"], case["idx"], case["dist"])
    assert same_bits(out, want) and not bits(out[2]).any()
    assert np.allclose(w.sum(1), 1, atol=32 * ref.U)  # (K + 4) u on every weight, K u for this sum
    assert not bits(g[torch.from_numpy(~listed)]).any()


def test_empty_and_defaults(ops):
    case = make_case(12, 0, 3, 4, seed=6)
    out, dxyz, dnew, dfeat = run_group(ops, case)
    assert out.shape == (0, 3, 7) and dnew.shape == (0, 3) and not dfeat.numpy().any() and not dxyz.numpy().any()
    out, g = run_interp(ops, case)
    assert out.shape == (0, 4) and g.shape == (12, 4) and not g.numpy().any()
    # n = 0: every index is outside
    case = make_case(0, 5, 2, 4, seed=7)
    out, _, _, dfeat = run_group(ops, case)
    assert out.shape == (5, 2, 7) and not out.numpy().any() and dfeat.shape == (0, 4)
    # new_xyz=None means xyz (the reference asserts on None before it reaches its default)
    case = make_case(20, 20, 3, 4, seed=8)
    case["new_xyz"] = case["xyz"]
    a = run_group(ops, case)
    b = run_group(ops, case, new_xyz=False)
    assert same_bits(a[0], b[0].numpy()) and same_bits(a[3], b[3].numpy())
    # xyz and new_xyz are then one tensor: its gradient is the sum of both roles
    assert torch.allclose(b[1], a[1] + a[2], rtol=0, atol=1e-5)
    # use_xyz=False: [m, K, c]
    out = run_group(ops, case, use_xyz=False)[0]
    assert out.shape == (20, 3, 4) and same_bits(out, case["feat"][case["idx"].astype(np.int64)])


def test_needs_input_grad_subsets(ops):
    case = make_case(30, 25, 4, 6, seed=9)
    full = run_group(ops, case)
    only_feat = run_group(ops, case, grads=(False, False, True))
    assert only_feat[1] is None and only_feat[2] is None and same_bits(only_feat[3], full[3].numpy())
    only_xyz = run_group(ops, case, grads=(True, False, False))
    assert only_xyz[2] is None and only_xyz[3] is None and same_bits(only_xyz[1], full[1].numpy())
    only_new = run_group(ops, case, grads=(False, True, False))
    assert only_new[1] is None and only_new[3] is None and same_bits(only_new[2], full[2].numpy())
    none = run_group(ops, case, grads=(False, False, False))
    assert not none[0].requires_grad and same_bits(none[0], full[0].numpy())
    out, g = run_interp(ops, case, grad=False)
    assert g is None and same_bits(out, run_interp(ops, case)[0].numpy())


def test_argument_errors(ops):
    from openseg3d_amd import _lib
    case = make_case(10, 8, 3, 4, seed=10)
    t = {k: torch.from_numpy(case[k]) for k in ("xyz", "new_xyz", "feat", "idx", "dist")}
    qg = ops.query_and_group
    with pytest.raises(ValueError, match=r"\(10, 2\)"):  # non-contiguous
        qg(3, t["xyz"], t["new_xyz"], t["feat"][:, ::2], t["idx"], None, None)
    with pytest.raises(ValueError, match="float64"):
        qg(3, t["xyz"].double(), t["new_xyz"], t["feat"], t["idx"], None, None)
    with pytest.raises(ValueError, match=r"\(24,\)"):
        qg(3, t["xyz"], t["new_xyz"], t["feat"], t["idx"].reshape(-1), None, None)
    with pytest.raises(ValueError, match=r"\(7, 3\)"):  # not [m, K]
        qg(3, t["xyz"], t["new_xyz"], t["feat"], t["idx"][:7], None, None)
    with pytest.raises(ValueError, match="65"):
        qg(65, t["xyz"], t["new_xyz"], t["feat"], torch.zeros((8, 65), dtype=torch.int32), None, None)
    with pytest.raises(ValueError):
        qg(0, t["xyz"], t["new_xyz"], t["feat"], torch.zeros((8, 0), dtype=torch.int32), None, None)
    with pytest.raises(_lib.Seg3dError, match="knn_query"):  # idx=None needs the device
        qg(3, t["xyz"], t["new_xyz"], t["feat"], None, torch.tensor([10]), torch.tensor([8]))
    with pytest.raises(_lib.Seg3dError, match="knn_query"):
        ops.interpolation(t["xyz"], t["new_xyz"], t["feat"], torch.tensor([10]), torch.tensor([8]))
    with pytest.raises(ValueError, match=r"\(8, 2\)"):
        ops.knn_interpolate(t["feat"], t["idx"], t["dist"][:, :2])
    with pytest.raises(ValueError, match="float64"):
        ops.knn_interpolate(t["feat"], t["idx"], t["dist"].double())
    with pytest.raises(ValueError, match="int64"):  # no silent narrowing
        qg(3, t["xyz"], t["new_xyz"], t["feat"], t["idx"].long(), None, None)
    with pytest.raises(ValueError, match="65"):
        ops.knn_interpolate(t["feat"], torch.zeros((8, 65), dtype=torch.int32), torch.zeros((8, 65)))
    # the C entries themselves: K outside 1..64, c < 1 and negative counts are SEG3D_EINVAL, checked before anything else
    lib = _lib.load()
    for n, m, k, c in ((10, 8, 0, 4), (10, 8, 65, 4), (10, 8, 3, 0), (-1, 8, 3, 4), (10, -1, 3, 4)):
        assert lib.seg3d_group_points_fwd_host(None, None, None, None, n, m, k, c, None) == _lib.EINVAL
        assert lib.seg3d_group_points_fwd(None, None, None, None, n, m, k, c, None, None) == _lib.EINVAL
        assert lib.seg3d_knn_interpolate_fwd_host(None, None, None, n, m, k, c, None, None) == _lib.EINVAL
        assert lib.seg3d_knn_interpolate_bwd(None, None, None, None, None, n, m, k, c, None, None, 0, None) == _lib.EINVAL
        assert lib.seg3d_group_points_bwd(None, None, None, None, n, m, k, c, 1, None, None, None, None, 0, None) == _lib.EINVAL
    for n, m in ((0, 8), (10, 0)):  # nothing to do: OK before any pointer is looked at
        assert lib.seg3d_group_points_fwd(None, None, None, None, n, m, 3, 4, None, None) == 0
        assert lib.seg3d_knn_interpolate_fwd(None, None, None, n, m, 3, 4, None, None, None) == 0
    assert _lib.query("seg3d_pointops_scratch_bytes", 1000, 16, 35) >= (16000 // ref.CHUNK + 1) * 35 * 4
