"""Class-weighted cross-entropy and OHEM by keep_ratio on the device (seg3d_ce_select_fwd/bwd in csrc/loss_select.hip) against
the reference's float64 results (tests/golden/losses_select.npz, make_golden_losses_select.py) and against the modules' own
float64 torch composition (test_losses_select_host.py holds that to the reference at 1e-12).

Bar, everywhere a value or a gradient is compared: that of test_gpu_losses_pointwise.py (its ``check``): the larger of 2e-6
relative on the value / 1e-9 + 1e-5 max|grad| on the gradient, and twice the deviation of a float32 torch run of the same
formulas from the float64 result on the same inputs.  Upstream gradient 0.4.

keep_ratio compares every row: a float32 kernel and a float64 composition select the same rows when the losses on the two
sides of the cut are further apart than their float32 errors.  The size sweep asserts that of its own inputs (float64 gap
between the last kept and the first dropped loss >= 1e-5 and >= 16 x the largest per-row error of the float32 composition)
before it compares; with c = 1 every loss is 0 and every gradient is 0 whatever is selected, and there the selection
itself is tested (test_one_class_is_all_ties)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_losses_pointwise import UPSTREAM, check, run, size_inputs
from test_losses_select_host import CASES, make_case, select_kwargs

pytestmark = pytest.mark.gpu

MEAN_WEIGHTED, MEAN_ALL, THRESH, RATIO = 0, 1, 2, 3
SIZES_N = (0, 1, 2, 63, 64, 65, 257, 2049, 70001)
SIZES_C = (1, 3, 22, 64)
RATIOS = (0.3, 0.7, 1.0)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "losses_select.npz")))


def sweep_inputs(n, c):
    """size_inputs of test_gpu_losses_pointwise.py -- but for (70001, 22), where its seed leaves 1.03e-5 between the two
    losses at the unweighted 0.7 cut, 9.7 x the float32 composition's per-row error: short of the 16 x that
    build_size_refs asserts.  The same construction from another seed leaves 22 x at its narrowest cut."""
    if (n, c) != (70001, 22):
        return size_inputs(n, c)
    g = torch.Generator().manual_seed(1000 * n + c + 7919)
    x = torch.randn(n, c, generator=g) * 2.5
    y = torch.randint(0, c, (n,), generator=g)
    y[1::5] = 255
    return x, y


def size_weights(c):
    """the class weights of test_gpu_losses_pointwise.size_modules"""
    return (0.5 + torch.rand(c, generator=torch.Generator().manual_seed(c))).tolist()


def size_cases(c):
    """name -> (module, keyword arguments of ops.cross_entropy_select): keep_ratio with and without weights, and the two
    other modes that carry weights"""
    from openseg3d_amd import losses
    w = size_weights(c)
    cases = {}
    for ratio in RATIOS:
        cases[f"ratio{ratio}"] = (losses.OHEMCrossEntropyLoss(keep_ratio=ratio), dict(keep_ratio=ratio))
        cases[f"ratio{ratio}_weighted"] = (losses.OHEMCrossEntropyLoss(keep_ratio=ratio, class_weight=w),
                                           dict(keep_ratio=ratio, class_weight=w))
    cases["thresh_weighted"] = (losses.OHEMCrossEntropyLoss(keep_thresh=0.7, class_weight=w),
                                dict(keep_thresh=0.7, class_weight=w))
    cases["ce_weighted"] = (losses.CrossEntropyLoss(class_weight=w), dict(class_weight=w, weighted_mean=True))
    return cases


def cut_gap(x, y, w, ratio):
    """(kept, float64 gap between the kept-th largest loss and the next, largest per-row error of the float32 composition);
    the gap is None where no cut runs between two rows (kept = 0 or all)"""
    valid = y != 255
    rows = {}
    for dtype in (torch.float64, torch.float32):
        weight = None if w is None else torch.tensor(w, dtype=dtype)
        rows[dtype] = F.cross_entropy(x.to(dtype), y, weight=weight, ignore_index=255, reduction="none")[valid].double()
    n_valid = int(valid.sum())
    kept = int(n_valid * ratio)
    err = float((rows[torch.float32] - rows[torch.float64]).abs().max()) if n_valid else 0.0
    if kept == 0 or kept >= n_valid:
        return kept, None, err
    ordered = rows[torch.float64].sort(descending=True)[0]
    return kept, float(ordered[kept - 1] - ordered[kept]), err


def build_size_refs():
    """(n, c, case) -> (float64 composition result, float32 composition's deviations, kept or None), once, on the CPU."""
    refs = {}
    for n in SIZES_N:
        for c in SIZES_C:
            if n == 0:
                continue
            x, y = sweep_inputs(n, c)
            for case, (fn, kwargs) in size_cases(c).items():
                kept = None
                if "keep_ratio" in kwargs:
                    kept, gap, row_err = cut_gap(x, y, kwargs.get("class_weight"), kwargs["keep_ratio"])
                    if gap is not None and c > 1:
                        assert gap >= 1e-5 and gap >= 16 * row_err, (n, c, case, gap, row_err)
                    if kept == 0:  # the mean over nothing: NaN in torch, 0 on the device
                        refs[n, c, case] = (None, 0.0, 0.0, 0)
                        continue
                r64 = run(fn, x, y, dtype=torch.float64)
                if np.isnan(r64[0]):  # keep_thresh and no valid row below it (one class: every probability is 1)
                    valid = y != 255
                    probs = F.softmax(x.double(), dim=1)[valid].gather(1, y[valid].unsqueeze(1))
                    assert "thresh" in case and not bool((probs < 0.7).any()) and np.abs(r64[1]).max() == 0.0, (n, c, case)
                    refs[n, c, case] = (None, 0.0, 0.0, 0)
                    continue
                r32 = run(fn, x, y, dtype=torch.float32)
                refs[n, c, case] = (r64, abs(r32[0] - r64[0]), np.abs(r32[1] - r64[1]).max(), kept)
    return refs


@pytest.fixture(scope="module")
def size_refs():
    return build_size_refs()


def raw_forward(x, y, mode, class_weight=None, keep_thresh=0.0, keep_ratio=0.0, ignore_index=255):
    """seg3d_ce_select_fwd itself: (lse [n], stats [2]) on the device."""
    from openseg3d_amd import _lib, ops
    n, c = x.shape
    lse = torch.empty((n,), dtype=torch.float32, device=x.device)
    stats = torch.empty((2,), dtype=torch.float32, device=x.device)
    ws_bytes = _lib.query("seg3d_ce_select_workspace_bytes", n)
    ws = ops._workspace(ws_bytes, x.device)
    w = None if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float32, device=x.device)
    _lib.call("seg3d_ce_select_fwd", ops._ptr(x), ops._ptr(y), n, c, ignore_index, ops._ptr(w) if w is not None else None,
              mode, float(keep_thresh), float(keep_ratio), ops._ptr(lse), ops._ptr(stats), ops._ptr(ws), ws_bytes,
              ops._stream())
    return lse, stats


def counted_rows(lse):
    return torch.nonzero(lse != float("inf")).flatten().cpu().tolist()


@pytest.mark.parametrize("name", CASES)
def test_matches_reference_modules(dev, golden, name):
    """Every fixture case through the new entry points (ops.cross_entropy_select) and through the module that a user builds
    (which, without weights and without keep_ratio, stays on seg3d_cross_entropy_fwd)."""
    from openseg3d_amd import ops
    weights = golden["class_weight"].tolist()
    thresh, ratio = float(golden["keep_thresh"]), float(golden["keep_ratio"])
    x, y = torch.from_numpy(golden["logits"]), torch.from_numpy(golden["labels"])
    ref = (float(golden[name]), golden[name + "_grad"] * UPSTREAM)
    errs = float(golden[name + "_fp32_val_err"]), float(golden[name + "_fp32_grad_err"]) * UPSTREAM
    check(run(ops.cross_entropy_select, x, y, device=dev, **select_kwargs(name, weights, thresh, ratio)), ref, *errs, name)
    check(run(make_case(name, weights, thresh, ratio), x, y, device=dev), ref, *errs, name + " (module)")


@pytest.mark.parametrize("c", SIZES_C)
@pytest.mark.parametrize("n", SIZES_N)
def test_sizes_match_float64_composition(dev, size_refs, n, c):
    """A wave, the wave edge, more than one workgroup (256 rows each), 274 workgroups that each flush a histogram; one
    class, an odd width, the headline width and a wide one."""
    from openseg3d_amd import ops
    x, y = sweep_inputs(n, c)
    for case, (_, kwargs) in size_cases(c).items():
        got = run(ops.cross_entropy_select, x, y, device=dev, ignore_index=255, **kwargs)
        if n == 0:
            assert got[0] == 0.0 and got[1].shape == (0, c), (case, got)
            continue
        ref, fp32_val_err, fp32_grad_err, kept = size_refs[n, c, case]
        if kept == 0:
            assert got[0] == 0.0 and np.abs(got[1]).max() == 0.0, (case, got)
            continue
        check(got, ref, fp32_val_err, fp32_grad_err, f"{case} n={n} c={c}")
        if kept is not None and c > 1:  # exactly the kept rows carry a gradient
            assert int(np.abs(got[1]).max(axis=1).astype(bool).sum()) == kept, (case, n, c)


@pytest.mark.parametrize("n", [300, 2049, 70001])
def test_one_class_is_all_ties(dev, n):
    """c = 1: every loss is 0, the whole input is one tie.  Exactly kept rows are counted, and they are the first valid
    ones in row order."""
    x, y = size_inputs(n, 1)
    valid = torch.nonzero(y != 255).flatten().tolist()
    for ratio in (0.3, 0.7):
        kept = int(len(valid) * ratio)
        lse, stats = raw_forward(x.to(dev), y.to(dev), RATIO, keep_ratio=ratio)
        assert stats.cpu().tolist() == [0.0, float(kept)]
        assert counted_rows(lse) == valid[:kept], (n, ratio)


def test_ties_across_workgroups_with_gradient(dev):
    """7 distinct rows, each 300 times (row r is base[r % 7]) over 9 workgroups, some rows ignored: the cut falls inside a
    group of equal losses.  The counted rows and the gradient are those of the stable-sort composition."""
    from openseg3d_amd import losses, ops
    g = torch.Generator().manual_seed(17)
    base = torch.randn(7, 22, generator=g) * 2.5
    x = base.repeat(300, 1)
    y = (torch.arange(2100) % 7) * 3
    y[5::11] = 255
    per_group = F.cross_entropy(base.double(), torch.arange(7) * 3, reduction="none").sort()[0]
    assert float((per_group[1:] - per_group[:-1]).min()) > 1e-3  # the groups are far apart
    per_row = F.cross_entropy(x.double(), y, ignore_index=255, reduction="none")[y != 255].sort(descending=True)[0]
    for ratio in (0.5, 0.2):
        fn = losses.OHEMCrossEntropyLoss(keep_ratio=ratio)
        r64 = run(fn, x, y, dtype=torch.float64)
        r32 = run(fn, x, y, dtype=torch.float32)
        want_rows = np.nonzero(np.abs(r64[1]).max(axis=1))[0].tolist()
        n_valid = int((y != 255).sum())
        kept = int(n_valid * ratio)
        assert len(want_rows) == kept and float(per_row[kept - 1]) == float(per_row[kept])  # the cut is inside a group
        lse, stats = raw_forward(x.to(dev), y.to(dev), RATIO, keep_ratio=ratio)
        assert counted_rows(lse) == want_rows and float(stats[1]) == len(want_rows)
        got = run(ops.cross_entropy_select, x, y, device=dev, ignore_index=255, keep_ratio=ratio)
        check(got, r64, abs(r32[0] - r64[0]), np.abs(r32[1] - r64[1]).max(), f"ties ratio {ratio}")
        assert np.nonzero(np.abs(got[1]).max(axis=1))[0].tolist() == want_rows


def test_keep_count_is_pythons(dev):
    """kept = int(n_valid * keep_ratio) in float64, as the reference computes it -- also where the product lands a hair
    beside an integer (0.7 * 10, 0.3 * 90, 0.1 * 30, n / 3)."""
    x, _ = size_inputs(3335, 3)
    x = x.to(dev)
    for n_valid in (1, 3, 10, 30, 90, 1000, 3333):
        y = torch.full((3335,), 255)
        y[torch.randperm(3335, generator=torch.Generator().manual_seed(n_valid))[:n_valid]] = 1
        y = y.to(dev)
        for ratio in (0.1, 0.3, 1.0 / 3.0, 0.7, 0.29, 0.999999):
            lse, stats = raw_forward(x, y, RATIO, keep_ratio=ratio)
            kept = int(n_valid * ratio)
            assert float(stats[1]) == kept and len(counted_rows(lse)) == kept, (n_valid, ratio)


def test_special_values(dev):
    from openseg3d_amd import losses, ops
    n, c = 700, 22
    x, y = size_inputs(n, c)
    valid = torch.nonzero(y != 255).flatten()
    # a NaN loss ranks above every other, +inf included
    xn = x.clone()
    nan_row, inf_row = int(valid[100]), int(valid[7])
    xn[nan_row, 3] = float("nan")
    xn[inf_row] = 0.0
    xn[inf_row, int(y[inf_row])] = float("-inf")  # loss +inf
    lse, stats = raw_forward(xn.to(dev), y.to(dev), RATIO, keep_ratio=1.5 / len(valid))  # kept = 1
    assert float(stats[1]) == 1.0 and counted_rows(lse) == [nan_row] and bool(torch.isnan(stats[0]))
    lse, stats = raw_forward(xn.to(dev), y.to(dev), RATIO, keep_ratio=2.5 / len(valid))  # kept = 2
    assert counted_rows(lse) == sorted([nan_row, inf_row])
    # negative class weights make negative losses: they order below the positive ones, by value
    w = size_weights(c)
    for j in range(0, c, 2):
        w[j] = -w[j]
    fn = losses.OHEMCrossEntropyLoss(keep_ratio=0.7, class_weight=w)
    r64 = run(fn, x, y, dtype=torch.float64)
    r32 = run(fn, x, y, dtype=torch.float32)
    kept, gap, row_err = cut_gap(x, y, w, 0.7)
    assert gap >= 1e-5 and gap >= 16 * row_err, (gap, row_err)
    per_row = F.cross_entropy(x.double(), y, weight=torch.tensor(w, dtype=torch.float64), ignore_index=255, reduction="none")
    assert float(per_row[y != 255].sort(descending=True)[0][kept - 1]) < 0  # the cut lies among the negative losses
    got = run(ops.cross_entropy_select, x, y, device=dev, ignore_index=255, keep_ratio=0.7, class_weight=w)
    check(got, r64, abs(r32[0] - r64[0]), np.abs(r32[1] - r64[1]).max(), "negative weights")
    assert np.array_equal(np.abs(got[1]).max(axis=1) > 0, np.abs(r64[1]).max(axis=1) > 0)
    # -0.0 and +0.0 are one value: a row with loss -0.0 (weight -1, loss 0) ties with the rows of loss +0.0
    xz = torch.zeros(6, 2)
    xz[:, 0] = 200.0  # lse - x[0] == 0 exactly
    yz = torch.tensor([0, 0, 0, 0, 0, 0])
    lse, stats = raw_forward(torch.cat([xz, -xz]).to(dev), torch.cat([yz, yz + 1]).to(dev), RATIO, class_weight=[1.0, -1.0],
                             keep_ratio=0.25)
    assert counted_rows(lse) == [0, 1, 2] and float(stats[0]) == 0.0
    # keep_ratio > 1 keeps every valid row: the plain mean
    lse_all, stats_all = raw_forward(x.to(dev), y.to(dev), MEAN_ALL)
    lse_big, stats_big = raw_forward(x.to(dev), y.to(dev), RATIO, keep_ratio=1.7)
    assert float(stats_big[1]) == len(valid) and torch.equal(lse_big, lse_all) and torch.equal(stats_big, stats_all)
    # nothing valid, and a zero weight sum: 0, not NaN, and a zero gradient
    for kwargs in (dict(keep_ratio=0.3), dict(keep_thresh=0.7, class_weight=w), dict(weighted_mean=True, class_weight=w)):
        val, grad = run(ops.cross_entropy_select, x, torch.full((n,), 255), device=dev, ignore_index=255, **kwargs)
        assert val == 0.0 and np.abs(grad).max() == 0.0, kwargs
    val, grad = run(ops.cross_entropy_select, x, y, device=dev, ignore_index=255, weighted_mean=True, class_weight=[0.0] * c)
    assert val == 0.0 and np.abs(grad).max() == 0.0
    # labels outside [0, c) that are not the ignore label are skipped like it
    y_out = y.clone()
    y_out[y == 255] = torch.tensor([-1, c, 300, -7])[torch.arange(int((y == 255).sum())) % 4]
    a = run(ops.cross_entropy_select, x, y, device=dev, ignore_index=255, keep_ratio=0.3, class_weight=size_weights(c))
    b = run(ops.cross_entropy_select, x, y_out, device=dev, ignore_index=255, keep_ratio=0.3, class_weight=size_weights(c))
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        ops.cross_entropy_select(x.to(dev), y.to(dev), weighted_mean=True, keep_ratio=0.3)
    with pytest.raises(ValueError):
        ops.cross_entropy_select(x.to(dev), y.to(dev), keep_ratio=-0.3)


def test_rows_do_not_depend_on_their_position(dev):
    """A row permutation permutes the gradient, bit for bit, and selects the same rows."""
    from openseg3d_amd import ops
    n, c = 2049, 22
    x, y = size_inputs(n, c)
    kwargs = dict(ignore_index=255, keep_ratio=0.3, class_weight=size_weights(c))
    base = run(ops.cross_entropy_select, x, y, device=dev, **kwargs)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    moved = run(ops.cross_entropy_select, x[perm], y[perm], device=dev, **kwargs)
    assert np.array_equal(moved[1], base[1][perm.numpy()])
    assert abs(moved[0] - base[0]) <= 2e-6 * abs(base[0])


def test_bit_reproducible(dev):
    """Integer atomics only: two calls on the same inputs give the same bits -- loss, counted rows and gradient."""
    from openseg3d_amd import ops
    n, c = 70001, 22
    x, y = size_inputs(n, c)
    xg, yg = x.to(dev), y.to(dev)
    w = torch.tensor(size_weights(c), device=dev)
    for kwargs in (dict(keep_ratio=0.3, class_weight=w), dict(keep_ratio=0.3), dict(weighted_mean=True, class_weight=w),
                   dict(keep_thresh=0.7, class_weight=w)):
        runs = []
        for _ in range(2):
            xx = xg.clone().requires_grad_(True)
            loss = ops.cross_entropy_select(xx, yg, ignore_index=255, **kwargs)
            (loss * UPSTREAM).backward()
            runs.append((loss.detach().clone(), xx.grad))
        assert bool(torch.isfinite(runs[0][0])) and bool(torch.isfinite(runs[0][1]).all())
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), kwargs
    a = raw_forward(xg, yg, RATIO, class_weight=w, keep_ratio=0.3)
    b = raw_forward(xg, yg, RATIO, class_weight=w, keep_ratio=0.3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_one_library_call_each_way_and_no_read_back(dev, monkeypatch):
    from openseg3d_amd import _lib, losses
    names, reads, call = [], [], _lib.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    def reading(what, fn):
        def wrapped(self, *args, **kwargs):
            reads.append(what)
            return fn(self, *args, **kwargs)
        return wrapped

    x, y = size_inputs(2049, 22)
    xg, yg = x.to(dev), y.to(dev)
    w = size_weights(22)
    modules = (losses.OHEMCrossEntropyLoss(keep_ratio=0.3), losses.OHEMCrossEntropyLoss(keep_ratio=0.3, class_weight=w),
               losses.OHEMCrossEntropyLoss(keep_thresh=0.7, class_weight=w), losses.OHEMCrossEntropyLoss(class_weight=w),
               losses.CrossEntropyLoss(class_weight=w))
    for fn in modules:
        fn(xg, yg)  # the class weights are uploaded once per device, on first use
    monkeypatch.setattr(_lib, "call", recording)
    for what in ("item", "tolist", "cpu", "numpy", "__bool__", "__float__", "__int__"):
        monkeypatch.setattr(torch.Tensor, what, reading(what, getattr(torch.Tensor, what)))
    for fn in modules:
        xx = xg.clone().requires_grad_(True)
        loss = fn(xx, yg)
        assert names == ["seg3d_ce_select_fwd"], names
        (loss * UPSTREAM).backward()
        assert names == ["seg3d_ce_select_fwd", "seg3d_ce_select_bwd"], names
        names.clear()
    assert reads == []


def test_unchanged_path_keeps_its_bits(dev):
    """ops.cross_entropy without the new options, and the modules that use it, still are seg3d_cross_entropy_fwd."""
    from openseg3d_amd import _lib, losses, ops
    x, y = size_inputs(70001, 22)
    xg, yg = x.to(dev), y.to(dev)
    n, c = xg.shape
    for keep_thresh, fn in ((0.0, losses.CrossEntropyLoss()), (0.7, losses.OHEMCrossEntropyLoss(keep_thresh=0.7))):
        lse = torch.empty((n,), dtype=torch.float32, device=dev)
        stats = torch.empty((2,), dtype=torch.float32, device=dev)
        ws_bytes = _lib.query("seg3d_cross_entropy_workspace_bytes", n)
        ws = ops._workspace(ws_bytes, dev)
        _lib.call("seg3d_cross_entropy_fwd", ops._ptr(xg), ops._ptr(yg), n, c, 255, keep_thresh, ops._ptr(lse),
                  ops._ptr(stats), ops._ptr(ws), ws_bytes, ops._stream())
        direct = stats[0].clone()
        assert torch.equal(ops.cross_entropy(xg, yg, ignore_index=255, keep_thresh=keep_thresh or None), direct)
        assert torch.equal(fn(xg, yg), direct)


def test_compute_loss_through_the_model(dev):
    """tools/train.py:71-110 with MODEL.LOSSES = {weighted_ce, ohem_ce_ratio, lovasz} and class weights on a small Segformer
    batch: a finite loss, a finite gradient on every parameter, and the float32 sum of the terms taken one by one."""
    from openseg3d_amd import batch as B, config, losses, ops, scene, segformer
    cfg = config.default_cfg()
    cfg.MODEL.LOSSES = {"weighted_ce": 1.0, "ohem_ce_ratio": 1.0, "lovasz": 1.0}
    cfg.DATASET.CLASS_WEIGHT = [1.16 + 0.5 * j for j in range(22)]
    ds = config.DatasetSpec(cfg)
    torch.manual_seed(0)
    model = segformer.build_segmentor(cfg, ds).to(dev).train()
    crit = losses.build_criterion(cfg, ds)
    assert [type(f).__name__ for f, _ in crit] == ["CrossEntropyLoss", "OHEMCrossEntropyLoss", "LovaszLoss"]
    assert losses._fused_terms(crit) is None
    pts = scene.make_small_scene(3, 6000, extent=12.0)
    b = B.make_batch([pts], ds.voxel_size, ds.point_cloud_range)
    n = b["points"].shape[0]
    point_labels = (torch.arange(n, device=dev) * 7 % 23).long()
    point_labels[point_labels == 22] = 255
    b["point_labels"] = point_labels
    b["voxel_labels"] = ops.prepare_voxel_labels(b["point_voxel_ids"], point_labels.to(torch.uint8),
                                                 b["voxel_coords"].shape[0], ignore_index=255).long()
    res = model(b)
    loss = losses.compute_loss(res, b, crit, cfg)
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0.0
    assert not [k for k, p in model.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    aux_gt = ops.aux_voxel_labels(res["voxel_coords"], res["aux_voxel_coords"], b["voxel_labels"], 1, cfg.DATASET.VOXEL_SIZE,
                                  cfg.DATASET.POINT_CLOUD_RANGE)
    with torch.no_grad():
        want = 0
        for fn, w in crit:
            want = want + fn(res["point_out"], point_labels) * w
        for fn, w in crit:
            want = want + fn(res["voxel_out"], b["voxel_labels"]) * w
        for fn, w in crit:
            want = want + cfg.MODEL.AUX_LOSS_WEIGHT * fn(res["aux_voxel_out"], aux_gt) * w
        # the two new terms against their float64 composition on the same logits
        for fn in (crit[0][0], crit[1][0]):
            o, t = res["point_out"].detach(), point_labels
            ref = float(fn(o.double().cpu(), t.cpu()))
            assert abs(float(fn(o, t)) - ref) <= 1e-5 * abs(ref), (type(fn).__name__, float(fn(o, t)), ref)
    assert torch.equal(want, loss.detach())
