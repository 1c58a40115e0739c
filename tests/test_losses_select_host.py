"""Class-weighted cross-entropy and OHEM by keep_ratio without a GPU: the modules' torch composition (the branch every CPU /
float64 input takes) against the reference's float64 results in tests/golden/losses_select.npz
(make_golden_losses_select.py), the two new build_criterion keys, keep_ratio's precedence, the rule for equal losses at
the cut, and the argument checks of seg3d_ce_select_fwd / _bwd (they return before anything is enqueued)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from openseg3d_amd import losses

C = 22
CASES = ["ohem_none", "ohem_thresh", "ohem_ratio", "ohem_weighted_none", "ohem_weighted_thresh", "ohem_weighted_ratio",
         "ce_weighted"]


def make_case(name, weights, keep_thresh=0.7, keep_ratio=0.3):
    """name -> module, the cases of make_golden_losses_select.cases."""
    w = weights if "weighted" in name else None
    if name == "ce_weighted":
        return losses.CrossEntropyLoss(ignore_index=255, class_weight=w)
    return losses.OHEMCrossEntropyLoss(keep_thresh=keep_thresh if name.endswith("thresh") else None,
                                       keep_ratio=keep_ratio if name.endswith("ratio") else None, class_weight=w)


def select_kwargs(name, weights, keep_thresh=0.7, keep_ratio=0.3):
    """name -> keyword arguments of ops.cross_entropy_select for the same case."""
    return dict(ignore_index=255, class_weight=weights if "weighted" in name else None,
                keep_thresh=keep_thresh if name.endswith("thresh") else None,
                keep_ratio=keep_ratio if name.endswith("ratio") else None, weighted_mean=name == "ce_weighted")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "losses_select.npz")))


@pytest.mark.parametrize("name", CASES)
def test_composition_matches_reference_fp64(golden, name):
    """Value and input gradient of the float64 fallback within 1e-12 relative of the reference's.  Without class weights
    and without keep_ratio the module has no torch branch (it calls ops.cross_entropy, as before): those two cases reach
    the composition's plain-mean and keep_thresh lines with weights of exactly 1."""
    fn = make_case(name, golden["class_weight"].tolist(), float(golden["keep_thresh"]), float(golden["keep_ratio"]))
    if name in ("ohem_none", "ohem_thresh"):
        fn.class_weight = [1.0] * C
    x = torch.from_numpy(golden["logits"]).double().requires_grad_(True)
    loss = fn(x, torch.from_numpy(golden["labels"]))
    loss.backward()
    assert loss.dtype == torch.float64 and loss.dim() == 0
    ref, ref_grad = float(golden[name]), golden[name + "_grad"]
    assert abs(float(loss.detach()) - ref) <= 1e-12 * abs(ref), (float(loss.detach()), ref)
    err = np.abs(x.grad.numpy() - ref_grad).max()
    assert err <= 1e-12 * np.abs(ref_grad).max(), err


def test_fixture_inputs(golden):
    x, y, w = golden["logits"], golden["labels"], golden["class_weight"]
    assert x.shape == (257, C) and x.dtype == np.float32 and y.dtype == np.int64
    assert (y[::7] == 255).all() and (y == 255).sum() == len(y[::7])
    assert w.shape == (C,) and w.min() >= 1.0 and w.max() <= 11.5 and w.max() / w.min() > 4
    n_valid = int((y != 255).sum())
    for name in ("ohem_ratio", "ohem_weighted_ratio"):
        assert int(golden[name + "_kept"]) == int(n_valid * float(golden["keep_ratio"])) == 66
        assert int(golden[name + "_grad"].any(axis=1).sum()) == 66 and float(golden[name + "_gap"]) > 1e-4
    # the selectors select: the three unweighted values differ, and the hardest 30 % average far above the mean
    assert float(golden["ohem_ratio"]) > float(golden["ohem_thresh"]) > float(golden["ohem_none"])
    for name in CASES:
        assert float(golden[name + "_fp32_val_err"]) < 1e-6 * abs(float(golden[name]))
        assert float(golden[name + "_fp32_grad_err"]) < 1e-5 * np.abs(golden[name + "_grad"]).max()


def test_class_surface(tmp_path, golden):
    assert losses.CrossEntropyLoss().class_weight is None and losses.CrossEntropyLoss().ignore_index == 255
    assert losses.CrossEntropyLoss(loss_name="loss_a").loss_name == "loss_a"
    assert losses.CrossEntropyLoss(class_weight=[1.0, 2.0]).loss_name == "loss_cross_entropy"
    w = golden["class_weight"]
    path = str(tmp_path / "w.npy")
    np.save(path, w)
    x, y = torch.from_numpy(golden["logits"]).double(), torch.from_numpy(golden["labels"])
    for cls in (losses.CrossEntropyLoss, losses.OHEMCrossEntropyLoss):
        a, b = cls(class_weight=w.tolist()), cls(class_weight=path)  # through get_class_weight, like Focal and Dice
        assert np.array_equal(np.asarray(b.class_weight), w)
        assert float(a(x, y)) == float(b(x, y))
        with pytest.raises(ValueError):
            cls(class_weight="weights.txt")
    # a tensor, what the reference's module is given, still works
    t = losses.OHEMCrossEntropyLoss(class_weight=torch.from_numpy(w), keep_ratio=0.3)
    assert float(t(x, y)) == float(losses.OHEMCrossEntropyLoss(class_weight=w.tolist(), keep_ratio=0.3)(x, y))


def test_build_criterion_keys():
    from openseg3d_amd import config
    cfg = config.default_cfg()
    ds = config.DatasetSpec(cfg)
    weights = [1.0 + 0.5 * i for i in range(C)]
    cfg.DATASET.CLASS_WEIGHT = weights
    cfg.MODEL.LOSSES = {"weighted_ce": 1.0, "ohem_ce_ratio": 0.5, "lovasz": 1.0}
    crit = losses.build_criterion(cfg, ds)
    assert [(type(f).__name__, w) for f, w in crit] == [("CrossEntropyLoss", 1.0), ("OHEMCrossEntropyLoss", 0.5),
                                                        ("LovaszLoss", 1.0)]
    ce, ohem = crit[0][0], crit[1][0]
    assert list(ce.class_weight) == weights and ce.ignore_index == ds.ignore_index == 255
    assert ohem.keep_ratio == cfg.MODEL.OHEM_KEEP_RATIO == 0.3 and ohem.keep_thresh is None and ohem.class_weight is None
    assert ohem.ignore_index == 255
    assert losses._fused_terms(crit) is None  # these run in compute_loss's per-term loop
    assert losses._fused_terms(crit[:1]) is None and losses._fused_terms(crit[1:]) is None
    cfg.DATASET.CLASS_WEIGHT = []  # the default: no weights
    assert losses.build_criterion(cfg, ds)[0][0].class_weight is None
    cfg.MODEL.LOSSES = {"ohem_ce": 1.0, "lovasz": 1.0}  # the default criterion is what it was, and still fuses
    crit = losses.build_criterion(cfg, ds)
    assert [type(f).__name__ for f, _ in crit] == ["OHEMCrossEntropyLoss", "LovaszLoss"]
    assert crit[0][0].keep_ratio is None and crit[0][0].keep_thresh == 0.7
    assert losses._fused_terms(crit) == (255, 0.7, 1.0, 1.0)


def test_keep_ratio_wins_over_keep_thresh(golden):
    x, y = torch.from_numpy(golden["logits"]).double(), torch.from_numpy(golden["labels"])
    both = losses.OHEMCrossEntropyLoss(keep_ratio=0.3, keep_thresh=0.7)(x, y)
    assert float(both) == pytest.approx(float(golden["ohem_ratio"]), rel=1e-12)
    assert float(both) != pytest.approx(float(golden["ohem_thresh"]), rel=1e-3)
    # keep_ratio 0 / None is no selector (the reference tests truth): keep_thresh applies
    ones = [1.0] * C  # with weights the module takes its torch branch on the CPU
    assert float(losses.OHEMCrossEntropyLoss(keep_ratio=0, keep_thresh=0.7, class_weight=ones)(x, y)) == pytest.approx(
        float(golden["ohem_thresh"]), rel=1e-12)


def test_equal_losses_are_kept_in_row_order():
    """7 distinct rows, each 6 times: 42 valid rows, keep_ratio 0.5 keeps 21 = the 3 hardest groups and half of the fourth,
    and of that group the 3 copies with the lowest row indices (torch.sort(descending=True, stable=True))."""
    g = torch.Generator().manual_seed(5)
    base = torch.randn(7, 5, generator=g, dtype=torch.float64) * 2
    x = base.repeat(6, 1).requires_grad_(True)  # row r is base[r % 7]
    y = (torch.arange(42) % 7) % 5
    per_group = torch.nn.functional.cross_entropy(base, y[:7], reduction="none")
    assert len(set(per_group.tolist())) == 7
    order = per_group.argsort(descending=True)
    loss = losses.OHEMCrossEntropyLoss(keep_ratio=0.5)(x, y)
    loss.backward()
    kept = x.grad.abs().sum(dim=1) > 0
    want = torch.zeros(42, dtype=torch.bool)
    for grp in order[:3].tolist():
        want[grp::7] = True
    want[int(order[3])::7][:3] = True
    assert int(kept.sum()) == 21 and torch.equal(kept, want)
    mean = float((per_group[order[:3]].sum() * 6 + per_group[order[3]] * 3) / 21)
    assert float(loss.detach()) == pytest.approx(mean, rel=1e-14)


def test_nan_loss_ranks_first():
    x = torch.zeros(6, 3, dtype=torch.float64)
    x[4, 0] = float("nan")
    x[2, 1] = -5.0
    y = torch.tensor([0, 0, 1, 0, 0, 255])
    xx = x.clone().requires_grad_(True)
    loss = losses.OHEMCrossEntropyLoss(keep_ratio=0.4)(xx, y)  # int(5 * 0.4) = 2: the NaN row, then row 2
    assert bool(torch.isnan(loss))
    loss.backward()
    assert [i for i in range(6) if bool((xx.grad[i] != 0).any())] == [2, 4]


def test_device_op_rejects_other_inputs():
    from openseg3d_amd import ops
    y = torch.zeros(4, dtype=torch.long)
    for x, lab in ((torch.zeros(4, 3), y), (torch.zeros(4, 3, dtype=torch.float64), y), (torch.zeros(4, 3), y.int())):
        with pytest.raises(ValueError):
            ops.cross_entropy_select(x, lab, keep_ratio=0.3)


def _fwd(lib, n=4, c=3, mode=3, keep_thresh=0.0, keep_ratio=0.3, ptr=0x1000, ws_bytes=1 << 30, stats=0x1000, ws=0x1000):
    p = ctypes.c_void_p
    return lib.seg3d_ce_select_fwd(p(ptr), p(ptr), n, c, 255, None, mode, keep_thresh, keep_ratio, p(ptr), p(stats), p(ws),
                                   ws_bytes, None)


def test_entry_points_validate_before_enqueueing():
    """Every refusal below is decided on the host: the pointers are fake and no GPU need be present, so nothing can have
    been launched."""
    from openseg3d_amd import _lib
    lib = _lib.load()
    need = _lib.query("seg3d_ce_select_workspace_bytes", 4)
    assert need > 0 and _lib.query("seg3d_ce_select_workspace_bytes", 0) > 0
    assert _lib.query("seg3d_ce_select_workspace_bytes", 1 << 20) >= 4 << 20  # the keys: 4 bytes a row
    assert _lib.query("seg3d_ce_select_workspace_bytes", -1) == 0
    assert _lib.query("seg3d_ce_select_workspace_bytes", 1 << 31) == 0
    for bad in (dict(n=-1), dict(n=1 << 31), dict(c=0), dict(c=4097), dict(mode=-1), dict(mode=4), dict(stats=None),
                dict(ws=None), dict(ws_bytes=need - 1), dict(ptr=None), dict(keep_ratio=0.0), dict(keep_ratio=-0.5),
                dict(keep_ratio=float("nan")), dict(mode=2, keep_thresh=0.0), dict(mode=2, keep_thresh=float("nan"))):
        assert _fwd(lib, **bad) == _lib.EINVAL, bad
    p = ctypes.c_void_p
    fake = p(0x1000)

    def bwd(n=4, c=3, mode=3, x=fake, stats=fake, gout=fake, dx=fake):
        return lib.seg3d_ce_select_bwd(x, x, None, x, stats, gout, n, c, mode, dx, None)

    for bad in (dict(n=-1), dict(n=1 << 31), dict(c=0), dict(c=4097), dict(mode=-1), dict(mode=4), dict(stats=None),
                dict(gout=None), dict(x=None), dict(dx=None)):
        assert bwd(**bad) == _lib.EINVAL, bad
    assert bwd(n=0, x=None, dx=None) == _lib.OK  # nothing to write, nothing launched
