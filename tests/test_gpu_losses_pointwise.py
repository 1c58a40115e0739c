"""FocalLoss and DiceLoss on the device (seg3d_focal_loss_fwd/bwd, seg3d_dice_loss_fwd/bwd in csrc/loss_pointwise.hip) against
the reference modules' float64 results (tests/golden/losses_pointwise.npz, make_golden_losses_pointwise.py) and against the
modules' own float64 torch composition (test_losses_pointwise_host.py holds that to the reference at 1e-12).

Bar, everywhere a value or a gradient is compared: the larger of
  * the sibling losses' bars (test_gpu_losses.py): 2e-6 relative on the value, 1e-9 + 1e-5 max|grad| on the gradient;
  * twice the deviation of a float32 run of the same formulas in torch from the float64 result on the same inputs (stored
    in the fixture for its cases, computed here on the CPU for the size sweep).
A fixed-order float32 kernel sits at the float32 error of the formulas; the factor 2 covers another summation order."""
import os

import numpy as np
import pytest
import torch

from test_losses_pointwise_host import CASES, make_case

pytestmark = pytest.mark.gpu

UPSTREAM = 0.4


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "losses_pointwise.npz")))


def run(fn, x, y, dtype=None, device=None, **kwargs):
    """(value, gradient) as float64 numpy, upstream gradient 0.4."""
    xx = x.detach().clone().to(dtype=dtype, device=device).requires_grad_(True)
    loss = fn(xx, y.to(device=device), **kwargs)
    (loss * UPSTREAM).backward()
    return float(loss.detach()), xx.grad.detach().double().cpu().numpy()


def check(got, ref, fp32_val_err, fp32_grad_err, what):
    val_bar = max(2e-6 * abs(ref[0]), 2.0 * fp32_val_err)
    grad_bar = max(1e-9 + 1e-5 * np.abs(ref[1]).max(initial=0.0), 2.0 * fp32_grad_err)
    val_err = abs(got[0] - ref[0])
    grad_err = np.abs(got[1] - ref[1]).max(initial=0.0)
    print(f"{what}: value err {val_err:.3e} (bar {val_bar:.3e})  grad err {grad_err:.3e} (bar {grad_bar:.3e})")
    assert val_err <= val_bar, (what, got[0], ref[0], val_err, val_bar)
    assert grad_err <= grad_bar, (what, grad_err, grad_bar)


@pytest.mark.parametrize("name", CASES)
def test_matches_reference_modules(dev, golden, name):
    fn, kwargs = make_case(name, golden["class_weight"].tolist())
    x, y = torch.from_numpy(golden["logits"]), torch.from_numpy(golden["labels"])
    got = run(fn, x, y, device=dev, **kwargs)
    ref = (float(golden[name]), golden[name + "_grad"] * UPSTREAM)
    check(got, ref, float(golden[name + "_fp32_val_err"]), float(golden[name + "_fp32_grad_err"]) * UPSTREAM, name)


def size_inputs(n, c):
    g = torch.Generator().manual_seed(1000 * n + c)
    x = torch.randn(n, c, generator=g) * 2.5
    y = torch.randint(0, c, (n,), generator=g)
    if n > 1:
        y[1::5] = 255
    return x, y


def size_modules(c):
    from openseg3d_amd import losses
    w = (0.5 + torch.rand(c, generator=torch.Generator().manual_seed(c))).tolist()
    return {"focal": (losses.FocalLoss(), {}),
            "focal_gamma1.5_weighted_sum": (losses.FocalLoss(gamma=1.5, alpha=0.25, class_weight=w, reduction="sum"), {}),
            "dice": (losses.DiceLoss(), {}),
            "dice_exp3_weighted": (losses.DiceLoss(exponent=3, smooth=0.5, class_weight=w, loss_weight=0.7), {"avg_factor": 3.0})}


@pytest.fixture(scope="module")
def size_refs():
    """(n, c, case) -> (float64 composition result, float32 composition's deviation from it), computed once on the CPU."""
    refs = {}
    for n in (1, 63, 64, 65, 257, 2049):
        for c in (1, 3, 22, 64):
            x, y = size_inputs(n, c)
            for case, (fn, kwargs) in size_modules(c).items():
                r64 = run(fn, x, y, dtype=torch.float64, **kwargs)
                r32 = run(fn, x, y, dtype=torch.float32, **kwargs)
                refs[n, c, case] = (r64, abs(r32[0] - r64[0]), np.abs(r32[1] - r64[1]).max())
    return refs


@pytest.mark.parametrize("c", [1, 3, 22, 64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2049])
def test_sizes_match_float64_composition(dev, size_refs, n, c):
    """One wave, the wave edge, a workgroup edge (dice: 128 rows; focal: 256 elements), more than one partial; one class,
    an odd width, the headline width and the widest the kernels take."""
    x, y = size_inputs(n, c)
    for case, (fn, kwargs) in size_modules(c).items():
        got = run(fn, x, y, device=dev, **kwargs)
        if n == 0:  # the mean over nothing: 0 on the device (NaN in torch), and an empty gradient
            assert got[0] == 0.0 and got[1].shape == (0, c), (case, got)
            continue
        ref, fp32_val_err, fp32_grad_err = size_refs[n, c, case]
        check(got, ref, fp32_val_err, fp32_grad_err, f"{case} n={n} c={c}")


def test_focal_properties(dev):
    from openseg3d_amd import losses, ops
    n, c = 700, 22
    x, y = size_inputs(n, c)
    xg, yg = x.to(dev), y.to(dev)
    fn = losses.FocalLoss()
    base = run(fn, x, y, device=dev)
    # rows with the ignore label: exactly 0
    assert np.abs(base[1][(y == 255).numpy()]).max() == 0.0 and np.abs(base[1][(y != 255).numpy()]).min() > 0.0
    # all rows ignored: loss 0, gradient 0 (mean and sum)
    for red in ("mean", "sum"):
        val, grad = run(losses.FocalLoss(reduction=red), x, torch.full((n,), 255), device=dev)
        assert val == 0.0 and np.abs(grad).max() == 0.0
    # labels outside [0, c) that are not the ignore label are skipped like it, and not counted
    y_out = y.clone()
    y_out[y == 255] = torch.tensor([-1, c, 300, -7])[torch.arange(int((y == 255).sum())) % 4]
    out = run(fn, x, y_out, device=dev)
    assert out[0] == base[0] and np.array_equal(out[1], base[1])
    # a row permutation permutes the gradient and moves the loss by no more than the summation order can
    ref64 = run(fn, x, y, dtype=torch.float64)
    ref32 = run(fn, x, y, dtype=torch.float32)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    moved = run(fn, x[perm], y[perm], device=dev)
    check((moved[0], moved[1]), (ref64[0], ref64[1][perm.numpy()]), abs(ref32[0] - ref64[0]),
          np.abs(ref32[1] - ref64[1]).max(), "focal permuted")
    assert np.array_equal(moved[1], base[1][perm.numpy()])  # per element, nothing depends on the row's position
    with pytest.raises(ValueError):
        ops.focal_loss(xg, yg, reduction="none")
    with pytest.raises(ValueError):
        ops.focal_loss(torch.zeros(4, 65, device=dev), yg[:4])


def test_dice_properties(dev):
    from openseg3d_amd import losses
    n, c = 700, 22
    x, y = size_inputs(n, c)
    fn = losses.DiceLoss()
    base = run(fn, x, y, device=dev)
    ref64 = run(fn, x, y, dtype=torch.float64)
    ref32 = run(fn, x, y, dtype=torch.float32)
    fp32_val_err, fp32_grad_err = abs(ref32[0] - ref64[0]), np.abs(ref32[1] - ref64[1]).max()
    # ignored rows carry the composition's gradient (through the denominator), not 0
    ignored = (y == 255).numpy()
    assert np.abs(ref64[1][ignored]).max(axis=1).min() > 0.0
    check((base[0], base[1][ignored]), (ref64[0], ref64[1][ignored]), fp32_val_err, fp32_grad_err, "dice ignored rows")
    assert np.abs(base[1][ignored]).max(axis=1).min() > 0.0
    # every row's logit gradient sums to 0 (softmax)
    assert np.abs(base[1].sum(axis=1)).max() <= 1e-9
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    moved = run(fn, x[perm], y[perm], device=dev)
    check(moved, (ref64[0], ref64[1][perm.numpy()]), fp32_val_err, fp32_grad_err, "dice permuted")
    assert np.array_equal(moved[1], base[1][perm.numpy()])  # a row's gradient does not depend on its position
    # labels outside [0, c) are clamped into it (dice_loss.py:99-101), as in the composition
    y_out = y.clone()
    y_out[::9] = 300
    y_out[4::9] = -3
    check(run(fn, x, y_out, device=dev), run(fn, x, y_out, dtype=torch.float64), fp32_val_err, fp32_grad_err, "dice clamped")
    # ignore_index inside [0, c): that class is left out of the sum, its rows out of the numerator
    fn3 = losses.DiceLoss(ignore_index=3)
    check(run(fn3, x, y, device=dev), run(fn3, x, y, dtype=torch.float64), fp32_val_err, fp32_grad_err, "dice ignore 3")
    with pytest.raises(ValueError):
        fn(x.to(dev), y.to(dev), avg_factor=2.0, reduction_override="sum")


@pytest.mark.parametrize("n", [2049, 174633])
def test_bit_reproducible(dev, n):
    """No floating-point atomics: two calls on the same inputs give the same bits, loss and gradient."""
    from openseg3d_amd import losses
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, 22, generator=g) * 2.5).to(dev)
    y = torch.randint(0, 22, (n,), generator=g)
    y[torch.rand(n, generator=g) < 0.1] = 255
    y = y.to(dev)
    for fn in (losses.FocalLoss(), losses.FocalLoss(gamma=1.5, reduction="sum"), losses.DiceLoss(), losses.DiceLoss(exponent=3)):
        runs = []
        for _ in range(2):
            xx = x.clone().requires_grad_(True)
            loss = fn(xx, y)
            (loss * UPSTREAM).backward()
            runs.append((loss.detach().clone(), xx.grad))
        assert bool(torch.isfinite(runs[0][0])) and bool(torch.isfinite(runs[0][1]).all())
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), type(fn).__name__


def test_one_library_call_each_way(dev, monkeypatch):
    """Each loss is one library call forward (the pass over the logits and the fixed-order finalize of its partials: the
    two launches of seg3d_*_loss_fwd) and one backward (a single launch), recorded as test_gpu_encoder_layer.py records
    them; the workspace query launches nothing."""
    from openseg3d_amd import _lib, losses
    names, call = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    monkeypatch.setattr(_lib, "call", recording)
    x, y = size_inputs(2049, 22)
    for fn, stem in ((losses.FocalLoss(), "seg3d_focal_loss"), (losses.DiceLoss(), "seg3d_dice_loss")):
        xx = x.to(dev).requires_grad_(True)
        loss = fn(xx, y.to(dev))
        assert names == [stem + "_fwd"], names
        (loss * UPSTREAM).backward()
        assert names == [stem + "_fwd", stem + "_bwd"], names
        names.clear()


def test_compute_loss_with_focal_and_dice_through_the_model(dev):
    """tools/train.py:71-110 with MODEL.LOSSES = {ohem_ce, focal, dice} on a small Segformer batch: finite loss, finite
    gradient on every parameter, and the same bits from the same state and seed."""
    from openseg3d_amd import batch as B, config, losses, ops, scene, segformer
    cfg = config.default_cfg()
    cfg.MODEL.LOSSES = {"ohem_ce": 1.0, "focal": 1.0, "dice": 1.0}
    ds = config.DatasetSpec(cfg)
    torch.manual_seed(0)
    model = segformer.build_segmentor(cfg, ds).to(dev).train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    crit = losses.build_criterion(cfg, ds)
    assert [type(f).__name__ for f, _ in crit] == ["OHEMCrossEntropyLoss", "FocalLoss", "DiceLoss"]
    pts = scene.make_small_scene(3, 6000, extent=12.0)
    runs = []
    for _ in range(2):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(123)
        b = B.make_batch([pts], ds.voxel_size, ds.point_cloud_range)
        n = b["points"].shape[0]
        point_labels = (torch.arange(n, device=dev) * 7 % 23).long()
        point_labels[point_labels == 22] = 255
        b["point_labels"] = point_labels
        b["voxel_labels"] = ops.prepare_voxel_labels(b["point_voxel_ids"], point_labels.to(torch.uint8),
                                                     b["voxel_coords"].shape[0], ignore_index=255).long()
        loss = losses.compute_loss(model(b), b, crit, cfg)
        loss.backward()
        runs.append((loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert bool(torch.isfinite(runs[0][0])) and float(runs[0][0]) > 0.0
    assert not [k for k, g in runs[0][1].items() if not bool(torch.isfinite(g).all())]
    assert torch.equal(runs[0][0], runs[1][0])
    assert not [k for k in runs[0][1] if not torch.equal(runs[0][1][k], runs[1][1][k])]
