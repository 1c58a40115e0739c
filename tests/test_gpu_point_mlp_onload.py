"""Per-point MLPs in training: BatchNorm1d + ReLU applied on operand load (ops.POINT_BN_ONLOAD).

The change is a bit-exact transformation -- the activated tensor z = max(y * scale + shift, 0) is formed in registers by
the kernels that used to read it, with the multiply, add and max of the separate affine pass -- so every check here is
torch.equal against the composed path, never a tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------- part A
def _bn_bwd_inputs(m, c):
    """x, scale, shift whose pre-activation v = x * scale + shift holds exact +0.0 and -0.0 and values of either sign within
    1 ulp of zero (the smallest subnormal and the smallest normal), next to ordinary values of both signs."""
    g = _gen(1000 + m + c)
    x = torch.randn(m, c, generator=g)
    scale = torch.rand(c, generator=g) + 0.5
    shift = torch.randn(c, generator=g) * 0.3
    # columns 0..3: scale 1, shift +0.0 -> v = x exactly; columns 4..7: scale 1, shift -0.0 -> v = x, and -0.0 stays -0.0
    scale[:8] = 1.0
    shift[:4] = 0.0
    shift[4:8] = -0.0
    tiny = torch.tensor([0.0, -0.0, 1.401298464324817e-45, -1.401298464324817e-45, 1.1754943508222875e-38,
                         -1.1754943508222875e-38, 1.0, -1.0])
    rows = torch.arange(m)
    for col in range(8):
        x[:, col] = tiny[(3 * rows + col) % 8]
    # a column whose affine cancels to zero exactly: x = 2, scale = 0.5, shift = -1 -> v = +0.0
    x[::3, 8] = 2.0
    scale[8], shift[8] = 0.5, -1.0
    v = x * scale + shift
    assert (v == 0).any() and torch.signbit(v[v == 0]).any() and (~torch.signbit(v[v == 0])).any()
    return x, scale, shift


@pytest.mark.parametrize("m,c", [(2, 64), (31, 64), (1237, 128), (4099, 256), (70001, 96)])
def test_batchnorm_backward_from_the_pre_activation_equals_the_one_that_reads_y(m, c):
    from openseg3d_amd import _lib
    from openseg3d_amd.ops import _ptr, _stream, _workspace
    x, scale, shift = _bn_bwd_inputs(m, c)
    g = _gen(7 * m + c)
    dy = torch.randn(m, c, generator=g).to(DEV)
    mean = (torch.randn(c, generator=g) * 0.2).to(DEV)
    rstd = (torch.rand(c, generator=g) + 0.5).to(DEV)
    gamma = (torch.randn(c, generator=g)).to(DEV)
    x, scale, shift = x.to(DEV), scale.to(DEV), shift.to(DEV)
    y = torch.empty_like(x)
    _lib.call("seg3d_affine_act", _ptr(x), None, _ptr(scale), _ptr(shift), 1, m, c, _ptr(y), _stream())
    assert (y == 0).any() and (y > 0).any()
    ws_bytes = _lib.query("seg3d_batchnorm_workspace_bytes", m, c)
    out = []
    for pre in (False, True):
        dx = torch.full_like(x, float("nan"))
        sums = torch.full((2, c), float("nan"), device=DEV)
        ws = _workspace(ws_bytes, DEV)
        if pre:
            _lib.call("seg3d_batchnorm_bwd_pre", _ptr(dy), _ptr(x), _ptr(scale), _ptr(shift), _ptr(mean), _ptr(rstd),
                      _ptr(gamma), m, c, _ptr(dx), _ptr(sums), _ptr(ws), ws_bytes, _stream())
        else:
            _lib.call("seg3d_batchnorm_bwd", _ptr(dy), _ptr(y), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), 1, m, c,
                      _ptr(dx), None, _ptr(sums), _ptr(ws), ws_bytes, _stream())
        out.append((dx, sums[1].clone(), sums[0].clone()))
    torch.cuda.synchronize()
    assert torch.isfinite(out[0][0]).all()
    for name, a, b in zip(("dx", "dgamma", "dbeta"), out[0], out[1]):
        assert torch.equal(a, b), name


# ---------------------------------------------------------------------------------------------------------------- part B-D
def _layer(cin, cout, seed, big_shift):
    g = _gen(seed)
    bn = torch.nn.BatchNorm1d(cin)
    lin = torch.nn.Linear(cin, cout, bias=cout == 64)  # (the point encoder's last Linear, 256 -> 64, has a bias)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(cin, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(cin, generator=g) * 0.3)
        if big_shift:  # a padded row that was not masked would add max(0 * s + t, 0) * dy = 1e6-grade terms to dW
            bn.bias.fill_(1.0e6)
        bn.running_mean.copy_(torch.randn(cin, generator=g))
        bn.running_var.copy_(torch.rand(cin, generator=g) + 0.5)
        lin.weight.copy_(torch.randn(cout, cin, generator=g) / cin ** 0.5)
        if lin.bias is not None:
            lin.bias.copy_(torch.randn(cout, generator=g))
    return bn.to(DEV).train(), lin.to(DEV).train()


@pytest.mark.parametrize("m,cin,cout,big_shift", [
    (31, 64, 128, False),      # only the partial 32-row step of the weight gradient
    (31, 64, 128, True),       # ... with a shift that shows an unmasked padded row
    (333, 128, 256, False),    # row clamp in the six-product kernel (333 = 2 * 128 + 77)
    (1237, 256, 64, False),
    (4099, 256, 128, False),   # several weight-gradient chunks, the last one partial
    (4099, 256, 128, True),
    (70001, 64, 128, False),
])
def test_bn_relu_linear_equals_the_composed_path(m, cin, cout, big_shift):
    from openseg3d_amd import ops
    g = _gen(m + cin + cout)
    x0 = torch.randn(m, cin, generator=g).to(DEV)
    x0[::5, :4] = 0.0
    dy = torch.randn(m, cout, generator=g).to(DEV)
    res = []
    for fused in (False, True):
        bn, lin = _layer(cin, cout, 5 + cin, big_shift)
        x = x0.clone().requires_grad_(True)
        if fused:
            assert ops.bn_relu_linear_fits(x, bn, lin)
            y = ops.bn_relu_linear(x, bn, lin)
        else:
            y = ops.linear(ops.batch_norm_act(x, bn, relu=True), lin.weight, lin.bias, exact=True)
        y.backward(dy)
        torch.cuda.synchronize()
        res.append(dict(y=y.detach(), dx_pre=x.grad, dW=lin.weight.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad,
                        running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                        num_batches_tracked=bn.num_batches_tracked.clone()))
        if lin.bias is not None:
            res[-1]["db"] = lin.bias.grad
    assert int(res[1]["num_batches_tracked"]) == 1
    assert torch.isfinite(res[0]["dW"]).all() and float(res[0]["dW"].abs().max()) > 0
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k


# ---------------------------------------------------------------------------------------------------------------- step
def _segformer_step(monkeypatch, onload, storage="fp32"):
    """(loss, gradients, calls of ops.bn_relu_linear) of one training step on a small two-sample scene, from fixed seeds."""
    from openseg3d_amd import batch as B, config, losses, ops, scene, segformer
    monkeypatch.setattr(ops, "POINT_BN_ONLOAD", onload)
    monkeypatch.setattr(ops, "TRAIN_STORAGE", storage)
    calls = []
    real = getattr(ops.bn_relu_linear, "real", ops.bn_relu_linear)  # (an earlier step of the same test left its counter)

    def counted(x, bn, lin):
        calls.append(tuple(lin.weight.shape))
        return real(x, bn, lin)

    counted.real = real
    monkeypatch.setattr(ops, "bn_relu_linear", counted)
    cfg = config.default_cfg()
    ds = config.DatasetSpec(cfg)
    torch.manual_seed(1)
    model = segformer.build_segmentor(cfg, ds).to(DEV).train()
    crit = losses.build_criterion(cfg, ds)
    samples = [scene.make_small_scene(17, 9000, extent=10.0), scene.make_small_scene(18, 5000, extent=6.0)]
    torch.manual_seed(123)
    b = B.make_batch(samples, ds.voxel_size, ds.point_cloud_range)
    n = b["points"].shape[0]
    b["point_labels"] = (torch.arange(n, device=DEV) * 5 % 22).long()
    b["voxel_labels"] = ops.prepare_voxel_labels(b["point_voxel_ids"], b["point_labels"].to(torch.uint8),
                                                 b["voxel_coords"].shape[0]).long()
    loss = losses.compute_loss(model(b), b, crit, cfg)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    buffers = {k: v.clone() for k, v in model.named_buffers()}
    return loss.detach().clone(), grads, buffers, calls


def test_segformer_step_is_the_same_with_the_switch_off_and_on(monkeypatch):
    off = _segformer_step(monkeypatch, False)
    on = _segformer_step(monkeypatch, True)
    again = _segformer_step(monkeypatch, True)
    assert len(off[3]) == 0
    # point_encoder 64 -> 128 -> 256 -> 64 and fusion_encoder 256 -> 128 -> 64 behind their BatchNorm + ReLU
    assert sorted(tuple(s) for s in on[3]) == sorted([(128, 64), (256, 128), (64, 256), (128, 256), (64, 128)])
    for other in (on, again):
        assert torch.equal(off[0], other[0])
        differing = [k for k in off[1] if not torch.equal(off[1][k], other[1][k])]
        assert not differing, differing[:8]
        differing = [k for k in off[2] if not torch.equal(off[2][k], other[2][k])]
        assert not differing, differing[:8]


def test_bf16_training_copies_keep_the_composed_path(monkeypatch):
    loss, grads, _, calls = _segformer_step(monkeypatch, True, storage="bf16")
    assert len(calls) == 0
    assert torch.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())
