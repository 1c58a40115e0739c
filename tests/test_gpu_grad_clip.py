"""Gradient-norm clipping on the GPU: seg3d_grad_norm / seg3d_grad_scale through optim.GradClipper against the exact norm
(tests/grad_clip_ref.py: within 1 float32 ulp; coefficient and scaled gradients bit for bit) at every size where the
kernels take another path, the sync-free steady state, and a clipped training step of the model."""
import pytest
import torch

import grad_clip_ref as G
from openseg3d_amd import _lib, optim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def block():
    return int(_lib.load().seg3d_optim_block_elems())


@pytest.mark.parametrize("pattern", G.PATTERNS_FINITE)
def test_norm_coefficient_and_scale(dev, pattern):
    G.check_finite_pattern(block(), dev, pattern, G.reference(block(), pattern))


def test_zero_gradients(dev):
    G.check_zeros(block(), dev)


@pytest.mark.parametrize("pattern", ["inf", "nan"])
def test_nonfinite_gradients_follow_torch(dev, pattern):
    G.check_nonfinite(block(), dev, pattern)


def test_scale_agrees_with_the_host_twin(dev):
    """The same gradients clipped on both sides with the same max_norm: norms within the ulp both are allowed, and where the
    two coefficients agree (they are functions of the norm written) the gradients do, bit for bit."""
    b = block()
    grads = G.values(b, "noise")
    gpu, cpu = G.Case(b, dev, grads), G.Case(b, torch.device("cpu"), grads)
    m = float(G.reference(b, "noise")) / 3
    cg, cc = optim.GradClipper(gpu.params, m), optim.GradClipper(cpu.params, m)
    ng, nc = cg(), cc()
    assert G.ulps(ng.cpu(), G.reference(b, "noise")) <= 1.0 and G.ulps(nc, G.reference(b, "noise")) <= 1.0
    if G.same_bits(ng, nc):
        assert G.same_bits(cg.last_coef, cc.last_coef)
        assert all(G.same_bits(x, y) for x, y in zip(gpu.grads(), cpu.grads()))


def record_calls(monkeypatch):
    names, call = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    monkeypatch.setattr(_lib, "call", recording)
    return names


def test_steady_state_is_two_calls_and_no_sync(dev, monkeypatch):
    """Calls two and three of a GradClipper: the two library calls, nothing that synchronises, the table of call one; after
    zero_grad(set_to_none=True) and gradients at other addresses the table is rebuilt and the result still right."""
    b = block()
    case = G.Case(b, dev, G.values(b, "noise"))
    ref = G.reference(b, "noise")
    clipper = optim.GradClipper(case.params, float(ref) / 2)
    first = clipper()
    names = record_calls(monkeypatch)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        table = clipper._plan.table
        norms = []
        for _ in range(2):
            before = len(names)
            norms.append(clipper())
            assert names[before:] == ["seg3d_grad_norm", "seg3d_grad_scale"]
            assert clipper._plan.table is table
        old = [p.grad for p in case.params] + [case.buf]  # kept alive: the new gradients get other addresses
        for p in case.params:
            p.grad = None
        case.set_grads()
        assert case.params[0].grad.data_ptr() != old[0].data_ptr()
        before = len(names)
        rebuilt = clipper()
        assert names[before:] == ["seg3d_grad_norm", "seg3d_grad_scale"]
        assert clipper._plan.table is not table
        coef = clipper.last_coef
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert G.ulps(first.cpu(), ref) <= 1.0 and G.same_bits(rebuilt, first)
    assert float(norms[1]) <= float(norms[0]) < float(first)  # each call saw what the one before had left
    assert all(G.same_bits(a, g * coef.cpu()) for a, g in zip(case.grads(), case.start))
    assert case.view_surroundings_untouched()
    del old


def test_clip_under_stream_capture_is_refused(dev):
    p = torch.ones(100, device=dev, requires_grad=True)
    p.grad = torch.ones(100, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            with pytest.raises(NotImplementedError, match="capture"):
                optim.clip_grad_norm_([p], 1.0)
        finally:
            graph.capture_end()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(p.grad.cpu(), torch.ones(100))


def test_two_devices_are_refused_by_name(dev):
    p = torch.ones(4, device=dev, requires_grad=True)
    p.grad = torch.ones(4, device=dev)
    q = torch.ones(4, requires_grad=True)
    q.grad = torch.ones(4)
    with pytest.raises(NotImplementedError, match="one device.*cuda:0.*cpu"):
        optim.clip_grad_norm_([p, q], 1.0)


def test_clipped_training_step_of_the_model(dev):
    """The small training case of tests/test_gpu_optim.py: after loss.backward() -- whose weight gradients are written on a
    side stream and joined when the pass ends -- opt.clip_grad_norm_(half the norm) returns the exact norm of the gradients
    as they were (1 ulp), leaves m * norm / (norm + 1e-6) (4 ulp: one rounding of the coefficient, one per element
    product, one for each of the two norms), and opt.step() then moves the parameters."""
    from openseg3d_amd import batch as B, config, scene, segformer
    torch.manual_seed(0)
    cfg = config.default_cfg()
    cfg.TRAIN.OPTIMIZER = "adamw"
    ds = config.DatasetSpec(cfg)
    model = segformer.build_segmentor(cfg, ds).to(dev).train()
    opt = optim.build_optimizer(cfg, model)
    samples = [scene.make_small_scene(7, 6000, extent=9.0), scene.make_small_scene(8, 4000, extent=6.0)]
    ce = torch.nn.functional.cross_entropy
    b = B.make_batch(samples, ds.voxel_size, ds.point_cloud_range)
    labels = torch.arange(b["points"].shape[0], device=dev) % 22
    opt.zero_grad(set_to_none=True)
    res = model(b)
    loss = (ce(res["point_out"], labels) + ce(res["voxel_out"], labels[:1].expand(res["voxel_out"].shape[0]))
            + 0.4 * ce(res["aux_voxel_out"], labels[:1].expand(res["aux_voxel_out"].shape[0])))
    loss.backward()
    params = [p for p in model.parameters() if p.grad is not None]
    assert len(params) > 100
    before = [p.grad.detach().clone() for p in params]
    ref = G.exact_norm(before)
    m = float(ref) / 2
    norm = opt.clip_grad_norm_(m)
    err = G.ulps(norm.cpu(), ref)
    print(f"model: norm {float(norm)!r}, exact {float(ref)!r}, {err} ulp")
    assert float(ref) > 0 and err <= 1.0, (float(norm), float(ref), err)
    coef = opt._clipper.last_coef
    assert all(G.same_bits(p.grad, g * coef) for p, g in zip(params, before))
    after = optim.grad_norm(model.parameters())
    want = m * float(norm) / (float(norm) + 1e-6)
    err = G.ulps(after.cpu(), want)
    print(f"model: norm after the clip {float(after)!r}, expected {want!r}, {err} ulp")
    assert err <= 4.0, (float(after), want, err)
    start = [p.detach().clone() for p in params]
    opt.step()
    assert all(torch.isfinite(p).all() for p in params)
    assert sum(not torch.equal(p.detach(), s) for p, s in zip(params, start)) > len(params) // 2
