"""openseg3d_amd.optim on the GPU: the multi-tensor kernel (seg3d_optim_step) against its host twin bit for bit at every
size where it takes another path, the sync-free steady state, more hyper-parameter sets than one launch holds, the
weight-pack caches after a step, and three training steps of the model through build_optimizer."""
import numpy as np
import pytest
import torch

import optim_ref as R
from openseg3d_amd import _lib, optim

pytestmark = pytest.mark.gpu

VARIANTS = {
    "sgd_momentum": (optim.SGD, R.SGD_GROUPS),
    "sgd_plain": (optim.SGD, [dict(kw, momentum=0.0) for kw in R.SGD_GROUPS]),
    "adamw": (optim.AdamW, R.ADAMW_GROUPS),
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def block():
    return int(_lib.load().seg3d_optim_block_elems())


class Case:
    """One optimizer over the shapes of optim_ref plus: [-3] a copy of the (block + 1)-element tensor whose gradient is a
    view at element offset 1 of a larger buffer (4-byte aligned: the scalar path), [-2] a copy of the 65-element tensor
    whose state buffers get misaligned after the first step, [-1] a parameter that never has a gradient."""

    def __init__(self, variant, device, start):
        cls, group_kw = VARIANTS[variant]
        b = block()
        sizes = R.sizes(b)
        self.start = start + [start[sizes.index(b + 1)].clone(), start[sizes.index(65)].clone(), torch.ones(7)]
        self.device = device
        self.params = [t.clone().to(device).requires_grad_() for t in self.start]
        self.opt = cls(R.split_groups(self.params, group_kw))
        self.i_offset, self.i_state, self.i_none = len(self.start) - 3, len(self.start) - 2, len(self.start) - 1

    def set_grads(self, it):
        grads = R.make_grads(self.start, it)
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if i == self.i_none:
                p.grad = None
            elif i == self.i_offset:
                buf = torch.zeros(g.numel() + 5, device=self.device)
                buf[1:1 + g.numel()].copy_(g)
                p.grad = buf[1:1 + g.numel()]
                assert p.grad.data_ptr() % 16 == 4
            else:
                p.grad = g.to(self.device)

    def misalign_state(self):
        """Through the public surface: load_state_dict keeps a state tensor that already has the parameter's device and
        dtype, so a view at element offset 1 stays where it is."""
        sd = self.opt.state_dict()
        pid = [i for g, packed in zip(self.opt.param_groups, sd["param_groups"]) for q, i in zip(g["params"], packed["params"])
               if q is self.params[self.i_state]][0]
        entry = sd["state"].get(pid, {})
        moved = 0
        for k, v in list(entry.items()):
            if k != "step":
                buf = torch.zeros(v.numel() + 5, device=self.device)
                buf[1:1 + v.numel()].copy_(v)
                entry[k] = buf[1:1 + v.numel()]
                moved += 1
        self.opt.load_state_dict(sd)
        for k, v in self.opt.state[self.params[self.i_state]].items():
            if k != "step":
                assert v.data_ptr() % 16 == 4, k
        return moved

    def snapshot(self):
        out = [p.detach().cpu().clone() for p in self.params]
        for p in self.params:
            for k, v in sorted(self.opt.state.get(p, {}).items()):
                out.append(v.detach().cpu().clone())
        return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_is_bit_identical_to_the_host_twin(dev, variant):
    start = R.make_params(block())
    gpu, cpu = Case(variant, dev, list(start)), Case(variant, torch.device("cpu"), list(start))
    for it in range(5):
        gpu.set_grads(it), cpu.set_grads(it)
        gpu.opt.step(), cpu.opt.step()
        if it == 0:
            assert gpu.misalign_state() == cpu.misalign_state() == {"sgd_momentum": 1, "sgd_plain": 0, "adamw": 2}[variant]
        if it in (0, 1, 4):
            a, b = gpu.snapshot(), cpu.snapshot()
            assert len(a) == len(b)
            bad = [i for i, (x, y) in enumerate(zip(a, b)) if not torch.equal(x, y)]
            assert not bad, (it, bad)
    assert torch.equal(gpu.params[gpu.i_none].detach().cpu(), torch.ones(7)) and gpu.params[gpu.i_none] not in gpu.opt.state
    assert not torch.equal(gpu.params[0].detach().cpu(), start[0])  # and the steps did move the values
    for p in gpu.params:
        assert torch.isfinite(p).all()


def record_calls(monkeypatch):
    names, call = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    monkeypatch.setattr(_lib, "call", recording)
    return names


@pytest.mark.parametrize("variant", ["sgd_momentum", "adamw"])
def test_steady_state_is_one_call_and_no_sync(dev, monkeypatch, variant):
    """Steps three and four: one library call each, nothing that synchronises, the table of step two reused although the
    learning rate changed in between; after zero_grad(set_to_none=True) and a new backward still one call, on a new table."""
    cls, group_kw = VARIANTS[variant]
    params = [t.to(dev).requires_grad_() for t in R.make_params(block())]
    opt = cls(R.split_groups(params, group_kw))
    sched = optim.WarmupPolyLR(opt, max_iters=20, warmup_iters=4)

    def backward():
        sum((p * (i + 1.0)).sum() for i, p in enumerate(params)).backward()

    backward()
    for _ in range(2):  # the first step builds the table, the second drops SGD's first-step flags
        opt.step()
        sched.step()
    names = record_calls(monkeypatch)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        table = opt._plans[dev].table
        lrs = []
        for _ in range(2):
            before = len(names)
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
            assert names[before:] == ["seg3d_optim_step"]
            assert opt._plans[dev].table is table
        assert lrs[0] != lrs[1]
        old = [p.grad for p in params]  # kept alive: the new gradients get other addresses
        opt.zero_grad(set_to_none=True)
        backward()
        before = len(names)
        opt.step()
        assert names[before:] == ["seg3d_optim_step"]
        assert opt._plans[dev].table is not table
        del old
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in params)


@pytest.mark.parametrize("variant", ["sgd_momentum", "adamw"])
def test_more_hyper_sets_than_one_launch_holds(dev, monkeypatch, variant):
    cls, group_kw = VARIANTS[variant]
    n_groups = _lib.OPTIM_MAX_HYPER + 1
    b = block()
    gen = torch.Generator().manual_seed(5)
    start = [torch.randn(n, generator=gen) for _ in range(n_groups) for n in (65, b + 1)]
    kws = [dict(group_kw[0], lr=group_kw[0]["lr"] * (1 + 0.1 * i), weight_decay=1e-3 * i) for i in range(n_groups)]

    def make(device):
        ps = [t.clone().to(device).requires_grad_() for t in start]
        return ps, cls([dict(kw, params=ps[2 * i:2 * i + 2]) for i, kw in enumerate(kws)])

    (gp, gopt), (cp, copt) = make(dev), make(torch.device("cpu"))
    names = record_calls(monkeypatch)
    for it in range(2):
        for p, q, g in zip(gp, cp, R.make_grads(start, it)):
            p.grad, q.grad = g.to(dev), g.clone()
        gopt.step(), copt.step()
    assert sorted(names) == ["seg3d_optim_step"] * 4 + ["seg3d_optim_step_host"] * 4  # two launches per step and side
    for i, (p, q) in enumerate(zip(gp, cp)):
        assert torch.equal(p.detach().cpu(), q.detach()), i
        for k, v in copt.state[q].items():
            assert torch.equal(gopt.state[p][k].cpu(), v), (i, k)
    # every group really used its own scalars: two groups with the same start and gradient end apart
    assert not torch.equal(cp[0].detach() - start[0], cp[2].detach() - start[2])


class PackNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from openseg3d_amd import spconv
        self.conv = spconv.SubMConv3d(48, 48, 3, padding=1, bias=True)
        self.bn = torch.nn.BatchNorm1d(48, eps=1e-3)
        self.lin = torch.nn.Linear(48, 32)

    def forward(self, t):
        from openseg3d_amd import ops
        if self.training:
            y = self.conv(t).features
        else:
            y = self.conv.forward_bn_act(t, self.bn, relu=True).features  # BatchNorm folded into the packed weights
        return ops.linear(y, self.lin.weight, self.lin.bias)


@pytest.mark.parametrize("mode", ["train", "eval_folded"])
@pytest.mark.parametrize("variant", ["sgd_momentum", "adamw"])
def test_packed_and_folded_weights_follow_the_step(dev, variant, mode):
    """The step writes parameters behind autograd's back (no Tensor._version bump), like torch's fused optimizers; the
    library's optimizer post-step hook must fire for these classes too.  forward, step, forward == a fresh module built
    from the updated state_dict, bit for bit."""
    from openseg3d_amd import spconv
    rs = np.random.RandomState(3)
    shape = [8, 12, 12]
    flat = rs.choice(shape[0] * shape[1] * shape[2], 200, replace=False)
    coords = np.stack([np.zeros_like(flat), flat // 144, flat // 12 % 12, flat % 12], 1).astype(np.int32)
    coords_d = torch.from_numpy(coords).to(dev)
    torch.manual_seed(11)
    x = torch.randn(200, 48, device=dev)
    net = PackNet().to(dev)
    with torch.no_grad():
        net.bn.running_mean.normal_()
        net.bn.running_var.uniform_(0.5, 2.0)
        net.bn.weight.normal_()
    cls, group_kw = VARIANTS[variant]
    opt = cls(net.parameters(), **dict(group_kw[0], lr=0.05))

    def forward(m):
        t = spconv.SparseConvTensor(x, coords_d, shape, 1)
        if mode == "train":
            return m.train()(t)
        with torch.no_grad():
            return m.eval()(t)

    first = forward(net)
    if mode == "train":
        first.square().mean().backward()
        assert net.conv.weight.grad.abs().max() > 0
    else:
        for p in net.parameters():
            p.grad = torch.randn_like(p) * 0.1
    before = net.conv.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, net.conv.weight.detach())
    second = forward(net).detach()
    fresh = PackNet().to(dev)
    fresh.load_state_dict(net.state_dict())
    want = forward(fresh).detach()
    assert torch.equal(second, want), float((second - want).abs().max())
    assert not torch.equal(second, first.detach())


@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_three_training_steps_through_the_builders(dev, name):
    """The small training case of tests/test_gpu_training.py with build_optimizer / build_scheduler instead of
    torch.optim.SGD: the same batch three times, the loss must fall."""
    from openseg3d_amd import batch as B, config, scene, segformer
    torch.manual_seed(0)
    cfg = config.default_cfg()
    cfg.TRAIN.OPTIMIZER = name
    cfg.TRAIN.LR_SCHEDULER = "cosine_annealing"
    if name == "sgd":
        cfg.TRAIN.LR = 0.01
    ds = config.DatasetSpec(cfg)
    model = segformer.build_segmentor(cfg, ds).to(dev).train()
    opt = optim.build_optimizer(cfg, model)
    sched = optim.build_scheduler(cfg, opt, 1, 100)
    assert type(opt) is (optim.SGD if name == "sgd" else optim.AdamW)
    samples = [scene.make_small_scene(7, 6000, extent=9.0), scene.make_small_scene(8, 4000, extent=6.0)]
    ce = torch.nn.functional.cross_entropy
    losses = []
    for _ in range(3):
        b = B.make_batch(samples, ds.voxel_size, ds.point_cloud_range)
        labels = torch.arange(b["points"].shape[0], device=dev) % 22
        opt.zero_grad(set_to_none=True)
        res = model(b)
        loss = (ce(res["point_out"], labels) + ce(res["voxel_out"], labels[:1].expand(res["voxel_out"].shape[0]))
                + 0.4 * ce(res["aux_voxel_out"], labels[:1].expand(res["aux_voxel_out"].shape[0])))
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss))
    assert all(l == l and l < 1e4 for l in losses)
    assert losses[-1] < losses[0], losses
    assert all(torch.isfinite(p).all() for p in model.parameters())


@pytest.mark.parametrize("first", [False, True])
def test_step_under_stream_capture_is_refused(dev, first):
    """The hyper-parameters travel by value in the kernel arguments: a captured step would replay frozen ones.  Refused as
    the very first step too, it has created no momentum buffer, and the eager retry is a true first step."""
    p = torch.ones(100, device=dev, requires_grad=True)
    p.grad = torch.ones(100, device=dev)
    opt = optim.SGD([p], lr=0.1, momentum=0.9)
    if not first:
        opt.step()
    torch.cuda.synchronize()
    after_one = p.detach().clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            with pytest.raises(NotImplementedError, match="capture"):
                opt.step()
        finally:
            graph.capture_end()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(p.detach(), after_one)
    if first:
        assert len(opt.state) == 0
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(p.detach().cpu(), torch.full((100,), 1.0) - torch.tensor(0.1) * 1.0)
        assert torch.equal(opt.state[p]["momentum_buffer"].cpu(), torch.ones(100))
