"""openseg3d_amd.optim on the CPU: the host twin of the multi-tensor step (seg3d_optim_step_host, the arithmetic the GPU
kernel shares bit for bit) against float64 and against torch.optim, state-dict interchange, the builders and schedules."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import optim_ref as R
from openseg3d_amd import _lib, config, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGOS = {"sgd": (optim.SGD, torch.optim.SGD, R.SGD_GROUPS), "adamw": (optim.AdamW, torch.optim.AdamW, R.ADAMW_GROUPS)}


def block():
    return int(_lib.load().seg3d_optim_block_elems())


def leaves(tensors):
    return [t.clone().requires_grad_() for t in tensors]


def set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()


def allowed(torch_err):
    """At most twice torch's own distance from float64; 1 ulp where torch's is 0."""
    return 2.0 * torch_err if torch_err > 0 else 1.0


def run_three(algo, n_steps, skip=None):
    """ours (host twin), torch foreach=False and float64 from one start over the same gradients -> params, optimizers"""
    ours_cls, torch_cls, group_kw = ALGOS[algo]
    start = R.make_params(block())
    a, b = leaves(start), leaves(start)
    ours = ours_cls(R.split_groups(a, group_kw))
    theirs = torch_cls(R.split_groups(b, group_kw), foreach=False)
    ref = R.Ref64(algo, start, [i % len(group_kw) for i in range(len(start))], group_kw)
    for it in range(n_steps):
        grads = R.make_grads(start, it)
        if skip is not None and it == skip[0]:
            grads[skip[1]] = None
        set_grads(a, grads), set_grads(b, grads)
        ours.step(), theirs.step(), ref.step(grads)
    return a, b, ref, ours, theirs


@pytest.mark.parametrize("algo", ["sgd", "adamw"])
def test_host_twin_vs_float64(algo):
    """Five steps, fresh gradients each, two groups with different lr / weight decay, every size of optim_ref.sizes.
    Yardstick: torch's own fp32 CPU optimizer (foreach=False) against the same float64 run; the twin may be at most twice
    as far from float64 as torch, per tensor, in max |dp| / ulp(|p|) (1 ulp where torch's error is 0): both are fp32
    evaluations of one formula and differ only in where a multiply-add is fused.
    Measured, worst tensor (the [48, 3, 3, 3, 48] weight or the 8199-element vector; the large figures belong to elements
    that pass close to zero, where ulp(|p|) is tiny): SGD twin 3645 ulp / torch 7079 ulp; AdamW twin 1258 / torch 1002;
    on the tensors of up to 65 elements both stay below 6 ulp and mostly agree to the digit."""
    a, b, ref, _, _ = run_three(algo, 5)
    rows = []
    for i, (p, q) in enumerate(zip(a, b)):
        rows.append((tuple(p.shape), R.ulp_error(p, ref.p[i]), R.ulp_error(q, ref.p[i])))
    print(algo, "twin / torch ulp:", [(s, round(e, 2), round(t, 2)) for s, e, t in rows])
    print(algo, "worst: twin %.2f torch %.2f" % (max(r[1] for r in rows), max(r[2] for r in rows)))
    for shape, e, t in rows:
        assert e <= allowed(t), (algo, shape, e, t)


def test_adamw_scalars_are_pinned():
    """optim.adamw_scalars / sgd_scalars against literals: (1 - lr wd, 1 - beta1, beta2, 1 - beta2, lr / bc1, sqrt(bc2), eps)
    for the two groups of optim_ref at a few step counts, worked out in 40-digit decimal arithmetic.  1e-12 relative:
    the function is double arithmetic and loses at most 1 / (1 - beta) = 1000 times 1.1e-16 in its subtractions."""
    g0, g1 = R.ADAMW_GROUPS
    want = {
        (0, 1): (0.99999, 0.1, 0.999, 0.001, 1e-2, 3.162277660168379e-2, 1e-8),
        (0, 3): (0.99999, 0.1, 0.999, 0.001, 3.690036900369004e-3, 5.474487190596029e-2, 1e-8),
        (1, 2): (0.9997, 0.15, 0.99, 0.01, 1.081081081081081e-2, 1.410673597966588e-1, 1e-6),
        (1, 1000): (0.9997, 0.15, 0.99, 0.01, 3e-3, 9.999784141433201e-1, 1e-6),
    }
    for (gi, step), w in want.items():
        g = (g0, g1)[gi]
        got = optim.adamw_scalars(g["lr"], g["betas"], g["eps"], g["weight_decay"], float(step))
        assert len(got) == 8 and got[7] == 0.0
        for k, (x, y) in enumerate(zip(got, w)):
            assert abs(x - y) <= 1e-12 * abs(y), (gi, step, k, x, y)
    assert optim.sgd_scalars(0.05, 1e-4, 0.9) == (0.05, 1e-4, 0.9, 0.0, 0.0, 0.0, 0.0, 0.0)


def same_structure(a, b):
    """keys and value types of two optimizer state dicts"""
    assert a.keys() == b.keys()
    assert len(a["param_groups"]) == len(b["param_groups"])
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert list(ga.keys()) == list(gb.keys())
        for k in ga:
            if k not in ("foreach", "fused"):  # the implementation choice of torch's own step; None / False / True
                assert type(ga[k]) is type(gb[k]), k
        assert ga["params"] == gb["params"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys(), k
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert type(x) is type(y) and x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, (k, name)


@pytest.mark.parametrize("direction", ["ours_to_torch", "torch_to_ours"])
@pytest.mark.parametrize("algo", ["sgd", "adamw"])
def test_state_dict_interchange(algo, direction):
    """Three steps on one side, the state dict through torch.save / torch.load into the other class, two more steps on
    each side: both continuations stay within the tolerance of test_host_twin_vs_float64 of the float64 run, and the
    dicts of the two classes have the same keys and value types."""
    ours_cls, torch_cls, group_kw = ALGOS[algo]
    start = R.make_params(block())
    src_p, dst_p, yard_p = leaves(start), leaves(start), leaves(start)
    make_ours = lambda ps: ours_cls(R.split_groups(ps, group_kw))
    make_torch = lambda ps: torch_cls(R.split_groups(ps, group_kw), foreach=False)
    src, dst = (make_ours(src_p), make_torch(dst_p)) if direction == "ours_to_torch" else (make_torch(src_p), make_ours(dst_p))
    yard = make_torch(yard_p)
    ref = R.Ref64(algo, start, [i % len(group_kw) for i in range(len(start))], group_kw)
    for it in range(5):
        grads = R.make_grads(start, it)
        set_grads(src_p, grads), set_grads(yard_p, grads)
        src.step(), yard.step(), ref.step(grads)
        if it == 2:
            buf = io.BytesIO()
            torch.save(src.state_dict(), buf)
            buf.seek(0)
            dst.load_state_dict(torch.load(buf))
            same_structure(src.state_dict(), dst.state_dict())
            with torch.no_grad():
                for p, q in zip(dst_p, src_p):
                    p.copy_(q)
        if it > 2:
            set_grads(dst_p, grads)
            dst.step()
    same_structure(src.state_dict(), dst.state_dict())
    for i in range(len(start)):
        t = R.ulp_error(yard_p[i], ref.p[i])
        assert R.ulp_error(src_p[i], ref.p[i]) <= allowed(t), (i, "source side")
        assert R.ulp_error(dst_p[i], ref.p[i]) <= allowed(t), (i, "loaded side")
    if algo == "adamw":
        steps = [float(s["step"]) for s in dst.state_dict()["state"].values()]
        assert steps and all(s == 5.0 for s in steps)


@pytest.mark.parametrize("algo", ["sgd", "adamw"])
def test_parameter_without_gradient_is_skipped(algo):
    """grad None on the second step: the value stays, no state is touched, AdamW's step count lags by one and the third
    step uses the parameter's own bias corrections: the step counts equal torch's, and the values stay within the
    tolerance of test_host_twin_vs_float64 of a float64 run that counts each parameter's steps itself."""
    which = 6  # the 65-element tensor
    for n_steps in (2, 3):
        a, b, ref, ours, theirs = run_three(algo, n_steps, skip=(1, which))
        if n_steps == 2:
            one, _, _, _, _ = run_three(algo, 1)
            assert torch.equal(a[which], one[which])
        for i, (p, q) in enumerate(zip(a, b)):
            assert R.ulp_error(p, ref.p[i]) <= allowed(R.ulp_error(q, ref.p[i])), i
        if algo == "adamw":
            assert float(ours.state[a[which]]["step"]) == n_steps - 1 == float(theirs.state[b[which]]["step"])
            assert float(ours.state[a[0]]["step"]) == n_steps
    # a parameter that never had a gradient has no state at all
    p, q = leaves([torch.ones(5), torch.ones(7)])
    o = ALGOS[algo][0]([p, q], lr=0.1, **({"momentum": 0.9} if algo == "sgd" else {}))
    p.grad = torch.ones(5)
    o.step()
    assert q not in o.state and len(o.state_dict()["state"]) == 1 and torch.equal(q, torch.ones(7))


def test_sgd_without_momentum_keeps_no_state():
    p, q = leaves([torch.arange(5.0)] * 2)
    ours, theirs = optim.SGD([p], lr=0.1, weight_decay=0.01), torch.optim.SGD([q], lr=0.1, weight_decay=0.01, foreach=False)
    for _ in range(2):
        p.grad, q.grad = torch.full((5,), 0.5), torch.full((5,), 0.5)
        ours.step(), theirs.step()
    assert len(ours.state) == 0 and ours.state_dict()["state"] == theirs.state_dict()["state"] == {}
    assert torch.allclose(p, q, rtol=0, atol=1e-6) and not torch.equal(p.detach(), torch.arange(5.0))


class TinyModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 3)
        self.b = torch.nn.Linear(3, 2)


def test_builders_follow_the_config(tmp_path):
    model = TinyModel()
    cfg = config.default_cfg()
    opt = optim.build_optimizer(cfg, model)
    assert type(opt) is optim.AdamW and len(opt.param_groups) == 1
    g = opt.param_groups[0]
    assert g["lr"] == 0.001 and g["weight_decay"] == 0.01 and g["betas"] == (0.9, 0.999) and len(g["params"]) == 4
    sched = optim.build_scheduler(cfg, opt, 7, 11)
    assert type(sched) is optim.WarmupPolyLR and sched.max_iters == 77 and sched.warmup_iters == 11
    assert sched.warmup_factor == 0.001 and sched.warmup_method == "linear" and sched.power == 0.9
    # the reference's three YAML files (configs/waymo_*.yaml) share one and the same TRAIN block: this one, through the
    # YAML loader
    path = tmp_path / "train.yaml"
    path.write_text("TRAIN:\n  LR: 0.05\n  OPTIMIZER: 'sgd'\n  WEIGHT_DECAY: 0.0001\n  MOMENTUM: 0.9\n")
    cfg = config.cfg_from_file(str(path))
    opt = optim.build_optimizer(cfg, model)
    g = opt.param_groups[0]
    assert type(opt) is optim.SGD and (g["lr"], g["weight_decay"], g["momentum"]) == (0.05, 1e-4, 0.9)
    assert g["dampening"] == 0 and g["nesterov"] is False
    cfg.TRAIN.LR_SCHEDULER = "cosine_annealing"
    sched = optim.build_scheduler(cfg, opt, 3, 5)
    assert type(sched) is torch.optim.lr_scheduler.CosineAnnealingLR and sched.T_max == 15
    cfg.TRAIN.LR_SCHEDULER = "one_cycle"
    sched = optim.build_scheduler(cfg, optim.build_optimizer(cfg, model), 3, 5)
    assert type(sched) is torch.optim.lr_scheduler.OneCycleLR and sched.total_steps == 15
    cfg.TRAIN.LR_SCHEDULER = "step"
    with pytest.raises(NotImplementedError):
        optim.build_scheduler(cfg, opt, 3, 5)
    cfg.TRAIN.OPTIMIZER = "adam"
    with pytest.raises(NotImplementedError):
        optim.build_optimizer(cfg, model)


@pytest.mark.parametrize("algo", ["sgd", "adamw"])
def test_one_cycle_drives_momentum_and_betas(algo):
    """OneCycleLR rewrites lr and momentum (SGD) / betas[0] (AdamW) in the groups every step; the step reads them every
    time: three steps next to torch's optimizer under the same scheduler."""
    cfg = config.default_cfg()
    cfg.TRAIN.OPTIMIZER, cfg.TRAIN.LR_SCHEDULER, cfg.TRAIN.LR = algo, "one_cycle", 0.05 if algo == "sgd" else 0.002
    torch.manual_seed(0)
    m1, m2 = TinyModel(), TinyModel()
    m2.load_state_dict(m1.state_dict())
    ours = optim.build_optimizer(cfg, m1)
    if algo == "sgd":
        theirs = torch.optim.SGD(m2.parameters(), lr=cfg.TRAIN.LR, weight_decay=cfg.TRAIN.WEIGHT_DECAY,
                                 momentum=cfg.TRAIN.MOMENTUM, foreach=False)
    else:
        theirs = torch.optim.AdamW(m2.parameters(), lr=cfg.TRAIN.LR, weight_decay=cfg.TRAIN.WEIGHT_DECAY, foreach=False)
    s1, s2 = optim.build_scheduler(cfg, ours, 2, 5), optim.build_scheduler(cfg, theirs, 2, 5)
    start = [p.detach().clone() for p in m1.parameters()]
    ref = R.Ref64(algo, start, [0] * len(start), [None])
    seen = []
    for it in range(3):
        grads = R.make_grads(start, it)
        set_grads(list(m1.parameters()), grads), set_grads(list(m2.parameters()), grads)
        g1, g2 = ours.param_groups[0], theirs.param_groups[0]
        key = "momentum" if algo == "sgd" else "betas"
        assert g1["lr"] == g2["lr"] and g1[key] == g2[key]
        seen.append((g1["lr"], g1[key]))
        ref.group_kw = [dict(g1)]
        ours.step(), theirs.step(), ref.step(grads)
        s1.step(), s2.step()
    assert len({s[0] for s in seen}) == 3 and len({s[1] for s in seen}) == 3  # both really moved
    for i, (p, q) in enumerate(zip(m1.parameters(), m2.parameters())):
        assert R.ulp_error(p, ref.p[i]) <= allowed(R.ulp_error(q, ref.p[i])), i
    # ... and not what constant hyper-parameters would have given
    m3 = TinyModel()
    m3.load_state_dict({k: v for k, v in zip(m1.state_dict().keys(), start)})
    const = optim.build_optimizer(cfg, m3)
    for it in range(3):
        set_grads(list(m3.parameters()), R.make_grads(start, it))
        const.step()
    assert not torch.equal(m3.a.weight, m1.a.weight)


@pytest.mark.parametrize("variant,kw", [("linear", {}), ("constant", {"warmup_method": "constant"}),
                                        ("constant_ending", {"constant_ending": 0.1})])
def test_warmup_poly_lr_matches_the_recorded_schedule(golden_dir, variant, kw):
    """tests/golden/lr_schedules.npz: the reference class's learning rates over a whole 40-iteration schedule
    (tests/golden/make_golden_lr.py); both sides are double arithmetic."""
    d = np.load(os.path.join(golden_dir, "lr_schedules.npz"))
    base = d["base_lrs"].tolist()
    params = leaves([torch.zeros(1) for _ in base])
    opt = optim.SGD([{"params": [p], "lr": lr} for p, lr in zip(params, base)], lr=1.0)
    sched = optim.WarmupPolyLR(opt, max_iters=int(d["max_iters"]), warmup_iters=int(d["warmup_iters"]), **kw)
    rows = [[g["lr"] for g in opt.param_groups]]
    for _ in range(int(d["max_iters"])):
        set_grads(params, [torch.zeros(1) for _ in base])
        opt.step()
        sched.step()
        rows.append([g["lr"] for g in opt.param_groups])
        assert sched.get_last_lr() == rows[-1]
    want = d[variant]
    got = np.array(rows)
    assert got.shape == want.shape == (41, 2)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), np.abs(got - want).max()
    with pytest.raises(ValueError):
        optim.WarmupPolyLR(opt, max_iters=10, warmup_method="cosine")


def test_refused_options_name_themselves():
    p = leaves([torch.zeros(4)])
    for cls, kw, name in ((optim.SGD, dict(nesterov=True, momentum=0.9), "nesterov"), (optim.SGD, dict(dampening=0.1), "dampening"),
                          (optim.SGD, dict(maximize=True), "maximize"), (optim.AdamW, dict(amsgrad=True), "amsgrad"),
                          (optim.AdamW, dict(maximize=True), "maximize")):
        with pytest.raises(NotImplementedError, match=name):
            cls(p, lr=0.1, **kw)
        o = cls(p, lr=0.1)  # ... and when the option arrives later, through the groups
        o.param_groups[0].update(kw)
        p[0].grad = torch.ones(4)
        with pytest.raises(NotImplementedError, match=name):
            o.step()
    for cls in (optim.SGD, optim.AdamW):
        q = leaves([torch.zeros(4, dtype=torch.float64)])
        q[0].grad = torch.ones(4, dtype=torch.float64)
        with pytest.raises(NotImplementedError, match="float32"):
            cls(q, lr=0.1).step()
        q = [torch.zeros(4, 6).t().requires_grad_()]
        q[0].grad = torch.ones(6, 4)
        with pytest.raises(NotImplementedError, match="non-contiguous"):
            cls(q, lr=0.1).step()
        q = leaves([torch.zeros(4, 3)])
        q[0].grad = torch.ones(4, 3).to_sparse()
        with pytest.raises(NotImplementedError, match="sparse"):
            cls(q, lr=0.1).step()
        # a refused step has changed nothing: no counter moved
        q = leaves([torch.zeros(4), torch.zeros(4, dtype=torch.float64)])
        q[0].grad, q[1].grad = torch.ones(4), torch.ones(4, dtype=torch.float64)
        o = cls(q, lr=0.1)
        with pytest.raises(NotImplementedError):
            o.step()
        assert torch.equal(q[0].detach(), torch.zeros(4))
        assert len(o.state) == 0 and o.state_dict()["state"] == {}


@pytest.mark.parametrize("how", ["later_parameter", "later_group"])
@pytest.mark.parametrize("algo", ["sgd", "adamw"])
def test_refused_step_creates_no_state(algo, how):
    """A step() that raises for a later parameter, or for an option of a later group, has created no state for the
    earlier ones (SGD with momentum: no momentum buffer that the next step would read as if it had been written); the
    step retried once the cause is gone equals the first step of an optimizer that was never refused, bit for bit."""
    cls = ALGOS[algo][0]
    kw = dict(lr=0.1, momentum=0.9) if algo == "sgd" else dict(lr=0.1)
    bad = dict(nesterov=True) if algo == "sgd" else dict(amsgrad=True)
    start = [torch.linspace(-1, 1, 9), torch.linspace(1, 2, 5)]
    grads = [torch.linspace(0.5, -0.5, 9), torch.linspace(-1, 1, 5)]
    p, q = leaves(start)
    wrong = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    o = cls([dict(params=[p]), dict(params=[q, wrong])], **kw)
    p.grad, q.grad = grads[0].clone(), grads[1].clone()
    if how == "later_parameter":
        wrong.grad = torch.ones(4, dtype=torch.float64)
    else:
        o.param_groups[1].update(bad)
    with pytest.raises(NotImplementedError):
        o.step()
    assert len(o.state) == 0 and o.state_dict()["state"] == {}
    assert torch.equal(p.detach(), start[0]) and torch.equal(q.detach(), start[1])
    wrong.grad = None
    o.param_groups[1].update({k: False for k in bad})
    o.step()
    p2, q2 = leaves(start)
    fresh = cls([dict(params=[p2]), dict(params=[q2])], **kw)
    p2.grad, q2.grad = grads[0].clone(), grads[1].clone()
    fresh.step()
    assert torch.equal(p, p2) and torch.equal(q, q2) and not torch.equal(p.detach(), start[0])
    for x, y in ((p, p2), (q, q2)):
        assert o.state[x].keys() == fresh.state[y].keys()
        for k in o.state[x]:
            assert torch.equal(o.state[x][k], fresh.state[y][k]), k


def test_non_contiguous_gradient_is_made_contiguous():
    p, q = leaves([torch.ones(6, 4)] * 2)
    g = torch.arange(24.0).reshape(4, 6).t()
    assert not g.is_contiguous()
    p.grad, q.grad = g, g.contiguous()
    optim.SGD([p], lr=0.1).step(), optim.SGD([q], lr=0.1).step()
    assert torch.equal(p, q) and not torch.equal(p.detach(), torch.ones(6, 4))


def test_host_entry_arguments():
    lib = _lib.load()
    assert lib.seg3d_optim_block_elems() >= 256 and lib.seg3d_optim_block_elems() % 4 == 0
    hyper = (ctypes.c_float * 8)(0.1, 0, 0, 0, 0, 0, 0, 0)
    p, g = np.ones(5, np.float32), np.ones(5, np.float32)
    rec = np.zeros(1, dtype=optim._RECORD)
    rec[0] = (p.ctypes.data, g.ctypes.data, 0, 0, 5, 0, 0, 0, 0)
    table = ctypes.c_void_p(rec.ctypes.data)
    f = lib.seg3d_optim_step_host
    assert f(None, 1, 1, hyper, 1, _lib.OPTIM_SGD) == _lib.EINVAL        # null table with n > 0
    assert f(table, -1, 1, hyper, 1, _lib.OPTIM_SGD) == _lib.EINVAL      # negative count
    assert f(table, 1, -1, hyper, 1, _lib.OPTIM_SGD) == _lib.EINVAL
    assert f(table, 1, 1, hyper, 1, 2) == _lib.EINVAL                    # unknown algo
    assert f(table, 1, 1, hyper, 1, -1) == _lib.EINVAL
    assert f(table, 1, 1, None, 1, _lib.OPTIM_SGD) == _lib.EINVAL
    assert f(table, 1, 1, hyper, _lib.OPTIM_MAX_HYPER + 1, _lib.OPTIM_SGD) == _lib.EINVAL
    assert f(table, 1, 1, hyper, 1, _lib.OPTIM_ADAMW) == _lib.EINVAL     # AdamW without its state
    assert f(table, 1, 2, hyper, 1, _lib.OPTIM_SGD) == _lib.EINVAL       # total_blocks does not match the table
    assert np.array_equal(p, np.ones(5, np.float32))                      # a refused call writes nothing
    assert f(None, 0, 0, None, 0, _lib.OPTIM_SGD) == 0 and f(table, 0, 0, hyper, 1, _lib.OPTIM_ADAMW) == 0  # n = 0: no-op
    assert np.array_equal(p, np.ones(5, np.float32))
    assert f(table, 1, 1, hyper, 1, _lib.OPTIM_SGD) == 0
    assert np.array_equal(p, np.ones(5, np.float32) - np.float32(0.1) * np.float32(1.0))
    # the device entry refuses the same calls before any launch (nothing here touches a GPU)
    d = lib.seg3d_optim_step
    assert d(None, 1, 1, hyper, 1, _lib.OPTIM_SGD, None) == _lib.EINVAL
    assert d(table, -1, 1, hyper, 1, _lib.OPTIM_SGD, None) == _lib.EINVAL
    assert d(table, 1, 1, hyper, 1, 7, None) == _lib.EINVAL
    assert d(None, 0, 0, None, 0, _lib.OPTIM_SGD, None) == 0
    assert optim.SGD(leaves([torch.zeros(0)]), lr=0.1).step() is None  # nothing to do, no call fails
