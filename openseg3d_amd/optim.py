"""Optimizers and LR schedules of the training loop (tools/train.py:136-149; seg3d/models/builder.py:43-67).

``SGD`` and ``AdamW`` are ``torch.optim.Optimizer`` subclasses whose ``step()`` updates every parameter by ONE launch of
the library's multi-tensor kernel (csrc/optim.hip): ``param_groups`` keys and per-parameter state are
torch's, so ``state_dict()`` / ``load_state_dict()`` interchange with ``torch.optim`` and torch's schedulers
(``CosineAnnealingLR``, ``OneCycleLR``) drive them unchanged.  CUDA parameters go to ``seg3d_optim_step``, CPU parameters
to its plain-C++ host twin ``seg3d_optim_step_host`` (the same arithmetic bit for bit); neither is a fallback for the
other.  float32 only.

A steady-state step compares pointers on the host and makes one library call: the record table is kept on the device
and rebuilt only when a pointer, a count or a hyper-parameter-set assignment changes (``.grad`` re-allocated after
``zero_grad()``, redirected into the arena by ``dist.SceneParallel``); the hyper-parameters themselves travel in the
kernel arguments.  The library's global optimizer post-step hook (ops._register_optimizer_hook) fires for these classes
as for any torch optimizer, so packed and folded weights are rebuilt at their next use.

``clip_grad_norm_`` / ``GradClipper`` / ``grad_norm`` (and ``optimizer.clip_grad_norm_``) clip the global L2 norm of the
gradients between ``loss.backward()`` and ``step()`` on the same table design: three small launches beside the step, the
norm accumulated in fp64.
"""
import ctypes
import math

import numpy as np
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR, LRScheduler, OneCycleLR

from . import _lib
from . import ops  # noqa: F401  (registers the weight-cache hook on every optimizer step)

_RECORD = np.dtype(_lib.struct("seg3d_optim_tensor"))


def sgd_scalars(lr, weight_decay, momentum):
    """The scalar set of one SGD launch (seg3d_optim_hyper.v), as Python doubles."""
    return (float(lr), float(weight_decay), float(momentum), 0.0, 0.0, 0.0, 0.0, 0.0)


def adamw_scalars(lr, betas, eps, weight_decay, step):
    """The scalar set of one AdamW launch for a parameter at step count ``step`` (>= 1), as Python doubles: the
    expressions of torch's non-capturable single-tensor path, evaluated in double and rounded to float once."""
    lr, beta1, beta2 = float(lr), float(betas[0]), float(betas[1])
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return (1 - lr * weight_decay, 1 - beta1, beta2, 1 - beta2, lr / bias_correction1, bias_correction2 ** 0.5, float(eps),
            0.0)


class _Plan:
    """The record table of one device, as last uploaded."""
    __slots__ = ("sig", "table", "launches", "keep")


class _MultiTensorOptimizer(torch.optim.Optimizer):
    _ALGO = None

    def _refuse(self, group):
        raise NotImplementedError

    def _collect(self, gi, group, p):
        """-> (state0 pointer, state1 pointer, flags, scalar-set key) for one parameter with a gradient"""
        raise NotImplementedError

    def _scalars(self, group, key):
        """the scalar set (seg3d_optim_hyper.v) behind a key that _collect returned for a parameter of this group"""
        raise NotImplementedError

    def _begin(self):
        """nothing was refused: the step starts to create and count state"""

    def _collected(self):
        """every parameter of the step has been collected"""

    @staticmethod
    def _refuse_tensor(p, grad):
        if grad.is_sparse:
            raise NotImplementedError("sparse gradients are not supported by openseg3d_amd.optim")
        if p.dtype != torch.float32 or grad.dtype != torch.float32:
            raise NotImplementedError(f"non-float32 parameters are not supported by openseg3d_amd.optim (got {p.dtype} / "
                                      f"gradient {grad.dtype})")
        if not p.is_contiguous():
            raise NotImplementedError("non-contiguous parameters are not supported by openseg3d_amd.optim")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        block = _block_elems()
        f32 = torch.float32
        # every refusal comes first: a step() that raises has created no state and moved no counter
        work, cuda = [], False
        for gi, group in enumerate(self.param_groups):
            self._refuse(group)
            for p in group["params"]:
                grad = p.grad
                if grad is None:
                    continue
                if p.dtype is not f32 or grad.dtype is not f32 or grad.is_sparse or not p.is_contiguous():
                    self._refuse_tensor(p, grad)
                kind = p.device.type
                if kind == "cuda":
                    cuda = True
                elif kind != "cpu":
                    raise NotImplementedError(f"parameters on device {p.device} are not supported by openseg3d_amd.optim")
                work.append((gi, group, p, grad))
        if cuda and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("openseg3d_amd.optim: step() under stream capture is not supported (the hyper-"
                                      "parameters travel by value in the kernel arguments and would be frozen into the graph)")
        self._begin()
        collect = self._collect
        buckets = {}  # device -> (entries, set keys -> index, scalar sets, tensors kept alive over the call)
        last_dev = entries = set_index = sets = keep = None
        for gi, group, p, grad in work:
            dev = p.device
            if dev != last_dev:
                last_dev = dev
                if dev not in buckets:
                    buckets[dev] = ([], {}, [], [])
                entries, set_index, sets, keep = buckets[dev]
            if not grad.is_contiguous():
                grad = grad.contiguous()
                keep.append(grad)
            s0, s1, flags, key = collect(gi, group, p)
            n = p.numel()
            if n == 0:
                continue
            k = set_index.get(key)
            if k is None:
                k = set_index[key] = len(sets)
                sets.append(self._scalars(group, key))
            entries.append((p.data_ptr(), grad.data_ptr(), s0, s1, n, k, flags))
        self._collected()
        plans = self.__dict__.setdefault("_plans", {})
        for dev, (entries, _, sets, keep) in buckets.items():
            plan = plans.get(dev)
            if plan is None or plan.sig != entries:
                plan = plans[dev] = _build_plan(entries, dev, block)
            for first_set, n_sets, offset, n_rec, n_blocks in plan.launches:
                flat = [x for s in sets[first_set:first_set + n_sets] for x in s]
                hyper = (ctypes.c_float * len(flat))(*flat)
                if dev.type == "cuda":
                    with torch.cuda.device(dev):
                        _lib.call("seg3d_optim_step", ctypes.c_void_p(plan.table.data_ptr() + offset * 64), n_rec, n_blocks,
                                  hyper, n_sets, self._ALGO, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
                else:
                    _lib.call("seg3d_optim_step_host", ctypes.c_void_p(plan.table.ctypes.data + offset * 64), n_rec, n_blocks,
                              hyper, n_sets, self._ALGO)
        return loss

    def clip_grad_norm_(self, max_norm, error_if_nonfinite=False):
        """``clip_grad_norm_`` over this optimizer's own ``param_groups``, between ``loss.backward()`` and ``step()``; the
        clipper (record table, workspace) is kept on the optimizer.  Returns the total norm before clipping."""
        clipper = self.__dict__.get("_clipper")
        if clipper is None:
            clipper = self.__dict__["_clipper"] = GradClipper([], max_norm)
        clipper.params = [p for group in self.param_groups for p in group["params"]]
        clipper.max_norm = _checked_max_norm(max_norm)
        return clipper(error_if_nonfinite=error_if_nonfinite)


def _checked_max_norm(max_norm):
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError(f"max_norm must be >= 0, got {max_norm}")
    return max_norm


class _ClipPlan:
    """The gradient table of a GradClipper, as last uploaded, and the workspace of its norm pass."""
    __slots__ = ("sig", "dev", "table", "keep", "n", "blocks", "workspace", "workspace_bytes")


class GradClipper:
    """``torch.nn.utils.clip_grad_norm_`` (global L2 norm) on the library's table design (csrc/optim.hip):
    the norm in two launches with the squares summed in fp64 (``seg3d_grad_norm``), the scale in one that returns at once
    when the coefficient is 1 (``seg3d_grad_scale``).  ``clipper()`` clips in place and returns the total norm as a 0-d
    float32 tensor on the parameters' device; ``clipper.last_coef`` is the coefficient that was applied,
    min(max_norm / (norm + 1e-6), 1) in float32.  The table of (gradient pointer, count) records is kept across calls and
    rebuilt only when one of them changes; a steady-state call makes no host synchronisation and allocates the 8-byte
    result only.  CPU parameters run through the plain-C++ ``_host`` entries (the same definitions)."""

    def __init__(self, parameters, max_norm, norm_type=2.0):
        if isinstance(parameters, torch.Tensor):
            parameters = [parameters]
        if float(norm_type) != 2.0:
            raise NotImplementedError(f"norm_type={norm_type!r} is not supported by openseg3d_amd.optim (the L2 norm only)")
        self.params = list(parameters)
        self.max_norm = _checked_max_norm(max_norm)
        self.last_coef = None
        self._plan = None

    def __call__(self, error_if_nonfinite=False):
        return self._run(self.max_norm, True, error_if_nonfinite)

    def norm(self):
        """The norm pass alone: no gradient is written."""
        return self._run(math.inf, False, False)

    @torch.no_grad()
    def _run(self, max_norm, scale, error_if_nonfinite):
        entries, dev = [], None
        for p in self.params:
            grad = p.grad
            if grad is None:
                continue
            if p.dtype is not torch.float32 or grad.dtype is not torch.float32 or grad.is_sparse or not p.is_contiguous():
                _MultiTensorOptimizer._refuse_tensor(p, grad)
            if not grad.is_contiguous():
                raise NotImplementedError("non-contiguous gradients are not supported by openseg3d_amd.optim.GradClipper")
            if dev is None:
                dev = grad.device
                if dev.type not in ("cuda", "cpu"):
                    raise NotImplementedError(f"parameters on device {dev} are not supported by openseg3d_amd.optim")
            elif grad.device != dev:
                raise NotImplementedError(f"openseg3d_amd.optim.GradClipper: all parameters must live on one device, got "
                                          f"{dev} and {grad.device}")
            if grad.numel():
                entries.append((grad.data_ptr(), grad.numel()))
        if dev is None:  # no parameter has a gradient: norm 0, nothing to launch
            dev = self.params[0].device if self.params else torch.device("cpu")
            self.last_coef = torch.ones((), dtype=torch.float32, device=dev)
            return torch.zeros((), dtype=torch.float32, device=dev)
        cuda = dev.type == "cuda"
        if cuda and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("openseg3d_amd.optim: gradient clipping under stream capture is not supported (the "
                                      "record table follows the gradients' addresses from call to call)")
        plan = self._plan
        if plan is None or plan.sig != entries or plan.dev != dev:
            plan = self._plan = _build_clip_plan(entries, dev, _block_elems())
        if not cuda:
            result = np.zeros((2,), np.float32)
            args = (ctypes.c_void_p(plan.table.ctypes.data), plan.n, plan.blocks)
            _lib.call("seg3d_grad_norm_host", *args, max_norm, ctypes.c_void_p(result.ctypes.data))
            norm, coef = torch.tensor(result[0]), torch.tensor(result[1])
            if error_if_nonfinite and not math.isfinite(float(result[0])):
                raise RuntimeError(_NONFINITE)
            if scale:
                _lib.call("seg3d_grad_scale_host", *args, ctypes.c_void_p(result.ctypes.data + 4))
                self.last_coef = coef
            return norm
        with torch.cuda.device(dev):
            if ops._DEFERRED:  # weight gradients still pending on the side stream (a call from inside a backward pass)
                ops.finish_deferred(dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            result = torch.empty((2,), dtype=torch.float32, device=dev)
            args = (ctypes.c_void_p(plan.table.data_ptr()), plan.n, plan.blocks)
            _lib.call("seg3d_grad_norm", *args, max_norm, ctypes.c_void_p(plan.workspace.data_ptr()), plan.workspace_bytes,
                      ctypes.c_void_p(result.data_ptr()), stream)
            if error_if_nonfinite and not math.isfinite(float(result[0])):  # the one read-back
                raise RuntimeError(_NONFINITE)
            if scale:
                _lib.call("seg3d_grad_scale", *args, ctypes.c_void_p(result.data_ptr() + 4), stream)
                self.last_coef = result[1]
        return result[0]


_NONFINITE = ("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be clipped. To "
              "disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")


def _build_clip_plan(entries, dev, block):
    plan = _ClipPlan()
    plan.sig, plan.dev = list(entries), dev
    rec = np.zeros((len(entries),), dtype=_RECORD)
    blocks = 0
    for i, (g, n) in enumerate(entries):
        rec[i]["param"], rec[i]["count"], rec[i]["first_block"] = g, n, blocks
        blocks += (n + block - 1) // block
    plan.n, plan.blocks = len(entries), blocks
    plan.workspace_bytes = _lib.query("seg3d_grad_norm_workspace_bytes", blocks)
    if dev.type == "cuda":
        plan.keep = torch.from_numpy(rec.view(np.uint8)).pin_memory()
        plan.table = plan.keep.to(dev, non_blocking=True)
        plan.workspace = torch.empty((max(plan.workspace_bytes, 8),), dtype=torch.uint8, device=dev)
    else:
        plan.keep, plan.table, plan.workspace = None, rec, None
    return plan


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` with the squares summed in fp64 on the device (a transient GradClipper; a training
    loop keeps one, or calls the optimizer's ``clip_grad_norm_``).  ``foreach`` is accepted and ignored; with
    ``error_if_nonfinite=True`` the norm is read back once, before any gradient is written."""
    return GradClipper(parameters, max_norm, norm_type)(error_if_nonfinite=error_if_nonfinite)


def grad_norm(parameters):
    """The global L2 norm of the gradients (fp64 accumulation), nothing written: for logging."""
    return GradClipper(parameters, math.inf).norm()


def _block_elems(cache=[]):
    if not cache:
        cache.append(int(_lib.load().seg3d_optim_block_elems()))
    return cache[0]


def _build_plan(entries, dev, block):
    """Records grouped into launches of at most OPTIM_MAX_HYPER scalar sets each, uploaded once."""
    plan = _Plan()
    plan.sig = list(entries)
    order = sorted(range(len(entries)), key=lambda i: entries[i][5] // _lib.OPTIM_MAX_HYPER)  # stable
    rec = np.zeros((len(entries),), dtype=_RECORD)
    plan.launches = []
    n_sets_total = 1 + max((e[5] for e in entries), default=-1)
    at = 0
    for first_set in range(0, n_sets_total, _lib.OPTIM_MAX_HYPER):
        start, blocks = at, 0
        while at < len(order) and entries[order[at]][5] < first_set + _lib.OPTIM_MAX_HYPER:
            p, g, s0, s1, n, k, flags = entries[order[at]]
            rec[at] = (p, g, s0, s1, n, blocks, k - first_set, flags, 0)
            blocks += (n + block - 1) // block
            at += 1
        if at > start:
            n_sets = min(_lib.OPTIM_MAX_HYPER, n_sets_total - first_set)
            plan.launches.append((first_set, n_sets, start, at - start, blocks))
    if dev.type == "cuda":
        # pinned staging + asynchronous copy: a rebuild (every step after zero_grad(set_to_none=True)) stays sync-free
        plan.keep = torch.from_numpy(rec.view(np.uint8)).pin_memory()
        plan.table = plan.keep.to(dev, non_blocking=True)
    else:
        plan.keep, plan.table = None, rec
    return plan


class SGD(_MultiTensorOptimizer):
    """``torch.optim.SGD`` (momentum, weight decay; dampening 0, no Nesterov) on the library's multi-tensor step."""
    _ALGO = _lib.OPTIM_SGD

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False):
        defaults = dict(torch.optim.SGD([torch.zeros(1)], lr=0.1).defaults)  # torch's keys, whatever its version
        defaults.update(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize)
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"invalid lr / momentum / weight_decay: {lr} / {momentum} / {weight_decay}")
        self._refuse(defaults)
        super().__init__(params, defaults)

    def _refuse(self, group):
        if group["nesterov"]:
            raise NotImplementedError("nesterov=True is not supported by openseg3d_amd.optim.SGD")
        if group["dampening"] != 0:
            raise NotImplementedError("dampening != 0 is not supported by openseg3d_amd.optim.SGD")
        if group.get("maximize"):
            raise NotImplementedError("maximize=True is not supported by openseg3d_amd.optim.SGD")

    def _collect(self, gi, group, p):
        s0, flags = 0, 0
        if group["momentum"] != 0:
            state = self.state[p]
            buf = state.get("momentum_buffer")
            if buf is None:
                # zeros, not empty: should this step die after here (out of memory, say), the next one finds the buffer,
                # raises no first-step flag and computes mu * 0 + g' -- the same values
                buf = state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                flags = _lib.OPTIM_FIRST_STEP
            elif not buf.is_contiguous():
                buf = state["momentum_buffer"] = buf.contiguous()
            s0 = buf.data_ptr()
        return s0, 0, flags, gi

    def _scalars(self, group, key):
        return sgd_scalars(group["lr"], group["weight_decay"], group["momentum"])


class AdamW(_MultiTensorOptimizer):
    """``torch.optim.AdamW`` (decoupled weight decay, no amsgrad) on the library's multi-tensor step.  ``state['step']`` is a
    float32 scalar on the CPU, as in torch's default path: the bias corrections are host arithmetic."""
    _ALGO = _lib.OPTIM_ADAMW

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False):
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid lr / betas / eps / weight_decay: {lr} / {betas} / {eps} / {weight_decay}")
        self._refuse(defaults)
        super().__init__(params, defaults)

    def _refuse(self, group):
        if group["amsgrad"]:
            raise NotImplementedError("amsgrad=True is not supported by openseg3d_amd.optim.AdamW")
        if group.get("maximize"):
            raise NotImplementedError("maximize=True is not supported by openseg3d_amd.optim.AdamW")

    def _collect(self, gi, group, p):
        state = self.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        step_t = state["step"]
        if not step_t.is_cpu:  # loaded from a fused / capturable torch optimizer: one read-back, then host-side
            step_t = state["step"] = step_t.to("cpu", torch.float32)
        step = float(step_t) + 1.0
        self._stepped.append(step_t)
        m, v = state["exp_avg"], state["exp_avg_sq"]
        if not m.is_contiguous():
            m = state["exp_avg"] = m.contiguous()
        if not v.is_contiguous():
            v = state["exp_avg_sq"] = v.contiguous()
        return m.data_ptr(), v.data_ptr(), 0, (gi, step)

    def _scalars(self, group, key):
        return adamw_scalars(group["lr"], group["betas"], group["eps"], group["weight_decay"], key[1])

    def _begin(self):
        self._stepped = []  # the step counters of the parameters this step updates

    def _collected(self):
        if self._stepped:
            torch._foreach_add_(self._stepped, 1.0)
        self._stepped = []


class WarmupPolyLR(LRScheduler):
    """The reference's default schedule (seg3d/models/optimizers/lr_scheduler.py:38-83), stepped per iteration:
    lr = base_lr * warmup(it) * (1 - it / max_iters) ** power, where warmup rises from ``warmup_factor`` to 1 over the first
    ``warmup_iters`` iterations ('linear') or stays at ``warmup_factor`` ('constant'); after the warm-up, with
    ``constant_ending`` > 0, the lr never falls below base_lr * constant_ending."""

    def __init__(self, optimizer, max_iters, warmup_factor=0.001, warmup_iters=1000, warmup_method="linear", last_epoch=-1,
                 power=0.9, constant_ending=0.0):
        if warmup_method not in ("linear", "constant"):
            raise ValueError(f"Unknown warmup method: {warmup_method}")
        self.max_iters = max_iters
        self.warmup_factor = warmup_factor
        self.warmup_iters = warmup_iters
        self.warmup_method = warmup_method
        self.power = power
        self.constant_ending = constant_ending
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        it = self.last_epoch
        poly = math.pow(1.0 - it / self.max_iters, self.power)
        if it < self.warmup_iters:
            ramp = self.warmup_factor
            if self.warmup_method == "linear":
                alpha = it / self.warmup_iters
                ramp = self.warmup_factor * (1 - alpha) + alpha
            return [base * ramp * poly for base in self.base_lrs]
        if self.constant_ending > 0 and poly < self.constant_ending:
            return [base * self.constant_ending for base in self.base_lrs]
        return [base * 1.0 * poly for base in self.base_lrs]


def build_optimizer(cfg, model):
    """builder.py:43-54 with this module's classes: TRAIN.OPTIMIZER = adamw | sgd."""
    if cfg.TRAIN.OPTIMIZER == "adamw":
        return AdamW(model.parameters(), lr=cfg.TRAIN.LR, weight_decay=cfg.TRAIN.WEIGHT_DECAY)
    if cfg.TRAIN.OPTIMIZER == "sgd":
        return SGD(model.parameters(), lr=cfg.TRAIN.LR, weight_decay=cfg.TRAIN.WEIGHT_DECAY, momentum=cfg.TRAIN.MOMENTUM)
    raise NotImplementedError(f"TRAIN.OPTIMIZER = {cfg.TRAIN.OPTIMIZER!r}")


def build_scheduler(cfg, optimizer, epochs, iters_per_epoch):
    """builder.py:57-67: TRAIN.LR_SCHEDULER = cosine_annealing | warmup_poly_lr | one_cycle, stepped once per iteration."""
    if cfg.TRAIN.LR_SCHEDULER == "cosine_annealing":
        return CosineAnnealingLR(optimizer, T_max=epochs * iters_per_epoch)
    if cfg.TRAIN.LR_SCHEDULER == "warmup_poly_lr":
        return WarmupPolyLR(optimizer, max_iters=epochs * iters_per_epoch, warmup_iters=iters_per_epoch)
    if cfg.TRAIN.LR_SCHEDULER == "one_cycle":
        return OneCycleLR(optimizer, max_lr=cfg.TRAIN.LR, total_steps=epochs * iters_per_epoch)
    raise NotImplementedError(f"TRAIN.LR_SCHEDULER = {cfg.TRAIN.LR_SCHEDULER!r}")
