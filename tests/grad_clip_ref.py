"""Shared by tests/test_grad_clip_host.py and tests/test_gpu_grad_clip.py: the gradient sets at which the clipping entries
(seg3d_grad_norm / seg3d_grad_scale and their host twins) can go wrong, the exact norm, and the checks both sides run.

The exact norm is sqrt(math.fsum(float(x) * float(x) for every element)) rounded to float32.  A sum in fp64 of n
non-negative terms in any order is within (n - 1) * 2^-53 relative of exact -- 1.4e-10 for the 1.3 M elements here, far
below half a float32 ulp (3e-8) -- so an fp64 accumulation lands within 1 float32 ulp of the rounded exact norm; a larger gap
means the accumulation is not fp64.  Everything else is compared bit for bit."""
import functools
import itertools
import math

import numpy as np
import torch

import optim_ref as R
from openseg3d_amd import optim

PATTERNS_FINITE = ["noise", "huge", "tiny"]


def exact_norm(grads):
    """float32(sqrt(fsum of the squares)) of a list of float32 tensors; the squares are exact in float64."""
    lists = ((g.detach().cpu().double().flatten() ** 2).tolist() for g in grads if g is not None)
    return np.float32(math.sqrt(math.fsum(itertools.chain.from_iterable(lists))))


def ulps(got, ref32):
    """|got - ref| in float32 ulps of the reference"""
    return R.ulp_error(torch.as_tensor(got).reshape(1).float(), torch.tensor([float(ref32)], dtype=torch.float64))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def shapes(block):
    """optim_ref's sizes (1 ... 2 * block + 7, and an empty tensor), then 300 * block + 5 elements: more than 256 partials,
    so the second launch strides."""
    return list(R.sizes(block)) + [300 * block + 5]


def values(block, pattern, seed=0):
    """One float32 CPU gradient per shape.
    noise: normal, a per-tensor scale from 1e-3 to 1e3;  huge: the same with 5000 entries of 1e25 (their squares overflow
    float32, the norm 7.07e26 does not);  tiny: only 1e-30 (the squares underflow float32);  zeros;  inf / nan: noise with
    one such entry."""
    gen = torch.Generator().manual_seed(seed)
    ns = shapes(block)
    scales = np.logspace(-3, 3, len(ns))
    out = []
    for n, s in zip(ns, scales):
        if pattern == "tiny":
            out.append(torch.full((n,), 1e-30))
        elif pattern == "zeros":
            out.append(torch.zeros(n))
        else:
            out.append(torch.randn(n, generator=gen) * float(s))
    if pattern == "huge":
        out[-1][100:5100] = 1e25
    elif pattern == "inf":
        out[-1][block + 3] = float("inf")
    elif pattern == "nan":
        out[ns.index(65)][5] = float("nan")
    return out


@functools.lru_cache(maxsize=None)
def reference(block, pattern):
    """The exact norm of a Case over `values(block, pattern)` (the view's copy counts too): computed once per process."""
    g = values(block, pattern)
    return exact_norm(g + [g[R.sizes(block).index(block + 1)]])


SENTINEL = 7.0


class Case:
    """Parameters on `device` with the gradients of `values`, plus: [-2] a copy of the (block + 1)-element gradient that is
    a view at element offset 1 of a larger buffer (4-byte aligned: the element path), [-1] a parameter without a gradient."""

    def __init__(self, block, device, grads):
        self.block, self.device = block, device
        i_view = R.sizes(block).index(block + 1)
        self.start = [g.clone() for g in grads] + [grads[i_view].clone()]
        self.src = [g.to(device) for g in self.start]  # set_grads and restore copy on the device: nothing synchronises
        self.params = [torch.zeros(g.numel(), device=device, requires_grad=True) for g in self.start]
        self.params.append(torch.ones(7, device=device, requires_grad=True))
        self.i_view = len(self.start) - 1
        self.buf = None
        self.set_grads()

    def set_grads(self):
        for i, (p, g) in enumerate(zip(self.params, self.src)):
            if i == self.i_view:
                self.buf = torch.full((g.numel() + 5,), SENTINEL, device=self.device)
                self.buf[1:1 + g.numel()].copy_(g)
                p.grad = self.buf[1:1 + g.numel()]
                assert p.grad.data_ptr() % 16 == 4
            else:
                p.grad = g.clone()
        assert self.params[-1].grad is None

    def restore(self):
        """the starting values again, at the same addresses"""
        for p, g in zip(self.params, self.src):
            p.grad.copy_(g)

    def grads(self):
        return [p.grad.detach().cpu().clone() for p in self.params[:-1]]

    def view_surroundings_untouched(self):
        n = self.start[self.i_view].numel()
        b = self.buf.cpu()
        return bool((b[:1] == SENTINEL).all() and (b[1 + n:] == SENTINEL).all())


def expected_coef(max_norm, norm_written):
    """min(float32(max_norm) / (norm + float32(1e-6)), 1) in numpy float32, from the norm the library wrote"""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm_written) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else c


def check_finite_pattern(block, device, pattern, ref32):
    """Assertions 1 - 4 and 6 of one finite pattern: norm accuracy; the coefficient, the scaled gradients and the
    untouched ones bit for bit, for one max_norm below and one above the norm; the same two floats on a second call."""
    case = Case(block, device, values(block, pattern))
    ref = float(ref32)
    assert math.isfinite(ref) and ref > 0
    # (above: torch's coefficient is max_norm / (norm + 1e-6), which exceeds 1 for every norm once max_norm > norm + 1e-6)
    for max_norm in (ref * 0.5, ref * 2.0 + 1.0):
        case.restore()
        before = case.grads()
        clipper = optim.GradClipper(case.params, max_norm)
        norm = clipper()
        assert norm.shape == () and norm.dtype == torch.float32 and norm.device.type == device.type
        err = ulps(norm.cpu(), ref32)
        print(f"{pattern} on {device.type}: norm {float(norm)!r}, exact {ref!r}, {err} ulp")
        assert err <= 1.0, (pattern, float(norm), ref, err)
        coef = clipper.last_coef.cpu()
        want = expected_coef(max_norm, norm.cpu().numpy())
        assert coef.numpy().view(np.int32) == want.view(np.int32), (pattern, max_norm, float(coef), float(want))
        assert (float(coef) < 1.0) == (max_norm < ref)
        after = case.grads()
        for i, (a, b) in enumerate(zip(after, before)):
            assert same_bits(a, b * coef), (pattern, max_norm, i)
            if max_norm > ref:
                assert same_bits(a, b), (pattern, i)
        assert case.view_surroundings_untouched()
        # reproducibility: the same gradients at the same addresses, the same two floats
        case.restore()
        again = clipper()
        assert same_bits(again, norm) and same_bits(clipper.last_coef, coef)
    assert torch.equal(case.params[-1].detach().cpu(), torch.ones(7)) and case.params[-1].grad is None


def check_zeros(block, device):
    case = Case(block, device, values(block, "zeros"))
    clipper = optim.GradClipper(case.params, 1.0)
    norm = clipper()
    assert float(norm) == 0.0 and float(clipper.last_coef) == 1.0
    assert all(same_bits(a, b) for a, b in zip(case.grads(), case.start))
    assert case.view_surroundings_untouched()
    assert float(optim.grad_norm(case.params)) == 0.0


def classes(t):
    """0 = NaN, 1 = zero, 2 = another finite value, 3 = infinite"""
    return torch.where(t.isnan(), 0, torch.where(t == 0, 1, torch.where(t.isfinite(), 2, 3)))


def check_nonfinite(block, device, pattern):
    """The pattern of NaN, zero and finite values equals what torch.nn.utils.clip_grad_norm_ leaves on CPU copies; with
    error_if_nonfinite=True a RuntimeError and no gradient changed."""
    import pytest
    case = Case(block, device, values(block, pattern))
    theirs = [torch.zeros(g.numel(), requires_grad=True) for g in case.start]
    for p, g in zip(theirs, case.start):
        p.grad = g.clone()
    their_norm = torch.nn.utils.clip_grad_norm_(theirs, 1.0, foreach=False)
    before = case.grads()
    with pytest.raises(RuntimeError, match="non-finite"):
        optim.clip_grad_norm_(case.params, 1.0, error_if_nonfinite=True)
    assert all(same_bits(a, b) for a, b in zip(case.grads(), before))
    norm = optim.clip_grad_norm_(case.params, 1.0)
    assert torch.equal(classes(norm.cpu()), classes(their_norm)), (float(norm), float(their_norm))  # inf or NaN
    for i, (mine, p) in enumerate(zip(case.grads(), theirs)):
        assert torch.equal(classes(mine), classes(p.grad)), (pattern, i)
    if pattern == "inf":  # norm inf, coefficient 0: that entry NaN, the rest 0
        flat = torch.cat(case.grads()[:-1])
        assert int(flat.isnan().sum()) == 1 and int((flat == 0).sum()) == flat.numel() - 1
    else:
        assert all(bool(g.isnan().all()) for g in case.grads())
    assert case.view_surroundings_untouched()
