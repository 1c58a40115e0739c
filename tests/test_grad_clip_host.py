"""Gradient-norm clipping without a GPU: the host twins seg3d_grad_norm_host / seg3d_grad_scale_host through
optim.GradClipper / clip_grad_norm_ / grad_norm on CPU parameters against the exact norm (tests/grad_clip_ref.py: within
1 float32 ulp, everything else bit for bit), and the argument checks of all five C entries, which return before a launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import grad_clip_ref as G
from openseg3d_amd import _lib, optim

CPU = torch.device("cpu")


def block():
    return int(_lib.load().seg3d_optim_block_elems())


@pytest.mark.parametrize("pattern", G.PATTERNS_FINITE)
def test_norm_coefficient_and_scale(pattern):
    G.check_finite_pattern(block(), CPU, pattern, G.reference(block(), pattern))


def test_what_float32_accumulation_would_give():
    """The patterns do tell fp64 accumulation from fp32: the squares of `huge` overflow float32 (torch's own norm is inf),
    those of `tiny` underflow it; the exact norms are 7.07e26 and 1e-30 * sqrt(n)."""
    b = block()
    huge, tiny = G.values(b, "huge"), G.values(b, "tiny")
    params = [torch.zeros(g.numel(), requires_grad=True) for g in huge]
    for p, g in zip(params, huge):
        p.grad = g.clone()
    got = float(optim.grad_norm(params))
    assert math.isfinite(got) and abs(got / (1e25 * math.sqrt(5000)) - 1) < 1e-6
    assert math.isinf(float(torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=False)))  # (last: it ruins the gradients)
    n = sum(g.numel() for g in tiny) + b + 1
    assert abs(float(G.reference(b, "tiny")) / (1e-30 * math.sqrt(n)) - 1) < 1e-6


def test_zero_gradients():
    G.check_zeros(block(), CPU)


@pytest.mark.parametrize("pattern", ["inf", "nan"])
def test_nonfinite_gradients_follow_torch(pattern):
    G.check_nonfinite(block(), CPU, pattern)


def test_grad_norm_writes_nothing_and_no_gradient_means_zero():
    b = block()
    case = G.Case(b, CPU, G.values(b, "noise"))
    norm = optim.grad_norm(case.params)
    assert G.ulps(norm, G.reference(b, "noise")) <= 1.0
    assert all(G.same_bits(x, y) for x, y in zip(case.grads(), case.start))
    none = [torch.ones(3, requires_grad=True), torch.ones(5, requires_grad=True)]
    clipper = optim.GradClipper(none, 1.0)
    assert float(clipper()) == 0.0 and float(clipper.last_coef) == 1.0
    assert float(optim.clip_grad_norm_(none[0], 1.0)) == 0.0  # a single tensor, as in torch
    empty = torch.zeros(0, requires_grad=True)
    empty.grad = torch.zeros(0)
    clipper = optim.GradClipper([empty], 0.0)
    assert float(clipper()) == 0.0 and float(clipper.last_coef) == 1.0


@pytest.mark.parametrize("cls", [optim.SGD, optim.AdamW])
def test_optimizer_method_clips_its_own_groups(cls):
    b = block()
    start = G.values(b, "noise")[:8]
    params = [torch.zeros(g.numel(), requires_grad=True) for g in start]
    for p, g in zip(params, start):
        p.grad = g.clone()
    opt = cls([dict(params=params[:3]), dict(params=params[3:], lr=0.01)], lr=0.1)
    ref = G.exact_norm(start)
    norm = opt.clip_grad_norm_(float(ref) / 2)
    assert G.ulps(norm, ref) <= 1.0
    coef = opt._clipper.last_coef
    assert float(coef) < 1.0
    assert all(G.same_bits(p.grad, g * coef) for p, g in zip(params, start))
    table = opt._clipper._plan.table
    opt.clip_grad_norm_(float(ref))  # the same addresses: the table is kept
    assert opt._clipper._plan.table is table
    opt.step()
    assert all(not torch.equal(p.detach(), torch.zeros_like(p)) for p in params if p.numel())


def test_refusals():
    p = torch.zeros(4, requires_grad=True)
    p.grad = torch.ones(4)
    for norm_type in (1, 1.0, float("inf")):
        with pytest.raises(NotImplementedError, match=repr(norm_type).replace(".", r"\.")):
            optim.clip_grad_norm_([p], 1.0, norm_type=norm_type)
    assert float(optim.clip_grad_norm_([p], 10.0, norm_type=2, foreach=True)) == 2.0  # foreach: accepted and ignored
    with pytest.raises(ValueError, match="max_norm"):
        optim.clip_grad_norm_([p], -1.0)
    with pytest.raises(ValueError, match="max_norm"):
        optim.GradClipper([p], float("nan"))
    d = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    d.grad = torch.ones(4, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float32"):
        optim.clip_grad_norm_([p, d], 1.0)
    s = torch.zeros(4, requires_grad=True)
    s.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (4,))
    with pytest.raises(NotImplementedError, match="sparse"):
        optim.clip_grad_norm_([p, s], 1.0)
    t = torch.zeros(3, 4, requires_grad=True)
    t.grad = torch.ones(4, 3).t()
    with pytest.raises(NotImplementedError, match="non-contiguous gradients"):
        optim.clip_grad_norm_([p, t], 1.0)
    m = torch.zeros(4, device="meta", requires_grad=True)
    m.grad = torch.zeros(4, device="meta")
    with pytest.raises(NotImplementedError, match="one device.*cpu.*meta"):
        optim.clip_grad_norm_([p, m], 1.0)
    assert torch.equal(p.grad, torch.ones(4))  # nothing was scaled by a refused call


def records(entries):
    """host records of (array, count, first_block)"""
    rec = np.zeros((len(entries),), dtype=optim._RECORD)
    for i, (a, n, first) in enumerate(entries):
        rec[i]["param"], rec[i]["count"], rec[i]["first_block"] = (a.ctypes.data if a is not None else 0), n, first
    return rec


def test_argument_validation_of_the_c_entries():
    lib, b = _lib.load(), block()
    fake, inf = ctypes.c_void_p(256), float("inf")
    assert _lib.query("seg3d_grad_norm_workspace_bytes", 0) == 0
    assert _lib.query("seg3d_grad_norm_workspace_bytes", 301) == 301 * 8
    # the device entries: every case returns before a launch (the non-null addresses are never read)
    norm, scale = lib.seg3d_grad_norm, lib.seg3d_grad_scale
    assert norm(None, 1, 1, 1.0, fake, 8, fake, None) == _lib.EINVAL          # NULL table with n_tensors > 0
    assert norm(fake, 1, 1, 1.0, fake, 8, None, None) == _lib.EINVAL          # NULL result
    assert norm(fake, -1, 1, 1.0, fake, 8, fake, None) == _lib.EINVAL
    for blocks in (-1, 1 << 31):
        assert norm(fake, 1, blocks, 1.0, fake, 1 << 40, fake, None) == _lib.EINVAL
        assert scale(fake, 1, blocks, fake, None) == _lib.EINVAL
    for bad in (-1.0, -inf, float("nan")):
        assert norm(fake, 1, 1, bad, fake, 8, fake, None) == _lib.EINVAL
    assert norm(fake, 1, 1, 1.0, None, 8, fake, None) == _lib.EINVAL          # NULL workspace
    assert norm(fake, 3, 10, 1.0, fake, 79, fake, None) == _lib.EWORKSPACE    # one byte short
    assert norm(fake, 3, 10, inf, fake, 0, fake, None) == _lib.EWORKSPACE
    assert scale(None, 1, 1, fake, None) == _lib.EINVAL
    assert scale(fake, 1, 1, None, None) == _lib.EINVAL
    assert scale(None, 0, 0, fake, None) == 0                                 # nothing to do, nothing launched
    # the host entries: the same, and every record
    hnorm, hscale = lib.seg3d_grad_norm_host, lib.seg3d_grad_scale_host
    res = np.full((2,), -7.0, np.float32)
    rp, cp = ctypes.c_void_p(res.ctypes.data), ctypes.c_void_p(res.ctypes.data + 4)
    a, c = np.full((b + 1,), 2.0, np.float32), np.full((3,), 1.0, np.float32)
    good = records([(a, b + 1, 0), (None, 0, 2), (c, 3, 2)])
    bad_tables = {
        "null array": records([(a, b + 1, 0), (None, 3, 2)]),
        "negative count": records([(a, b + 1, 0), (c, -3, 2)]),
        "first_block out of order": records([(a, b + 1, 0), (c, 3, 1)]),
        "first_block not from 0": records([(a, b + 1, 1), (c, 3, 3)]),
    }
    for name, rec in bad_tables.items():
        tp = ctypes.c_void_p(rec.ctypes.data)
        assert hnorm(tp, len(rec), 3, 1.0, rp) == _lib.EINVAL, name
        assert hscale(tp, len(rec), 3, cp) == _lib.EINVAL, name
    tp = ctypes.c_void_p(good.ctypes.data)
    for blocks in (2, 4, -1, 1 << 31):                                       # a wrong sum of blocks
        assert hnorm(tp, 3, blocks, 1.0, rp) == _lib.EINVAL
        assert hscale(tp, 3, blocks, cp) == _lib.EINVAL
    assert hnorm(None, 3, 3, 1.0, rp) == _lib.EINVAL and hnorm(tp, 3, 3, 1.0, None) == _lib.EINVAL
    assert hscale(None, 3, 3, cp) == _lib.EINVAL and hscale(tp, 3, 3, None) == _lib.EINVAL
    for bad in (-1.0, float("nan")):
        assert hnorm(tp, 3, 3, bad, rp) == _lib.EINVAL
    assert res.tolist() == [-7.0, -7.0] and (a == 2.0).all()                  # a refused call writes nothing
    assert hnorm(None, 0, 0, 0.0, rp) == 0 and res.tolist() == [0.0, 1.0]     # nothing to sum: norm 0, coefficient 1
    assert hnorm(tp, 3, 3, 1.0, rp) == 0
    want = np.float32(math.sqrt(4.0 * (b + 1) + 3.0))
    assert res[0] == want and res[1] == np.float32(1.0) / (want + np.float32(1e-6))
    assert hscale(tp, 3, 3, cp) == 0
    assert (a == np.float32(2.0) * res[1]).all() and (c == res[1]).all()
    assert hnorm(tp, 3, 3, inf, rp) == 0 and res[1] == 1.0                    # max_norm = +inf: the norm alone
    before = a.copy()
    assert hscale(tp, 3, 3, cp) == 0 and np.array_equal(a, before)
