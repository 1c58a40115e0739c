"""One rank of tests/test_gpu_norms_range.py::test_sync_batchnorm_cases_on_three_ranks (started by dist.launch_local_ranks;
all ranks share cuda:0 over gloo).  One process group, many cases of ops.batch_norm_act on a SyncBatchNorm: every rank
checks its slice against tests/norm_ref.py's float64 BatchNorm over the rows of all ranks, with the tolerances of
tests/_syncbn_rank.py."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import norm_ref  # noqa: E402
from openseg3d_amd import dist as D, ops  # noqa: E402

EPS = 1e-3
DEV = torch.device("cuda:0")


def close(what, a, b, tol):
    a = a.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if b.numel() == 0:
        return
    err = float((a - b).abs().max())
    assert err <= tol * max(1.0, float(b.abs().max())), (what, err, tol)


def same_on_all_ranks(what, t, world):
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t.contiguous())
    for p in parts[1:]:
        assert torch.equal(parts[0], p), what


def run_case(rank, world, rows, c, relu, with_res, momentum, passes, seed):
    gen = torch.Generator().manual_seed(seed)  # the same on every rank: each builds all blocks and keeps its own
    xs = [torch.randn(n, c, generator=gen) * (1.0 + 0.5 * r) + 0.3 * r for r, n in enumerate(rows)]
    rs = [torch.randn(n, c, generator=gen) for n in rows] if with_res else None
    gs = [torch.randn(n, c, generator=gen) for n in rows]
    gamma, beta = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen)
    bn = torch.nn.SyncBatchNorm(c, eps=EPS, momentum=momentum).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    rm, rv, nbt = torch.zeros(c), torch.ones(c), 0
    what = f"rows {rows} c {c} relu {relu} res {with_res} momentum {momentum}"
    for step in range(passes):
        if step:
            xs = [x * 0.7 + 1.0 for x in xs]
        if relu:  # every pre-activation of the float64 reference at least 2e-3 from the kink (asserted at 1e-3 below)
            for _ in range(10):
                pres = norm_ref.batch_norm_ranks(xs, gamma, beta, EPS, ress=rs).pre
                if not any(bool((p.abs() < 2e-3).any()) for p in pres):
                    break
                for x, p in zip(xs, pres):
                    x[p.abs() < 2e-3] += 0.05
        ref = norm_ref.batch_norm_ranks(xs, gamma, beta, EPS, ress=rs, relu=relu, dys=gs)
        if relu:
            assert min(float(p.abs().min()) for p in ref.pre if p.numel()) > 1e-3, what
        full = norm_ref.batch_norm(torch.cat(xs), gamma, beta, EPS, running_mean=rm, running_var=rv, momentum=momentum,
                                   num_batches_tracked=nbt)
        rm, rv, nbt = full.running_mean, full.running_var, full.num_batches_tracked

        bn.zero_grad()
        x = xs[rank].to(DEV).requires_grad_()
        res = rs[rank].to(DEV).requires_grad_() if with_res else None
        y = ops.batch_norm_act(x, bn, relu=relu, res=res)
        assert "SyncBatchNormAct" in type(y.grad_fn).__name__, (what, type(y.grad_fn).__name__)
        (y * gs[rank].to(DEV)).sum().backward()
        assert y.shape == (rows[rank], c) and x.grad.shape == (rows[rank], c), what
        close(what + " y", y, ref.y[rank], 1e-5)
        close(what + " dx", x.grad, ref.dx[rank], 1e-5)
        if with_res:
            close(what + " dres", res.grad, ref.dres[rank], 1e-6)
        close(what + " running_mean", bn.running_mean, rm, 1e-6)
        close(what + " running_var", bn.running_var, rv, 1e-6)
        assert int(bn.num_batches_tracked) == nbt, what
        same_on_all_ranks(what + " running_mean", bn.running_mean, world)
        same_on_all_ranks(what + " running_var", bn.running_var, world)
        # parameter gradients stay rank-local (DDP averages them): this rank's share, and their sum over the ranks
        close(what + " dgamma local", bn.weight.grad, ref.dgamma_local[rank], 1e-5)
        close(what + " dbeta local", bn.bias.grad, ref.dbeta_local[rank], 1e-5)
        if rows[rank] == 0:
            assert y.numel() == 0 and x.grad.numel() == 0, what
            assert float(bn.weight.grad.abs().max()) == 0.0 and float(bn.bias.grad.abs().max()) == 0.0, what
        gw, gb = bn.weight.grad.clone(), bn.bias.grad.clone()
        dist.all_reduce(gw)
        dist.all_reduce(gb)
        close(what + " dgamma", gw, ref.dgamma, 1e-5)
        close(what + " dbeta", gb, ref.dbeta, 1e-5)


def main():
    rank, world, _ = D.init_job(backend="gloo", share_device=True)
    assert world == 3
    n = 0
    for rows in ([0, 1, 470], [300, 470, 640]):
        for c in (64, 256):
            for relu in (True, False):
                for with_res in (True, False):
                    run_case(rank, world, rows, c, relu, with_res, 0.01, 1, seed=100 + n)
                    n += 1
    run_case(rank, world, [300, 470, 640], 64, True, True, None, 2, seed=7)  # cumulative average over two passes
    run_case(rank, world, [0, 1, 470], 64, False, False, None, 2, seed=8)
    n += 2
    D.job_barrier(DEV)
    if rank == 0:
        print(f"SYNCBN CASES OK ({n} cases)", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
