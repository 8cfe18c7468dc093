"""Sharded training on the CPU: two and three gloo ranks run the product's own code -- ``parallel.global_moments`` (per-shard float64
moments, one all-gather, Chan's update), the sharded ``BaseOCLoss.compute_loss`` / ``training.kl_weights`` and ``parallel.all_reduce_grads``
-- and must reproduce the single-process value and gradient on the concatenated batch.

Bounds.  Moments: n exactly; mean and variance to 1e-9 relative of torch's float64 ``mean()`` / ``var()`` of the concatenated kept
values.  On the hard case (float32 values 1e4 + 1e-2 randn) the Chan combination is off by ~1e-12, a float64 sum / sum-of-squares
formulation by ~1e-4 and a float32 ``var()`` by ~8e-4: 1e-9 tells them apart (``test_the_bound_discriminates`` holds that here).
Gradient algebra: ``rnd`` is a float64 leaf; its gradient gathered over the ranks equals autograd's gradient of the single-process
expression to 1e-12."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from sde_sampler_lrds_amd import parallel
from sde_sampler_lrds_amd.losses import oc
from sde_sampler_lrds_amd.losses import training as T
from tests.sharded_training_worker import CountingDist

WORLDS = (2, 3)
TPS = 4  # traj_per_sample of the lv_traj case


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def moment_cases(world):
    """name -> (rnd [total,1], mask): every rank (and the parent) rebuilds the global batch from the seed."""
    cases = {}
    for total in (1000, 1001):
        g = torch.Generator().manual_seed(total)
        rnd = 3.0 * torch.randn(total, 1, generator=g) + 5.0
        cases[f"easy_{total}"] = (rnd, rnd < 9.0)
    g = torch.Generator().manual_seed(7)
    hard = (1e4 + 1e-2 * torch.randn(1001, 1, generator=g, dtype=torch.float64)).float()
    cases["hard"] = (hard, torch.ones_like(hard, dtype=torch.bool))
    lo, hi = parallel.shard_bounds(1001, world, 1)  # rank 1 keeps nothing
    row = torch.arange(1001).view(-1, 1)
    cases["hard_one_rank_empty"] = (hard, (row < lo) | (row >= hi))
    return cases


def grad_batch():
    """The float64 batch of the gradient-algebra cases: 251 samples x TPS trajectories, filter rnd < 9."""
    g = torch.Generator().manual_seed(11)
    return 3.0 * torch.randn(TPS * 251, 1, generator=g, dtype=torch.float64) + 5.0


def make_loss(method, dist_=None):
    loss = oc.BaseOCLoss(None, None, method=method, traj_per_sample=TPS if method == "lv_traj" else 1, max_rnd=9.0)
    loss.dist = dist_
    return loss


def shard_rows(rnd_all, method, world, rank):
    """This rank's rows of the global batch; 'lv_traj': whole samples -- all TPS trajectories of a sample on one rank (row j * S + i of
    the single-process batch is trajectory j of sample i)."""
    if method != "lv_traj":
        lo, hi = parallel.shard_bounds(rnd_all.shape[0], world, rank)
        return rnd_all[lo:hi]
    S = rnd_all.shape[0] // TPS
    lo, hi = parallel.shard_bounds(S, world, rank)
    return rnd_all.view(TPS, S, 1)[:, lo:hi].reshape(-1, 1)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {"rank": rank}
    for name, (rnd, mask) in moment_cases(world).items():
        lo, hi = parallel.shard_bounds(rnd.shape[0], world, rank)
        counting = CountingDist(dist)
        out[f"moments/{name}"] = (parallel.global_moments(rnd[lo:hi], mask[lo:hi], counting).tolist(), len(counting.calls))
    rnd_all = grad_batch()
    for method in ("lv", "lv_traj", "kl"):
        counting = CountingDist(dist)
        loss = make_loss(method, counting)
        shard = shard_rows(rnd_all, method, world, rank).clone().requires_grad_(True)
        value, metrics = loss.compute_loss(shard)
        value.backward()
        out[f"grad/{method}"] = (float(value.detach()), shard.grad.clone(), metrics["train/n_filtered_cumulative"], len(counting.calls))
    counting = CountingDist(dist)
    loss = make_loss("kl", counting)
    shard = shard_rows(rnd_all, "kl", world, rank).float()
    mask, w, value = T.kl_weights(loss, shard, None)
    out["kl_weights"] = (float(value), w.clone(), int(mask.sum()), loss.n_filtered, len(counting.calls))
    # all_reduce_grads: a gradient on every rank, one on no rank, one on rank 0 only
    params = [torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(4))]
    params[0].grad = torch.full((3, 2), float(rank + 1)) * torch.arange(6.0).view(3, 2)
    if rank == 0:
        params[2].grad = torch.tensor([1.0, -2.0, 3.0, 0.5])
    counting = CountingDist(dist)
    parallel.all_reduce_grads(params, counting)
    out["all_reduce_grads"] = ([None if p.grad is None else p.grad.clone() for p in params], list(counting.calls))
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


_RUNS = {}


def ranks(world):
    """What every rank of a ``world``-rank gloo run reported (one run per world size, shared by the tests; a failed run fails them all)."""
    if world not in _RUNS:
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        try:
            got = [q.get(timeout=180) for _ in range(world)]
            _RUNS[world] = sorted(got, key=lambda o: o["rank"])
        except Exception as e:  # noqa: BLE001 -- a rank died or timed out: remembered, not retried
            _RUNS[world] = e
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
            if p.exitcode != 0 and not isinstance(_RUNS[world], Exception):
                _RUNS[world] = RuntimeError(f"rank exited with {p.exitcode}")
    if isinstance(_RUNS[world], Exception):
        raise _RUNS[world]
    return _RUNS[world]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", ["easy_1000", "easy_1001", "hard", "hard_one_rank_empty"])
def test_global_moments_match_float64_torch(world, name):
    rnd, mask = moment_cases(world)[name]
    kept = rnd[mask].double()
    got = [r[f"moments/{name}"] for r in ranks(world)]
    assert all(g == got[0] for g in got), "ranks disagree"
    (n, mean, m2, rows), calls = got[0]
    assert calls == 1
    assert n == kept.numel() and rows == rnd.shape[0]
    e_mean = abs(mean - float(kept.mean())) / abs(float(kept.mean()))
    e_var = abs(m2 / (n - 1) - float(kept.var())) / float(kept.var())
    print(f"world {world} {name}: n {int(n)} of {int(rows)}, mean rel. error {e_mean:.1e}, variance rel. error {e_var:.1e}")
    assert e_mean < 1e-9 and e_var < 1e-9


def test_the_bound_discriminates():
    """On the hard case a float64 sum / sum-of-squares combination and a float32 var() both miss 1e-9 by orders of magnitude."""
    rnd, _ = moment_cases(2)["hard"]
    x = rnd.double().reshape(-1)
    ref = float(x.var())
    n = x.numel()
    naive = float((x * x).sum() - x.sum() ** 2 / n) / (n - 1)
    e_naive, e_f32 = abs(naive - ref) / ref, abs(float(rnd.var()) - ref) / ref
    print(f"hard case: float64 sum-of-squares off by {e_naive:.1e}, float32 var() by {e_f32:.1e}")
    assert e_naive > 1e-6 and e_f32 > 1e-6


def test_combine_moments_handles_empty_and_tiny_batches():
    x = torch.tensor([[1.0], [4.0]])
    keep = torch.ones(2, 1, dtype=torch.bool)
    empty = parallel.shard_moments(x[:0], keep[:0])
    assert empty.tolist() == [0.0, 0.0, 0.0, 0.0]
    assert parallel.shard_moments(x, ~keep).tolist() == [0.0, 0.0, 0.0, 2.0]
    both = parallel.combine_moments(torch.stack([empty, parallel.shard_moments(x[:1], keep[:1]), empty, parallel.shard_moments(x[1:], keep[1:])]))
    assert both.tolist() == [2.0, 2.5, 4.5, 2.0] and float(parallel.unbiased_var(both)) == 4.5
    # n <= 1: NaN, as torch.var
    assert torch.isnan(parallel.unbiased_var(parallel.shard_moments(x[:1], keep[:1]))) and torch.isnan(parallel.unbiased_var(empty))
    # entries the mask drops may be non-finite
    bad = torch.tensor([[float("inf")], [2.0], [float("nan")], [6.0]])
    assert parallel.shard_moments(bad, bad.isfinite()).tolist() == [2.0, 4.0, 8.0, 4.0]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("method", ["lv", "lv_traj", "kl"])
def test_sharded_value_and_gradient_equal_the_single_process_expression(world, method):
    rnd_all = grad_batch().requires_grad_(True)
    single = make_loss(method)
    value, metrics = single.compute_loss(rnd_all)
    value.backward()
    value = value.detach()
    got = [r[f"grad/{method}"] for r in ranks(world)]
    assert all(g[0] == got[0][0] for g in got), "the value differs between ranks"
    assert all(g[2] == metrics["train/n_filtered_cumulative"] for g in got), "n_filtered is not the global count on every rank"
    assert all(g[3] == 1 for g in got), "one collective per training value"
    shards = [g[1] for g in got]
    if method == "lv_traj":
        S = rnd_all.shape[0] // TPS
        gathered = torch.cat([s.view(TPS, -1, 1) for s in shards], dim=1).reshape(-1, 1)
        assert gathered.shape[0] == TPS * S
    else:
        gathered = torch.cat(shards)
    e_val, e_grad = abs(got[0][0] - float(value)), float((gathered - rnd_all.grad).abs().max())
    print(f"world {world} {method}: value {got[0][0]:.12f} (off by {e_val:.1e}), gradient off by {e_grad:.1e} (largest entry {float(rnd_all.grad.abs().max()):.1e})")
    assert e_val < 1e-12 * max(1.0, abs(float(value))) and e_grad < 1e-12


@pytest.mark.parametrize("world", WORLDS)
def test_kl_weights_divide_by_the_global_count(world):
    rnd_all = grad_batch().float()
    single = make_loss("kl")
    mask, w, value = T.kl_weights(single, rnd_all, None)
    got = [r["kl_weights"] for r in ranks(world)]
    assert all(g[0] == got[0][0] for g in got)
    assert sum(g[2] for g in got) == int(mask.sum()) and all(g[3] == single.n_filtered for g in got) and all(g[4] == 1 for g in got)
    assert torch.equal(torch.cat([g[1] for g in got]), w)  # mask / n with the same n: the same float32 quotient
    assert abs(got[0][0] - float(value)) < 1e-6 * abs(float(value))  # (the single-process mean is a float32 reduction)


@pytest.mark.parametrize("world", WORLDS)
def test_all_reduce_grads_sums_with_one_collective(world):
    for r in ranks(world):
        grads, calls = r["all_reduce_grads"]
        assert calls == ["all_reduce"]
        total = sum(range(1, world + 1))
        assert torch.equal(grads[0], float(total) * torch.arange(6.0).view(3, 2))
        assert grads[1] is None  # no rank had one
        assert torch.equal(grads[2], torch.tensor([1.0, -2.0, 3.0, 0.5]))  # rank 0's, zeros from the others


class _OneRank:
    """A process group of world size 1: any collective is an error."""

    @staticmethod
    def is_initialized():
        return True

    @staticmethod
    def get_world_size():
        return 1

    def __getattr__(self, name):
        raise AssertionError(f"dist.{name} used in a single-rank run")


@pytest.mark.parametrize("method", ["lv", "lv_traj", "kl"])
def test_without_a_process_group_the_value_is_todays(method):
    rnd = grad_batch().float()
    values = []
    for d in (None, _OneRank()):
        loss = make_loss(method, d)
        x = rnd.clone().requires_grad_(True)
        value, metrics = loss.compute_loss(x)
        value.backward()
        values.append((value.detach(), x.grad, metrics["train/n_filtered_cumulative"]))
    # today's expression, spelled out
    if method == "lv_traj":
        r = rnd.reshape(TPS, -1, 1)
        want = r[:, (r < 9.0).all(dim=0)].var(dim=0).mean()
    else:
        want = rnd[rnd < 9.0].var() if method == "lv" else rnd[rnd < 9.0].mean()
    assert torch.equal(values[0][0], want) and torch.equal(values[1][0], want)
    assert torch.equal(values[0][1], values[1][1]) and values[0][2] == values[1][2]
    p = torch.nn.Parameter(torch.ones(2))
    p.grad = torch.tensor([1.0, 2.0])
    parallel.all_reduce_grads([p], None)
    parallel.all_reduce_grads([p], _OneRank())
    assert torch.equal(p.grad, torch.tensor([1.0, 2.0]))
