"""Multi-GPU layer: particles are i.i.d. and never interact before the final estimator, so the batch is
sharded across ranks (one process per GPU) with NO collective inside the step loop.  The only exchange is
for the log-Z / ESS estimators of ``BaseOCLoss.compute_results`` (losses/oc.py:150-161): every rank reduces
its own shard on the device (``sdeng_logz``), the 8-float partial-statistics vectors are all-gathered
(RCCL over xGMI; 32 bytes per rank, latency-bound) and combined with a max-shifted log-sum-exp and Chan's
parallel variance.  Noise is keyed by the global particle index, so results do not depend on the sharding.

Training adds two collectives per step (second half of this file): ``global_moments`` -- the (n, mean, M2) of the log-weights over all
ranks, from which ``BaseOCLoss.compute_loss`` and ``training.kl_weights`` form the global log-variance / KL objective -- and
``all_reduce_grads``, one SUM all-reduce of every parameter gradient (``TrainableDiff.set_distributed``).
"""
from __future__ import annotations

import math

import torch


# Layout of the 8-float statistics vector sdeng_logz writes (include/sdeng.h) -- the ONE definition the kernel's consumers share:
# engine.logz_stats produces it, combine_stats / global_weights consume it, tests/test_gpu_units.py checks the kernel against
# stats_reference() index by index, and the 2-rank gloo test runs this module's own gather / combine code on it.
ELBO, LOGZ, VAR, ESS, MAX, SUM_EXP, SUM_EXP2, SUM = range(8)
N_STATS = 8


def stats_reference(rnd: torch.Tensor) -> torch.Tensor:
    """What sdeng_logz writes for one shard of log-weights ``rnd`` [B,1], restated with torch in fp64 (CPU or GPU).  Not used by the
    product path (``engine.logz_stats`` is): it pins the layout in tests and lets the gloo test run without a GPU."""
    v = -rnd.double().reshape(-1)
    n = v.numel()
    mx = v.max()
    e = torch.exp(v - mx)
    out = torch.empty(N_STATS, dtype=torch.float64)
    out[ELBO] = v.mean()
    out[LOGZ] = mx + e.sum().log() - math.log(n)
    out[VAR] = rnd.double().var() if n > 1 else 0.0
    out[ESS] = e.sum() ** 2 / (e ** 2).sum() / n
    out[MAX], out[SUM_EXP], out[SUM_EXP2], out[SUM] = mx, e.sum(), (e ** 2).sum(), v.sum()
    return out.float()


def shard_bounds(total: int, world: int, rank: int) -> tuple[int, int]:
    """Contiguous particle range [lo, hi) of ``rank`` (first ``total % world`` ranks get one extra)."""
    base, extra = divmod(total, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def combine_stats(stats: torch.Tensor, counts: torch.Tensor) -> dict:
    """stats [W,8] as written by sdeng_logz (include/sdeng.h), counts [W] -> global estimators.
    stats[:,2] = unbiased var(rnd), [:,4] = max(-rnd), [:,5] = sum exp(-rnd-max), [:,6] = sum exp(2(-rnd-max)),
    [:,7] = sum(-rnd)."""
    stats, counts = stats.double().cpu(), counts.double().cpu()
    n = counts.sum()
    gmax = stats[:, MAX].max()
    shift = torch.exp(stats[:, MAX] - gmax)
    se = (stats[:, SUM_EXP] * shift).sum()
    se2 = (stats[:, SUM_EXP2] * shift ** 2).sum()
    total = stats[:, SUM].sum()
    mean = total / n
    local_mean = stats[:, SUM] / counts
    m2 = (stats[:, VAR] * (counts - 1).clamp(min=0)).sum() + (counts * (local_mean - mean) ** 2).sum()
    return {
        "elbo": float(mean),
        "log_norm_const_is": float(gmax + torch.log(se) - math.log(float(n))),
        "lv_loss": float(m2 / (n - 1)) if n > 1 else 0.0,
        "ess": float(se * se / se2 / n),
        "n": int(n), "max_neg_rnd": float(gmax), "sum_exp": float(se),
    }


class PendingResults:
    """Estimators of one pass, still on the device: every kernel (and the all-gather) is enqueued, nothing has been
    read back.  ``result()`` synchronises and combines on the host.  Lets a caller keep several passes in flight."""

    def __init__(self, gathered: torch.Tensor):
        self.gathered = gathered  # [W, 9]: sdeng_logz statistics + particle count per rank

    def result(self) -> dict:
        g = self.gathered
        return combine_stats(g[:, :8], g[:, 8])


def _local_stats(rnd, stats_fn):
    if stats_fn is None:
        from . import engine
        return engine.logz_stats(rnd, want_weights=False)[0]
    return stats_fn(rnd).to(rnd.device)


def global_results_async(rnd: torch.Tensor, dist=None, stats_fn=None) -> PendingResults:
    """Enqueue the estimators over ALL ranks' particles from this rank's ``rnd`` shard [B,1] (device tensor).
    ``stats_fn`` replaces the HIP reduction (``engine.logz_stats``) -- the CPU tests pass ``stats_reference``."""
    stats = _local_stats(rnd, stats_fn)
    # torch.full, not torch.tensor([...], device=...): a host->device copy of pageable memory synchronises the stream and
    # would stop the caller from keeping several passes in flight
    count = torch.full((1,), float(rnd.shape[0]), dtype=stats.dtype, device=rnd.device)
    payload = torch.cat([stats, count])
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return PendingResults(payload.view(1, N_STATS + 1))
    world = dist.get_world_size()
    gathered = torch.empty(world * (N_STATS + 1), dtype=payload.dtype, device=payload.device)
    dist.all_gather_into_tensor(gathered, payload)
    return PendingResults(gathered.view(world, N_STATS + 1))


def global_results(rnd: torch.Tensor, dist=None, stats_fn=None) -> dict:
    """Estimators over ALL ranks' particles from this rank's ``rnd`` shard [B,1] (device tensor)."""
    return global_results_async(rnd, dist, stats_fn).result()


def global_weights(rnd: torch.Tensor, dist=None, stats_fn=None):
    """This rank's shard of ``Results.weights = softmax(-rnd, 0)`` (losses/oc.py:150-161) normalised over ALL ranks' particles:
    w_i = exp(-rnd_i - M) / S with M, S the global maximum and exponential sum from the same 36-byte all-gather.  Returns
    (weights [B_local, 1], global estimators dict); summed over the ranks the weights give 1."""
    res = global_results(rnd, dist, stats_fn)
    w = torch.exp((-rnd.double() - res["max_neg_rnd"])) / res["sum_exp"]
    return w.to(rnd.dtype).view(-1, 1), res


# ---- sharded training: the objective over ALL ranks' particles, the gradients summed across the ranks --------------------------------
# Layout of the per-shard moments vector (float64): the ONE definition shard_moments / combine_moments / global_moments share.
M_N, M_MEAN, M_M2, M_ROWS = range(4)
N_MOMENTS = 4


def is_sharded(dist) -> bool:
    """``dist`` is an initialised process group of more than one rank (anything else is today's single-process path)."""
    return dist is not None and dist.is_initialized() and dist.get_world_size() > 1


def _exchange(op: str, dist, out: torch.Tensor, *src: torch.Tensor) -> torch.Tensor:
    """ONE collective (``dist.all_gather_into_tensor(out, src)`` / ``dist.all_reduce(out)``) on the tensors where they live (RCCL), or
    -- a gloo group handed device tensors -- staged through the host.  -> the result, on ``out``'s device."""
    staged = out.is_cuda and "nccl" not in str(dist.get_backend())
    o, s = (out.cpu(), [t.cpu() for t in src]) if staged else (out, list(src))
    if op == "all_reduce":
        dist.all_reduce(o, op=dist.ReduceOp.SUM)
    else:
        dist.all_gather_into_tensor(o, *s)
    return o.to(out.device) if staged else o


def shard_moments(rnd: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """(n, mean, M2 = sum (x - mean)^2, rows) of the entries of one shard's ``rnd`` that ``mask`` keeps, as a float64 [4] on ``rnd``'s
    device (torch, like ``stats_reference``: CPU or GPU, two passes, nothing read back).  An empty shard -- no rows, or none kept --
    gives (0, 0, 0, rows); entries the mask drops may be non-finite."""
    v, m = rnd.detach().double().reshape(-1), mask.reshape(-1)
    n = m.sum().double()
    zero = torch.zeros((), dtype=torch.float64, device=v.device)
    mean = torch.where(m, v, zero).sum() / n.clamp(min=1.0)
    dev = torch.where(m, v - mean, zero)
    return torch.stack([n, mean, (dev * dev).sum(), torch.full_like(n, float(v.numel()))])


def combine_moments(moments: torch.Tensor) -> torch.Tensor:
    """moments [W,4] as written by ``shard_moments`` -> the [4] of the concatenated shards, folded in rank order with Chan's pairwise
    update (delta = mean_b - mean_a; mean = mean_a + delta n_b / n; M2 = M2_a + M2_b + delta^2 n_a n_b / n).  Stays on the device of
    ``moments``; empty shards drop out.  Not the sum / sum-of-squares form: at mean 1e4 and spread 1e-2 that one loses 1e-4 of the variance
    in float64 where this keeps 1e-12 (tests/test_sharded_training_cpu.py)."""
    acc = moments[0]
    for b in moments[1:]:
        n = acc[M_N] + b[M_N]
        frac = b[M_N] / n.clamp(min=1.0)
        delta = b[M_MEAN] - acc[M_MEAN]
        acc = torch.stack([n, acc[M_MEAN] + delta * frac, acc[M_M2] + b[M_M2] + delta * delta * acc[M_N] * frac, acc[M_ROWS] + b[M_ROWS]])
    return acc


def global_moments(rnd: torch.Tensor, mask: torch.Tensor, dist=None) -> torch.Tensor:
    """(n, mean, M2, rows) of the entries ``mask`` keeps over ALL ranks' shards of ``rnd`` -- float64 [4] on ``rnd``'s device, the same
    bits on every rank -- from ONE all-gather of 32 bytes per rank.  Without a process group of more than one rank: this shard's."""
    local = shard_moments(rnd, mask)
    if not is_sharded(dist):
        return local
    world = dist.get_world_size()
    gathered = _exchange("all_gather", dist, torch.empty(world * N_MOMENTS, dtype=local.dtype, device=local.device), local)
    return combine_moments(gathered.view(world, N_MOMENTS))


def unbiased_var(moments: torch.Tensor) -> torch.Tensor:
    """M2 / (n - 1) of a moments vector; NaN for n <= 1, as ``torch.var`` gives."""
    n = moments[M_N]
    return torch.where(n > 1, moments[M_M2] / (n - 1), torch.full_like(n, float("nan")))


def kept_mean(moments: torch.Tensor) -> torch.Tensor:
    """The mean of a moments vector; NaN for n = 0, as ``torch.mean`` of nothing gives."""
    n = moments[M_N]
    return torch.where(n > 0, moments[M_MEAN], torch.full_like(n, float("nan")))


def all_reduce_grads(params, dist) -> None:
    """Sum the ``.grad`` of every parameter over the ranks with ONE all-reduce: the gradients are flattened into one buffer (a missing one
    counts as zeros), followed by one flag per parameter (1 where this rank has a gradient), reduced with SUM and scattered back.  SUM, never
    AVG: the sharded objectives are already scaled by the global particle count, so each rank holds an exact partial sum.  A parameter
    without a gradient on ANY rank keeps ``None`` -- read from the summed flags, no second collective.  No process group of more than one rank:
    nothing happens."""
    params = list(params)
    if not is_sharded(dist) or not params:
        return
    dtype, device = params[0].dtype, params[0].device
    flat = [(p.grad.detach().reshape(-1).to(dtype) if p.grad is not None else torch.zeros(p.numel(), dtype=dtype, device=device)) for p in params]
    have = [p.grad is not None for p in params]
    flags = torch.ones(len(params), dtype=dtype, device=device) if all(have) else torch.tensor([float(h) for h in have], dtype=dtype).to(device)
    buf = _exchange("all_reduce", dist, torch.cat(flat + [flags]))
    n_par = len(params)
    # the summed flags are read back only where this rank lacks a gradient (the usual step has them all): they are >= 1 wherever it has one
    anyone = have if all(have) else (buf[-n_par:] > 0.5).tolist()
    off = 0
    for p, mine, some in zip(params, have, anyone):
        n = p.numel()
        if some:
            g = buf[off:off + n].view(p.shape).to(p.dtype)
            if mine:
                p.grad.copy_(g)
            else:
                p.grad = g.clone()
        off += n
