"""Inputs of the random-walk Metropolis and run_smc_sampler / run_re_sampler fixtures (tests/golden/rwmh_*.npz, run_*_d3.npz), shared by
their generator (tests/golden/gen_golden_rwmh.py) and by the CPU and GPU tests: the fixtures store what the reference returned, the inputs
are rebuilt from their meta here."""
from __future__ import annotations

import torch

from tests import golden_cases as gc

RWMH_CASES = ["rwmh_rings_d2", "rwmh_checkerboard_d2"]
RUN_CASES = ["run_smc_d3", "run_re_d3"]

# four starts outside every square of the width-4 checkerboard: three next to a square (the chains walk in: lp = -inf, then a proposal
# inside has log_acc = +inf), one far away (every proposal stays outside: log_acc = NaN, the chain never moves)
CHECKERBOARD_OUTSIDE = [[-3.0, 3.0], [1.0, 3.0], [-1.0, 1.0], [10.0, 10.0]]


def rwmh_x_init(m, target):
    """Start points of a rwmh fixture, one per 'mode' (mcmc_sample repeats each n_chains_per_mode times)."""
    if m["target"] == "rings":
        g = torch.Generator().manual_seed(m["seed"])
        return 3.0 * torch.randn(m["n_init"], 2, generator=g)
    return torch.cat([target.loc.detach().cpu().float(), torch.tensor(CHECKERBOARD_OUTSIDE)])


def rwmh_kwargs(m):
    n_chains = m["n_init"] * m["n_chains_per_mode"]
    return dict(mcmc_type="rwmh", step_size=m["step_size"], n_chains_per_mode=m["n_chains_per_mode"], dataset_length=n_chains * m["n_keep"],
                n_warmup_steps=m["n_warm"], adapt_step_size=True, shuffle=False)


def two_mode_log_prob(x):
    """Closed-form 3-D two-mode target of the run_* fixtures, unnormalised: N(+2, 0.3 I) + N(-2, 0.3 I) (the target end of
    golden_cases.tempered_log_prob_and_grads).  A plain function: nothing the engine can resolve."""
    m, v = 2.0, 0.3
    la, lb = -0.5 * ((x - m) ** 2).sum(-1) / v, -0.5 * ((x + m) ** 2).sum(-1) / v
    return torch.logsumexp(torch.stack([la, lb]), dim=0)


def two_mode_score(x):
    return gc.tempered_log_prob_and_grads(torch.ones(x.shape[0], 1, dtype=x.dtype, device=x.device), x)[1]


def run_inputs(m):
    """mean [d], var ([d] or [d,d]) and the keyword arguments of a run_smc_sampler / run_re_sampler fixture."""
    d = m["d"]
    g = torch.Generator().manual_seed(m["seed"])
    mean = 0.3 * torch.randn(d, generator=g)
    if m["full"]:
        a = torch.randn(d, d, generator=g)
        var = 0.5 * a @ a.T + 6.0 * torch.eye(d)
    else:
        var = 6.0 + 3.0 * torch.rand(d, generator=g)
    kw = dict(n_steps=m["n_levels"], step_size=m["step"], n_mcmc_steps=m["n_steps"], n_warmup_mcmc_steps=m["n_warm"],
              target_log_prob=two_mode_log_prob, target_score=two_mode_score if m["with_score"] else None)
    if m["sampler"] == "smc":
        kw.update(n_particles=m["B"], reweight_threshold=m["reweight_threshold"])
    else:
        kw.update(batch_size=m["B"], swap_frequency=m["swap_frequency"])
    return mean, var, kw
