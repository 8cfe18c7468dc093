"""Annealed samplers of ``sde_sampler/additions/ebm_mle.py``: ``smc_sampler`` (:11-195, annealed Langevin / sequential
Monte Carlo), ``make_re_pairings`` (:198-216), ``re_step`` (:219-266) and ``re_sampler`` (:269-400, replica exchange), on top
of the local moves of ``additions/mcmc.py``.  They are host compositions: what costs time is ``log_prob_and_grads(t, x)`` at
every proposal, which ``hip_tempered_log_prob_and_grads`` serves from the HIP distribution kernels and ``ebm_log_prob_and_grads``,
for an energy-based reference, from ``sdeng_tilted_eval`` (no autograd either way); over either, the unpreconditioned local moves of a
level run in one launch (``_native_route``).  ``MaximumLikelihoodEBM`` (:401-808) is the
trainer around them: its energies and their parameter gradients come from ``sdeng_tilted_vjp``, one launch per ``net.energy`` call.

Same arguments, return values, random-number consumption order and diagnostics as the reference, including the
preconditioned moves (``precond_matrix_per_noise``) and the PDDS transition and weights (``use_pdds_weights``).  Not provided:
the trainer's ``'smc_pdds'`` sampler type (the reference's branch reads an undefined ``x_init``)."""
from __future__ import annotations

import torch

from .. import engine as E
from .mcmc import heuristics_step_size, mala_step, precond_mala_step, precond_ula_step, ula_step


def hip_tempered_log_prob_and_grads(target, prior):
    """(t, x) -> (log pi_t(x) [B], grad [B,d]) for the geometric path pi_t = prior^(1-t) target^t, t in [0,1] one value per
    row ([B,1]); both log-densities and scores come from ``sdeng_dist_eval`` launches (any distribution the engine knows)."""
    def fn(t, x):
        lp1, s1 = E.dist_eval(target, x.detach())
        lp0, s0 = E.dist_eval(prior, x.detach())
        w = t.to(x.dtype).expand(x.shape[0], 1) if t.dim() else t
        return ((1.0 - w) * lp0 + w * lp1).flatten(), (1.0 - w) * s0 + w * s1
    fn.hip_pair = (target, prior)  # lets the samplers below run whole levels of local moves in one launch (sdeng_langevin_moves)
    return fn


# Local moves of a level as ONE HIP launch when they are not preconditioned and the density is one the engine knows as a whole: the
# annealing path of hip_tempered_log_prob_and_grads (csrc/prep_kernels.hip k_chain_moves, sdeng_langevin_moves) or an energy-based
# reference -- ebm_log_prob_and_grads(net) or the trainer's own MaximumLikelihoodEBM.log_prob_and_grads -- (csrc/tilted_moves_inst.hip
# k_tilted_moves, sdeng_tilted_moves).  NATIVE_MOVES = False: the host loop, one evaluation launch per move.  NATIVE_NOISE = False: the
# random numbers still come from torch's generator, drawn in the reference's order (the chains are then the reference's chains,
# tests/golden/smc_*.npz, re_*.npz); True: counter-based draws inside the kernel (seeded by NATIVE_SEED and a per-call counter).
NATIVE_MOVES, NATIVE_NOISE, NATIVE_SEED = True, False, 1
_native_calls = [0]


class _EbmRoute:
    """The route of local moves over an energy-based reference: its net."""

    def __init__(self, net):
        self.net = net


def _hip_net(log_prob_and_grads):
    """The energy-based reference behind a ``log_prob_and_grads`` callable, or None: the mark of ``ebm_log_prob_and_grads``, or the
    trainer's bound method (``MaximumLikelihoodEBM.hip_net``)."""
    net = getattr(log_prob_and_grads, "hip_net", None)
    if net is None and getattr(log_prob_and_grads, "__func__", None) is MaximumLikelihoodEBM.log_prob_and_grads:
        net = log_prob_and_grads.__self__.hip_net
    return net


def _native_route(log_prob_and_grads, x, precond):
    """The one route decision of the samplers' local moves: the (target, prior) pair of an analytic annealing path, an ``_EbmRoute``,
    or None -- the host loop.  No condition on the size: the one-launch moves were no slower at any measured shape (profiles/tilted_moves.log)."""
    if not NATIVE_MOVES or precond is not None or not x.is_cuda or x.dim() != 2 or x.dtype != torch.float32:
        return None
    pair = getattr(log_prob_and_grads, "hip_pair", None)
    if pair is not None:
        return pair
    net = _hip_net(log_prob_and_grads)
    if net is not None and E.tilted_refusal(net, x.device) is None:  # "tilted_eval would accept this net"; else the host loop raises its error
        return _EbmRoute(net)
    return None


def _native_run(route, t, x, lp, grad, step, n_moves, keep_from, use_ula, target_acceptance, want_samples=True):
    """n_moves local moves of all chains; x / lp / grad / step ([B,d], [B], [B,d], [B] contiguous) are updated in place.  ``route``: what
    ``_native_route`` returned.  A pair with ``grad is None``: random-walk Metropolis moves on ``pair[0]`` alone (no ``t``, no ULA);
    otherwise Langevin moves on the path between the pair, or over the energy-based reference at the rows' times ``t``."""
    _native_calls[0] += 1
    kw = dict(keep_from=keep_from, target_acceptance=target_acceptance if not use_ula else 0.0, noise="philox" if NATIVE_NOISE else "torch",
              seed=(NATIVE_SEED + 0x9E3779B97F4A7C15 * _native_calls[0]) & 0xFFFFFFFFFFFFFFFF, want_samples=want_samples)
    if isinstance(route, _EbmRoute):
        with torch.no_grad():
            return E.tilted_moves(route.net, t, x, lp, grad, step, n_moves, unadjusted=use_ula, **kw)
    if grad is None:
        return E.rwmh_moves(route[0], x, lp, step, n_moves, **kw)
    return E.langevin_moves(route[0], route[1], x, lp, grad, step, n_moves, t=None if t is None else t.reshape(-1), unadjusted=use_ula, **kw)


def _pmul(mat, v):
    return torch.matmul(mat, v.unsqueeze(-1)).squeeze(-1)


class _LocalMove:
    """One MALA (or ULA) move at a fixed level, plain or preconditioned, with the step-size heuristic of
    additions/mcmc.py:54-72.  State: (x, log-density, gradient, preconditioned gradient or None)."""

    def __init__(self, log_prob_and_grad, use_ula, target_acceptance, precond=None):
        self.f, self.use_ula, self.target, self.precond = log_prob_and_grad, use_ula, target_acceptance, precond

    def pgrad(self, grad):
        return None if self.precond is None else _pmul(self.precond[0], grad)

    def __call__(self, x, lp, grad, pgrad, step):
        log_acc = None
        if self.precond is not None:
            if self.use_ula:
                x, lp, grad, pgrad = precond_ula_step(x, lp, grad, pgrad, self.f, step, *self.precond)
            else:
                x, lp, grad, pgrad, log_acc = precond_mala_step(x, lp, grad, pgrad, self.f, step, *self.precond)
        elif self.use_ula:
            x, lp, grad = ula_step(x, lp, grad, self.f, step)
        else:
            x, lp, grad, log_acc = mala_step(x, lp, grad, self.f, step)
        if log_acc is not None and self.target > 0.0:
            step = heuristics_step_size(step, log_acc, target_acceptance=self.target)
        return x, lp, grad, pgrad, step, log_acc


def smc_sampler(x_init, times, log_prob_and_grads, n_warmup_mcmc_steps, n_mcmc_steps, step_sizes_per_noise, per_noise_init=False,
                reweight_threshold=1.0, use_pdds_weights=False, sde=None, target_acceptance=0.75, precond_matrix_per_noise=None,
                precond_matrix_chol_per_noise=None, use_ula=False, verbose=False):
    """additions/ebm_mle.py:11-195.  Levels are visited from the last (``times[-1]``) to the first; with
    ``reweight_threshold > 0`` the particles carry importance weights between levels and are resampled (multinomial) when
    the normalised ESS drops below the threshold; with ``use_pdds_weights`` they are first moved by the SDE's EI denoising
    kernel and weighted with the forward / backward transition densities (:88-107).
    Returns (samples [n_levels, n_mcmc_steps, B, *data], updated step sizes, diags)."""
    if per_noise_init and reweight_threshold > 0.0:
        raise ValueError("Can't use per_noise_init in SMC mode.")
    if sde is None and use_pdds_weights:
        raise ValueError("Can't use PDDS weights without the SDE object.")
    n_levels = times.shape[0]
    B = x_init.shape[1] if per_noise_init else x_init.shape[0]
    data_shape = x_init.shape[2:] if per_noise_init else x_init.shape[1:]
    smc = reweight_threshold > 0.0
    use_precond = precond_matrix_per_noise is not None and precond_matrix_chol_per_noise is not None
    samples = torch.empty((n_levels, n_mcmc_steps, B, *data_shape), device=x_init.device)
    ess_logs = torch.ones((n_levels,))
    mean_accs = torch.empty((n_levels,))
    log_w = torch.zeros((B,), device=x_init.device)
    x, x_prev, lp_prev, grad_prev = x_init.clone(), None, None, None
    for lvl in range(n_levels - 1, -1, -1):
        first = lvl == n_levels - 1
        x = x_init[lvl].clone() if per_noise_init else x.clone()
        precond = (precond_matrix_per_noise[lvl], precond_matrix_chol_per_noise[lvl]) if use_precond else None
        move = _LocalMove(lambda y, lvl=lvl: log_prob_and_grads(times[lvl], y), use_ula, target_acceptance, precond)
        step = step_sizes_per_noise[lvl]
        lp, grad = move.f(x)
        pgrad = move.pgrad(grad)
        if use_pdds_weights and not first:  # reverse-SDE move from the previous level, then the densities at the moved points
            x, z = sde.ei_integration_step(x_prev, sde.terminal_t - times[lvl + 1], sde.terminal_t - times[lvl], grad_prev)
            lp_backward = -0.5 * torch.sum(torch.square(z), dim=-1)
            mean_f, var_f = sde.transition_params(times[lvl], times[lvl + 1])
            lp_forward = -0.5 * torch.sum(torch.square(mean_f * x - x_prev) / var_f, dim=-1)
            lp, grad = move.f(x)
            pgrad = move.pgrad(grad)
        if smc and not first:
            if use_pdds_weights:
                log_w = lp - lp_prev
                log_w += lp_forward - lp_backward
            else:  # this level's density over the previous level's, at the same points
                log_w += lp - lp_prev
            w = torch.nn.functional.softmax(log_w, dim=0)
            ess = (1.0 / torch.sum(torch.square(w))) / B
            ess_logs[lvl] = ess.cpu().clone()
            if ess < reweight_threshold:
                idx = torch.multinomial(w, B, replacement=True)
                x, lp, grad = x[idx], lp[idx], grad[idx]
                if use_precond:
                    pgrad = pgrad[idx]
                log_w.zero_()
        route = _native_route(log_prob_and_grads, x, precond)
        if route is not None:  # all warm-up and sampling moves of the level in one launch
            x, lp, grad = x.contiguous(), lp.contiguous().clone(), grad.contiguous().clone()
            step_flat = step.to(torch.float32).reshape(-1).expand(B).contiguous().clone()
            got, acc_sum, _ = _native_run(route, times[lvl], x, lp, grad, step_flat, n_warmup_mcmc_steps + n_mcmc_steps,
                                          n_warmup_mcmc_steps, use_ula, target_acceptance)
            samples[lvl] = got
            step = step_flat.view(step.shape)
        else:
            for _ in range(n_warmup_mcmc_steps):
                x, lp, grad, pgrad, step, _ = move(x, lp, grad, pgrad, step)
            acc_sum = 0.0
            for i in range(n_mcmc_steps):
                x, lp, grad, pgrad, step, log_acc = move(x, lp, grad, pgrad, step)
                if log_acc is not None:
                    acc_sum = acc_sum + torch.exp(torch.minimum(torch.zeros_like(log_acc), log_acc))
                samples[lvl, i] = x.clone()
        if not use_ula:
            mean_accs[lvl] = (acc_sum / n_mcmc_steps).mean()
        step_sizes_per_noise[lvl] = step.clone()
        x_prev, grad_prev, lp_prev = x.clone(), grad.clone(), lp.clone()
        if verbose:
            print(f"smc level {lvl}: ess {float(ess_logs[lvl]):.3f}" + ("" if use_ula else f", local acc {float(mean_accs[lvl]):.3f}"))
    diags = {}
    if not use_ula:
        diags["local_acc"] = mean_accs
    if smc:
        diags["ess"] = ess_logs
    return samples, step_sizes_per_noise, diags


def make_re_pairings(num_noise_levels, device=None):
    """additions/ebm_mle.py:198-216: neighbour pairs (i, i+1) with i even, and with i odd."""
    lvl = torch.arange(num_noise_levels, device=device)
    has_next = lvl + 1 < num_noise_levels
    return [torch.stack([lvl[sel], lvl[sel] + 1], dim=-1) for sel in ((lvl % 2 == 0) & has_next, (lvl % 2 == 1) & has_next)]


def re_step(x, log_prob_x, grad_x, log_prob_and_grads, times, idx_i, idx_j, batch_size, data_shape, data_shape_ones):
    """additions/ebm_mle.py:219-266: propose swapping the states of levels ``idx_i`` and ``idx_j`` chain by chain; accept with
    probability min(1, pi_i(x_j) pi_j(x_i) / (pi_i(x_i) pi_j(x_j)))."""
    n_pairs = idx_i.shape[0]
    lp_ii, lp_jj = log_prob_x[idx_i], log_prob_x[idx_j]
    g_ii, g_jj = grad_x[idx_i], grad_x[idx_j]
    with torch.no_grad():
        lp_ij, g_ij = log_prob_and_grads(times[idx_i], x[idx_j])
        lp_ji, g_ji = log_prob_and_grads(times[idx_j], x[idx_i])
    log_acc = (lp_ij + lp_ji) - (lp_ii + lp_jj)
    swap = torch.rand_like(log_acc).log_().lt_(log_acc).bool()
    re_acc = swap.float().mean()
    old = x.clone()
    log_prob_x[idx_i] = torch.where(swap, lp_ij, lp_ii)
    log_prob_x[idx_j] = torch.where(swap, lp_ji, lp_jj)
    swap = swap.view((n_pairs, batch_size, *data_shape_ones))
    x[idx_i] = torch.where(swap, old[idx_j], old[idx_i])
    x[idx_j] = torch.where(swap, old[idx_i], old[idx_j])
    grad_x[idx_i] = torch.where(swap, g_ij, g_ii)
    grad_x[idx_j] = torch.where(swap, g_ji, g_jj)
    return x, log_prob_x, grad_x, re_acc


def re_sampler(x_init, times, log_prob_and_grads, swap_frequency, n_warmup_mcmc_steps, n_mcmc_steps, step_sizes_per_noise,
               per_noise_init=False, target_acceptance=0.75, precond_matrix_per_noise=None, precond_matrix_chol_per_noise=None,
               use_ula=False, verbose=False):
    """additions/ebm_mle.py:269-400: all levels advance together as one flattened batch of n_levels*B chains; every
    ``swap_frequency``-th step is a swap step (even pairs, then odd pairs, alternating) instead of a local move."""
    n_levels = times.shape[0]
    B = x_init.shape[1] if per_noise_init else x_init.shape[0]
    data_shape = x_init.shape[2:] if per_noise_init else x_init.shape[1:]
    ones = (1,) * len(data_shape)
    samples = torch.empty((n_levels, n_mcmc_steps, B, *data_shape), device=x_init.device)
    mean_local_accs = torch.zeros((n_levels,))
    mean_swap_acc = 0.0
    t_flat = times.reshape((-1, *ones))

    def batched(t, y):  # (K, B, ...) inputs of a swap step
        lp, g = log_prob_and_grads(t.view((-1, *ones)), y.view((-1, *data_shape)))
        return lp.view(y.shape[:2]), g.view(y.shape)

    precond = None
    if precond_matrix_per_noise is not None and precond_matrix_chol_per_noise is not None:  # [n_levels, B, d, d] -> one per chain
        precond = (precond_matrix_per_noise.view((-1, *precond_matrix_per_noise.shape[2:])),
                   precond_matrix_chol_per_noise.view((-1, *precond_matrix_chol_per_noise.shape[2:])))
    move = _LocalMove(lambda y: log_prob_and_grads(t_flat, y), use_ula, target_acceptance, precond)
    x = x_init.clone() if per_noise_init else x_init.unsqueeze(0).repeat((n_levels, 1, *ones))
    x = x.view((-1, *data_shape))
    step = step_sizes_per_noise.view((-1, *ones))
    lp, grad = move.f(x)
    pgrad = move.pgrad(grad)
    pairs = make_re_pairings(n_levels, x_init.device)
    native = _native_route(log_prob_and_grads, x, precond)
    total = n_warmup_mcmc_steps + n_mcmc_steps
    if native is not None:
        x, lp, grad = x.contiguous().clone(), lp.contiguous().clone(), grad.contiguous().clone()
        step_shape, step = step.shape, step.to(torch.float32).reshape(-1).expand(x.shape[0]).contiguous().clone()

    def store(it, y):
        if it >= n_warmup_mcmc_steps:
            samples[:, it - n_warmup_mcmc_steps] = y.reshape((-1, B, *data_shape))
        if verbose and it % 50 == 0:
            print(f"re step {it}: swap acc {float(mean_swap_acc):.3f}")

    it = 0
    while it < total:
        if it % swap_frequency == 0:
            pr = pairs[(it // swap_frequency) % 2]
            x, lp, grad, mean_swap_acc = re_step(x.view((-1, B, *data_shape)), lp.view((-1, B)), grad.view((-1, B, *data_shape)), batched,
                                                 times, pr[:, 0], pr[:, 1], B, data_shape, ones)
            x, grad, lp = x.reshape((-1, *data_shape)).contiguous(), grad.reshape((-1, *data_shape)).contiguous(), lp.flatten().contiguous()
            pgrad = move.pgrad(grad)
            store(it, x)
            it += 1
        elif native is None:  # one host move
            x, lp, grad, pgrad, step, log_acc = move(x, lp, grad, pgrad, step)
            if log_acc is not None:
                mean_local_accs = torch.exp(torch.minimum(torch.zeros_like(log_acc), log_acc)).view((-1, B)).mean(dim=-1)
            store(it, x)
            it += 1
        else:  # the local moves up to the next swap step in one launch
            run = min(swap_frequency - it % swap_frequency, total - it)
            keep = max(0, n_warmup_mcmc_steps - it)
            got, _, last = _native_run(native, t_flat, x, lp, grad, step, run, min(keep, run), use_ula, target_acceptance, want_samples=keep < run)
            if keep < run:
                first = it + keep - n_warmup_mcmc_steps
                samples[:, first:first + run - keep] = got.view(run - keep, n_levels, B, *data_shape).transpose(0, 1)
            if last is not None:
                mean_local_accs = last.view((-1, B)).mean(dim=-1)
            it += run
    if native is not None:
        step = step.view(step_shape)
    diags = {"swap_acc": mean_swap_acc}
    if not use_ula:
        diags["local_acc"] = mean_local_accs
    return samples, step, diags


def ebm_log_prob_and_grads(net):
    """The ``log_prob_and_grads(t, x)`` callable ``smc_sampler`` / ``re_sampler`` take, for an energy-based reference ``net``
    (``GMMTitledPotential`` / ``GaussTiltedPotential``): mirror of ``MaximumLikelihoodEBM.log_prob_and_grads``
    (additions/ebm_mle.py:440-446), served by one ``sdeng_tilted_eval`` launch per call -- no autograd.  The samplers call it for the
    initial evaluation and the swap steps; their local moves run over ``net`` in one launch per level (``sdeng_tilted_moves``) unless
    ``NATIVE_MOVES`` is off or the moves are preconditioned -- then the host loops call it once per move."""
    if not getattr(net, "has_unnorm_log_prob_and_grad", False):
        raise E.UnsupportedByEngine("ebm_log_prob_and_grads: the net has no unnorm_log_prob_and_grad (autograd energies are not on the HIP path)")

    def fn(t, x):
        with torch.no_grad():
            return E.tilted_eval(net, t, x.detach())
    fn.hip_net = net  # lets the samplers above run whole levels of local moves in one launch (sdeng_tilted_moves)
    return fn


class MaximumLikelihoodEBM(torch.nn.Module):
    """Maximum-likelihood training of an energy-based reference (mirror of additions/ebm_mle.py:401-808): positives are the data noised
    to every level, negatives come from the annealed samplers above (``'annealed_mcmc'``, ``'smc'``, ``'replica_exchange'``) or from
    Langevin chains started at the positives (``'cd'``), and the loss is mean(E(pos) - E(neg)) (+ ``reg_val`` mean(E^2)).  Same
    constructor, attributes, arguments, return tuples and random-number consumption order as the reference (DataLoader shuffle,
    ``randn_like`` for the positives, ``sample_prior`` on the very first batch, then the samplers).

    On the engine every ``net.energy`` of ``train`` is one ``sdeng_tilted_vjp`` launch and its backward the products of
    ``engine.tilted_param_grads`` (``net.param_grads`` is switched on for the duration of ``train``); the samplers evaluate through
    ``net.unnorm_log_prob_and_grad`` (``sdeng_tilted_eval``) with the parameters frozen.  ``'smc_pdds'`` raises: the reference's branch
    reads an ``x_init`` it never defines."""

    def __init__(self, sde, prior, net, sampler_type, step_sizes_per_noise=1e-3, precond_matrix_per_noise=None,
                 precond_matrix_chol_per_noise=None, use_ula=False, reweight_threshold=1.0, swap_frequency=16, target_acceptance=0.75,
                 perc_keep_mcmc=-1.0, use_snr_adapted_disc=False, start_eps=1e-3, end_eps=0.0, n_steps=100):
        super().__init__()
        self.sde, self.prior = sde, prior
        self.prior.cpu()
        self.net = net.cpu()
        self.sampler_type, self.reweight_threshold, self.swap_frequency = sampler_type, reweight_threshold, swap_frequency
        self.step_sizes_per_noise = step_sizes_per_noise
        self.precond_matrix_per_noise, self.precond_matrix_chol_per_noise = precond_matrix_per_noise, precond_matrix_chol_per_noise
        self.use_precond = precond_matrix_per_noise is not None and precond_matrix_chol_per_noise is not None
        self.use_ula, self.target_acceptance = use_ula, target_acceptance
        self.use_snr_adapted_disc, self.perc_keep_mcmc = use_snr_adapted_disc, perc_keep_mcmc
        self.start_eps, self.end_eps, self.n_steps = start_eps, end_eps, n_steps
        self.build_time_disc()

    def build_time_disc(self):
        from ..utils.common import get_timesteps
        kw = dict(sde=self.sde) if self.use_snr_adapted_disc else {}
        self.register_buffer("times", get_timesteps(start=self.start_eps, end=self.sde.terminal_t - self.end_eps, steps=self.n_steps,
                                                    **kw).unsqueeze(-1))

    @property
    def hip_net(self):
        """The net when ``log_prob_and_grads`` is its ``unnorm_log_prob_and_grad`` and nothing else: what the samplers' route decision
        reads off the bound method."""
        return self.net if getattr(self.net, "has_unnorm_log_prob_and_grad", False) else None

    def log_prob_and_grads(self, t, y):
        if self.net.has_unnorm_log_prob_and_grad:
            return self.net.unnorm_log_prob_and_grad(t, y)
        y_ = y.clone().requires_grad_(True)
        lp = self.net.unnorm_log_prob(t, y_)
        return lp, torch.autograd.grad(lp.sum(), y_)[0].detach()

    def sample_model(self, batch_size, times_expanded, is_very_first_negative_sampling, initial_n_warmup_mcmc_steps, n_warmup_mcmc_steps,
                     n_mcmc_steps, x_init_persistant):
        if self.sampler_type == "smc_pdds":
            raise NotImplementedError("sampler_type 'smc_pdds': the reference's branch reads an undefined x_init (additions/ebm_mle.py:487-503)")
        if self.sampler_type not in ("annealed_mcmc", "smc", "replica_exchange"):
            raise NotImplementedError("Sampler {} not found.".format(self.sampler_type))
        frozen = [p.requires_grad for p in self.net.parameters()]
        for p in self.net.parameters():
            p.requires_grad_(False)
        try:
            common = dict(times=times_expanded, log_prob_and_grads=self.log_prob_and_grads,
                          n_warmup_mcmc_steps=initial_n_warmup_mcmc_steps if is_very_first_negative_sampling else n_warmup_mcmc_steps,
                          n_mcmc_steps=n_mcmc_steps, step_sizes_per_noise=self.step_sizes_per_noise, target_acceptance=self.target_acceptance,
                          precond_matrix_per_noise=self.precond_matrix_per_noise if self.use_precond else None,
                          precond_matrix_chol_per_noise=self.precond_matrix_chol_per_noise if self.use_precond else None,
                          use_ula=self.use_ula, verbose=False)
            if self.sampler_type == "replica_exchange":
                xs_neg, self.step_sizes_per_noise, diags = re_sampler(x_init=x_init_persistant, swap_frequency=self.swap_frequency,
                                                                      per_noise_init=True, **common)
            else:
                x_init = self.prior.sample((batch_size,))
                xs_neg, self.step_sizes_per_noise, diags = smc_sampler(
                    x_init=x_init, reweight_threshold=self.reweight_threshold if self.sampler_type == "smc" else 0.0, **common)
        finally:
            for p, state in zip(self.net.parameters(), frozen):
                p.requires_grad_(state)
        return xs_neg, diags

    def cd_sampling(self, times_expanded, n_warmup_mcmc_steps, n_mcmc_steps, xs_pos):
        ones = (1,) * (xs_pos.dim() - 1)
        t_rows = times_expanded.reshape((-1, *ones))
        def f(z):  # the chains carry no graph (train detaches them): evaluated like the samplers' moves, by sdeng_tilted_eval
            with torch.no_grad():
                return self.log_prob_and_grads(t_rows, z)
        xs_neg = torch.empty((n_mcmc_steps, *xs_pos.shape), device=xs_pos.device)
        x = xs_pos.clone()
        lp, grad = f(x)
        precond = (self.precond_matrix_per_noise, self.precond_matrix_chol_per_noise) if self.use_precond else None
        move = _LocalMove(f, self.use_ula, self.target_acceptance, precond)
        pgrad, acc = move.pgrad(grad), None
        total = n_warmup_mcmc_steps + n_mcmc_steps
        with torch.no_grad():  # (as f evaluates: train calls this in grad mode with trainable parameters)
            route = _native_route(self.log_prob_and_grads, x, precond) if total > 0 and torch.is_tensor(self.step_sizes_per_noise) else None
        if route is not None:  # all moves of the batch in one launch
            lp, grad = lp.contiguous().clone(), grad.contiguous().clone()
            steps = self.step_sizes_per_noise
            step = steps.to(torch.float32).reshape(-1).expand(x.shape[0]).contiguous().clone()
            xs_neg, _, last = _native_run(route, t_rows, x, lp, grad, step, total, n_warmup_mcmc_steps, self.use_ula, self.target_acceptance)
            self.step_sizes_per_noise = step.view(steps.shape)
            return xs_neg, ({} if self.use_ula else {"local_acc": last.mean().cpu()})
        for it in range(n_warmup_mcmc_steps + n_mcmc_steps):
            x, lp, grad, pgrad, self.step_sizes_per_noise, log_acc = move(x, lp, grad, pgrad, self.step_sizes_per_noise)
            if log_acc is not None:
                acc = torch.exp(torch.minimum(torch.zeros_like(log_acc), log_acc)).mean().cpu()
            if it >= n_warmup_mcmc_steps:
                xs_neg[it - n_warmup_mcmc_steps] = x.clone()
        return xs_neg, ({} if self.use_ula else {"local_acc": acc})

    def save_logs(self, losses, losses_grad, diagnostics, use_ema, epoch_id, ckpt_filepath_maker):
        import pickle
        torch.save({k: v.cpu() for k, v in self.net.state_dict().items()}, ckpt_filepath_maker(epoch_id))
        if use_ema:
            torch.save({k: v.cpu() for k, v in self.ema_net.state_dict().items()}, ckpt_filepath_maker(epoch_id, suffix="ema"))
        torch.save(torch.FloatTensor(losses), ckpt_filepath_maker(epoch_id, suffix="losses"))
        if losses_grad is not None:
            torch.save(torch.FloatTensor(losses_grad), ckpt_filepath_maker(epoch_id, suffix="losses_grad"))
        with open(ckpt_filepath_maker(epoch_id, suffix="diag"), "wb") as f:
            pickle.dump(diagnostics, f)

    def train(self, data, batch_size, n_epochs, reweight_loss=False, lr=3e-4, decay=0.0, clip_val=1.0, initial_n_warmup_mcmc_steps=1024,
              n_mcmc_steps=32, n_accumulation_steps=1, reg_val=0.0, use_ema=False, ema_decay=0.995, ema_steps=10, ckpt_interval=-1,
              ckpt_filepath_maker=None, verbose=True):
        """additions/ebm_mle.py:590-801.  Returns (losses, gradient norms, diagnostics), or (losses, diagnostics) with ``clip_val <= 0``."""
        cd = self.sampler_type == "cd"
        if cd and n_accumulation_steps != 1:
            raise ValueError("Can't use n_accumulation_steps != 1 if sampler_type is CD.")
        if cd and reweight_loss:
            raise NotImplementedError("Loss scaling not implemented with CD.")
        if self.sampler_type == "smc_pdds":
            raise NotImplementedError("sampler_type 'smc_pdds': the reference's branch reads an undefined x_init (additions/ebm_mle.py:487-503)")
        if self.sampler_type not in ("annealed_mcmc", "smc", "replica_exchange", "cd"):
            raise NotImplementedError("Sampler {} not found.".format(self.sampler_type))
        E.require_gpu(data)
        had = getattr(self.net, "param_grads", False)
        self.net.param_grads = True
        try:
            return self._train(data, batch_size, n_epochs, reweight_loss, lr, decay, clip_val, initial_n_warmup_mcmc_steps, n_mcmc_steps,
                               n_accumulation_steps, reg_val, use_ema, ema_decay, ema_steps, ckpt_interval, ckpt_filepath_maker, verbose)
        finally:
            self.net.param_grads = had

    def _train(self, data, batch_size, n_epochs, reweight_loss, lr, decay, clip_val, initial_n_warmup_mcmc_steps, n_mcmc_steps,
               n_accumulation_steps, reg_val, use_ema, ema_decay, ema_steps, ckpt_interval, ckpt_filepath_maker, verbose):
        cd, n_levels, dev = self.sampler_type == "cd", self.times.shape[0], self.times.device
        optimizer = (torch.optim.AdamW(self.net.parameters(), lr=lr, weight_decay=decay) if decay > 0
                     else torch.optim.Adam(self.net.parameters(), lr=lr))
        if self.perc_keep_mcmc > 0:
            n_warmup, n_kept = int((1.0 - self.perc_keep_mcmc) * n_mcmc_steps), int(self.perc_keep_mcmc * n_mcmc_steps)
        else:
            n_warmup, n_kept = n_mcmc_steps - 1, 1
        eff_bs = batch_size if cd else min(batch_size * n_kept, data.shape[0])
        loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data), batch_size=eff_bs, shuffle=True, drop_last=True)
        n_batches = len(loader)
        if use_ema:
            alpha = min(1.0, (1.0 - ema_decay) * (n_accumulation_steps * n_levels * eff_bs * ema_steps / n_epochs))
            self.ema_net = torch.optim.swa_utils.AveragedModel(self.net, multi_avg_fn=torch.optim.swa_utils.get_ema_multi_avg_fn(1.0 - alpha))
            self.ema_net.module.param_grads = False  # the copy is for evaluation: the switch is train's, on the net it trains
        data_shape, ones = data.shape[1:], (1,) * (data.dim() - 1)
        per_level = lambda b: self.times.reshape((-1, 1, *ones)).repeat((1, b, *ones))  # noqa: E731
        ts = per_level(eff_bs)
        if cd:
            ts_neg = per_level(min(batch_size * n_kept, data.shape[0])).view((-1, *ones))
        times_expanded = per_level(batch_size)
        mean_factor = self.sde.s(ts)
        std_factor = mean_factor * torch.sqrt(self.sde.sigma_sq(ts))
        ts = ts.view((-1, *ones))
        # initial step sizes: one per level and chain
        st = self.step_sizes_per_noise
        if isinstance(st, float) or (torch.is_tensor(st) and st.dim() == 0):
            self.step_sizes_per_noise = st * torch.ones((n_levels, batch_size, *ones), device=dev)
        elif st.dim() > 0:
            self.step_sizes_per_noise = st.flatten().unsqueeze(1).repeat((1, batch_size)).to(dev).view((n_levels, batch_size, *ones))
        else:
            raise ValueError("Wrong shape of step_sizes_per_noise.")
        if cd:
            self.step_sizes_per_noise = self.step_sizes_per_noise.view((-1, *ones))
        if self.use_precond and self.sampler_type in ("replica_exchange", "cd"):  # one matrix per level -> one per chain
            def per_chain(m):
                m = m.unsqueeze(1).repeat((1, batch_size, *ones, *ones))
                return m.view((-1, *data_shape, *data_shape)) if cd else m
            self.precond_matrix_per_noise = per_chain(self.precond_matrix_per_noise)
            self.precond_matrix_chol_per_noise = per_chain(self.precond_matrix_chol_per_noise)
        x_persist = None
        if self.sampler_type == "replica_exchange":  # persistent state of the replicas
            if self.net.has_sample_prior:
                t_rows = self.times.clone().reshape((-1, 1)).repeat((1, batch_size)).view((-1, 1))
                x_persist = self.net.sample_prior(t_rows).view((n_levels, batch_size, -1))
            else:
                x_persist = self.prior.sample((n_levels, batch_size,))
        if verbose:
            from tqdm import trange
            epochs = trange(n_epochs)
        else:
            epochs = range(n_epochs)
        losses, losses_grad, diagnostics = [], ([] if clip_val > 0 else None), []
        first_sampling, global_step = True, 0
        tail = n_batches % n_accumulation_steps  # batches of the last, shorter accumulation group
        for epoch_id in epochs:
            for batch_id, batch in enumerate(loader):
                samples = batch[0]
                xs_pos = (mean_factor * samples.unsqueeze(0) + std_factor * torch.randn_like(samples)).view((-1, *data_shape))
                fresh = batch_id % n_accumulation_steps == 0  # negatives (and their energies) are renewed once per accumulation group
                if epoch_id == 0 and batch_id == 0 and self.net.has_sample_prior:
                    xs_neg, diags = self.net.sample_prior(ts_neg if cd else ts), {}
                elif fresh:
                    warm = initial_n_warmup_mcmc_steps if first_sampling else n_warmup
                    if cd:
                        xs_neg, diags = self.cd_sampling(times_expanded=times_expanded, n_warmup_mcmc_steps=warm, n_mcmc_steps=n_kept,
                                                         xs_pos=xs_pos)
                        xs_neg = xs_neg.detach()
                    else:
                        xs_neg, diags = self.sample_model(batch_size=batch_size, times_expanded=times_expanded,
                                                          is_very_first_negative_sampling=first_sampling,
                                                          initial_n_warmup_mcmc_steps=initial_n_warmup_mcmc_steps, n_warmup_mcmc_steps=n_warmup,
                                                          n_mcmc_steps=n_kept, x_init_persistant=x_persist)
                        xs_neg = xs_neg.detach()
                        if x_persist is not None:
                            x_persist = xs_neg[:, -1]
                    first_sampling = False
                    diagnostics.append(diags)
                    xs_neg = xs_neg.reshape((-1, *data_shape))
                en_pos = self.net.energy(ts, xs_pos).flatten()
                if fresh:
                    en_neg = self.net.energy(ts_neg if cd else ts, xs_neg).flatten()
                if cd:
                    loss = en_pos.mean() - en_neg.mean()
                else:
                    scale = 1.0 / self.sde.sigma_sq(ts).flatten() if reweight_loss else 1.0
                    loss = (scale * (en_pos - en_neg)).mean()
                if reg_val > 0:
                    loss = loss + reg_val * (torch.square(en_pos).mean() + torch.square(en_neg).mean())
                loss = loss / (tail if batch_id >= n_batches - tail else n_accumulation_steps)  # the group's average
                bad = "NaN loss detected." if torch.isnan(loss).any() else (
                    "Training diverged (loss = {:.2e}).".format(loss.item()) if loss.abs().item() > 1e9 else None)
                if bad:
                    self.save_logs(losses, losses_grad, diagnostics, use_ema, epoch_id, ckpt_filepath_maker)
                    raise RuntimeError(bad)
                losses.append(loss.item())
                loss.backward(retain_graph=n_accumulation_steps > 1)
                infos = {"loss": losses[-1]}
                if clip_val > 0:
                    losses_grad.append(torch.nn.utils.clip_grad_norm_(self.net.parameters(), clip_val).item())
                    infos["norm_grad_loss"] = losses_grad[-1]
                if verbose:
                    epochs.set_postfix(**infos, **{k: float(v.cpu().mean().item()) for k, v in diags.items()})
                if (batch_id + 1) % n_accumulation_steps == 0 or batch_id + 1 == n_batches:
                    optimizer.step()
                    global_step += 1
                    if use_ema and global_step % ema_steps == 0:
                        self.ema_net.update_parameters(self.net)
                    optimizer.zero_grad()
            if ckpt_interval > 0 and epoch_id % ckpt_interval == 0:
                self.save_logs(losses, losses_grad, diagnostics, use_ema, epoch_id, ckpt_filepath_maker)
        if clip_val > 0:
            return torch.FloatTensor(losses), torch.FloatTensor(losses_grad), diagnostics
        return torch.FloatTensor(losses), diagnostics

    def _apply(self, fn):
        new_self = super()._apply(fn)
        new_self.sde = new_self.sde._apply(fn)
        new_self.prior._apply(fn)
        new_self.net = new_self.net._apply(fn)
        return new_self
