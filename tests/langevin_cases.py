"""Inputs of the Langevin-move edge-shape tests (tests/test_gpu_langevin_moves.py) and the CPU check of their seeds
(tests/test_langevin_moves_cpu.py).  Every input comes from a seeded CPU generator, and the moves' random numbers from torch's global CPU
generator (tests/cpu_generator.py on the GPU), so the chains of a case are the same on both sides."""
import torch

EDGE_D = (1, 3, 5, 120, 255)  # around the four-wide noise loop; 120: 32 chains per block; 255: 16 chains per block, the LDS bound
EDGE_B = (1, 3, 65)           # below / above one block's 64 chains
N_MOVES = 4
MARGIN = 1e-3                 # the smallest |log u - log_acc| a case's seed must leave, in float32 torch on the CPU
# seed of each (d, B): chosen on the CPU so that no accept / reject decision of the MALA chains is within MARGIN of its threshold -- the
# one-launch kernel and the host composition round differently, and a decision that close may flip
SEEDS = {(1, 1): 1010, (1, 3): 1030, (1, 65): 1654, (3, 1): 3010, (3, 3): 3030, (3, 65): 3674, (5, 1): 5010, (5, 3): 5030, (5, 65): 5660,
         (120, 1): 120010, (120, 3): 120030, (120, 65): 120651, (255, 1): 255010, (255, 3): 255030, (255, 65): 255660}


def mixture_near_samples(d, B, g):
    """A two-component diagonal mixture of moderate width and B points drawn from it (generator g): log-densities stay O(d), so
    float32 resolves the acceptance ratio well below MARGIN."""
    from sde_sampler_lrds_amd.distr.gauss import GMM
    loc, scale = 0.8 * torch.randn(2, d, generator=g), 0.5 + 0.3 * torch.rand(2, d, generator=g)
    comp = (torch.rand(B, generator=g) < 0.4).long()
    x0 = loc[comp] + scale[comp] * torch.randn(B, d, generator=g)
    return GMM(dim=d, loc=loc, scale=scale, mixture_weights=torch.tensor([0.6, 0.4])), x0


def edge_inputs(d, B, seed):
    """-> target, prior, x0 [B,d], per-chain tempering weights [B,1], per-chain step sizes [B,1] (all on the CPU)."""
    from sde_sampler_lrds_amd.distr.gauss import IsotropicGauss
    g = torch.Generator().manual_seed(seed)
    target, x0 = mixture_near_samples(d, B, g)
    return target, IsotropicGauss(dim=d, scale=1.5), x0, torch.rand(B, 1, generator=g), 0.02 + 0.05 * torch.rand(B, 1, generator=g)


def torch_path(target, prior):
    """ebm_mle.hip_tempered_log_prob_and_grads with the distributions' own torch log-density and score."""
    def fn(t, x):
        w = t.to(x.dtype).expand(x.shape[0], 1)
        lp = (1.0 - w) * prior.unnorm_log_prob(x) + w * target.unnorm_log_prob(x)
        return lp.flatten(), (1.0 - w) * prior.score(x) + w * target.score(x)
    return fn


def host_chain(f, t, x0, step0, n_moves, use_ula, target_acceptance=0.75, margins=None):
    """mcmc.mala_step / ula_step + heuristics_step_size over the path f -> (states after every move [n_moves,B,d], x, lp, grad, step [B]).
    ``margins`` (a list, CPU only) receives |log u - log_acc| of every decision."""
    from sde_sampler_lrds_amd.additions import mcmc
    x, step = x0.clone(), step0.clone().view(-1, 1)
    lp, grad = f(t, x)
    xs = []
    for _ in range(n_moves):
        if use_ula:
            x, lp, grad = mcmc.ula_step(x, lp, grad, lambda y: f(t, y), step)
        else:
            before = torch.get_rng_state()
            x, lp, grad, log_acc = mcmc.mala_step(x, lp, grad, lambda y: f(t, y), step)
            if margins is not None:  # replay the move's draws: randn((B, d)) for the proposal, then the uniforms of the accept test
                after = torch.get_rng_state()
                torch.set_rng_state(before)
                torch.randn(x.shape)
                margins.append((torch.log(torch.rand(x.shape[0])) - log_acc).abs())
                torch.set_rng_state(after)
            step = mcmc.heuristics_step_size(step, log_acc, target_acceptance=target_acceptance)
        xs.append(x.clone())
    return torch.stack(xs), x, lp, grad, step.reshape(-1)
