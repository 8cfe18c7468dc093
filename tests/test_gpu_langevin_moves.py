"""The Langevin instantiation of the chain-move kernel (sdeng_langevin_moves) at its edge shapes, against the move-by-move host composition,
and its in-kernel Philox noise.  tests/test_make_model_gpu.py holds the 600-chain case and the samplers; tests/test_gpu_rwmh.py the same
shapes for the random-walk Metropolis instantiation."""
import pytest
import torch

from tests import langevin_cases as lc
from tests.cpu_generator import CpuGenerator

FLIP = 1e-3  # a chain whose accept / reject decision flipped differs by a whole proposal: max|dx| > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("use_ula", [False, True])
@pytest.mark.parametrize("B", lc.EDGE_B)
@pytest.mark.parametrize("d", lc.EDGE_D)
def test_edge_shapes(gpu, d, B, use_ula):
    """MALA with a prior and per-chain tempering weights, and ULA, 4 moves, keep_from at both ends and between, torch noise: the criteria of
    test_native_langevin_moves_equal_the_host_composition, with no flipped chain -- the seed of each shape leaves every decision
    lc.MARGIN from its threshold (tests/test_langevin_moves_cpu.py checks that on the CPU)."""
    from sde_sampler_lrds_amd import engine as E
    from sde_sampler_lrds_amd.additions import ebm_mle
    seed = lc.SEEDS[d, B]
    target, prior, x0, t, step0 = (v.to(gpu) for v in lc.edge_inputs(d, B, seed))
    f = ebm_mle.hip_tempered_log_prob_and_grads(target, prior)
    acc_target = 0.0 if use_ula else 0.75
    with CpuGenerator():
        torch.manual_seed(seed)
        xs_ref, x_ref, lp_ref, _, step_ref = lc.host_chain(f, t, x0, step0, lc.N_MOVES, use_ula)
        for keep_from in (0, 2, 4):
            torch.manual_seed(seed)
            xn = x0.clone()
            lpn, gn = f(t, xn)
            lpn, gn, stn = lpn.contiguous().clone(), gn.contiguous().clone(), step0.reshape(-1).clone()
            got, acc, last = E.langevin_moves(target, prior, xn, lpn, gn, stn, lc.N_MOVES, t=t.reshape(-1), keep_from=keep_from, unadjusted=use_ula,
                                              target_acceptance=acc_target)
            assert got.shape == (lc.N_MOVES - keep_from, B, d)
            assert (acc is None and last is None) if use_ula else (acc.shape == (B,) and last.shape == (B,))
            err = (xn - x_ref).abs().amax(dim=1)
            if keep_from < lc.N_MOVES:
                err = torch.maximum(err, (got - xs_ref[keep_from:]).abs().amax(dim=(0, 2)))
                assert torch.equal(got[-1], xn)
            same = err <= FLIP
            dx, dstep, dlp = float(err[same].max()), float((stn - step_ref)[same].abs().max()), float((lpn - lp_ref)[same].abs().max())
            print(f"{'ULA' if use_ula else 'MALA'} d={d} B={B} keep_from={keep_from}: {int((~same).sum())} of {B} chains flipped a decision; "
                  f"max |dx| {dx:.2e}, |dstep| {dstep:.2e}, |dlp| {dlp:.2e}")
            assert bool(same.all())
            assert dx < 2e-5 and dstep < 1e-7


def _gmm24(gpu, B):
    """The 3-component mixture of tests/test_gpu_rwmh.py, B points drawn from it, an N(0, 2.5^2 I) prior and per-chain tempering weights."""
    from sde_sampler_lrds_amd.distr.gauss import GMM, IsotropicGauss
    g = torch.Generator().manual_seed(4)
    d = 24
    loc, scale = 2.0 * torch.randn(3, d, generator=g), 0.5 + 0.3 * torch.rand(3, d, generator=g)
    comp = torch.randint(3, (B,), generator=g)
    x0 = loc[comp] + scale[comp] * torch.randn(B, d, generator=g)
    target = GMM(dim=d, loc=loc, scale=scale, mixture_weights=torch.tensor([0.5, 0.3, 0.2]))
    return target.to(gpu), IsotropicGauss(dim=d, scale=2.5).to(gpu), x0.to(gpu), torch.rand(B, 1, generator=g).to(gpu)


def _philox_run(target, prior, x0, t, step, n_moves, seed, chain0=0):
    from sde_sampler_lrds_amd import engine as E
    from sde_sampler_lrds_amd.additions import ebm_mle
    x = x0.clone()
    lp, grad = ebm_mle.hip_tempered_log_prob_and_grads(target, prior)(t, x)
    lp, grad = lp.contiguous().clone(), grad.contiguous().clone()
    st = torch.full((x.shape[0],), step, device=x.device)
    got, acc, last = E.langevin_moves(target, prior, x, lp, grad, st, n_moves, t=t.reshape(-1), target_acceptance=0.75, noise="philox", seed=seed,
                                      chain0=chain0)
    return got, acc, last, x, lp, grad, st


@pytest.mark.gpu
def test_philox_noise_is_reproducible_and_independent_of_the_split(gpu):
    """As the test of this name in tests/test_gpu_rwmh.py, for MALA (Philox streams 2 / 3): 130 chains are two full blocks and a third."""
    B = 130
    target, prior, x0, t = _gmm24(gpu, B)
    a = _philox_run(target, prior, x0, t, 0.05, 12, seed=77)
    b = _philox_run(target, prior, x0, t, 0.05, 12, seed=77)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    h = B // 2
    lo = _philox_run(target, prior, x0[:h].contiguous(), t[:h].contiguous(), 0.05, 12, seed=77, chain0=0)
    hi = _philox_run(target, prior, x0[h:].contiguous(), t[h:].contiguous(), 0.05, 12, seed=77, chain0=h)
    for full, p, q in zip(a, lo, hi):
        assert torch.equal(full, torch.cat([p, q], dim=1 if full.dim() == 3 else 0))
    c = _philox_run(target, prior, x0, t, 0.05, 12, seed=78)
    assert not torch.equal(a[3], c[3])
