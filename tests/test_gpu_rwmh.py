"""sdeng_rwmh_moves on the GPU: all random-walk Metropolis moves of all chains in one launch against the move-by-move host composition,
the edge shapes, the in-kernel Philox noise, the sampled law, the routing of mcmc_sample(mcmc_type='rwmh') and the run_smc_sampler /
run_re_sampler entry points."""
import math

import pytest
import torch

from tests import golden_cases as gc
from tests import rwmh_cases as rc
from tests.cpu_generator import CpuGenerator

FLIP = 1e-3  # a chain whose accept / reject decision fell within round-off of its threshold differs by a whole proposal: max|dx| > 1e-3


def _host_arm(target, x0, lp0, step0, n_moves, target_acceptance):
    """mcmc.rwmh_step + heuristics_step_size over sdeng_dist_eval log-densities -> (states after every move, x, lp, step)."""
    from sde_sampler_lrds_amd import engine as E
    from sde_sampler_lrds_amd.additions import mcmc
    x, lp, step = x0.clone(), lp0.clone(), step0.clone().view(-1, 1)
    xs = []
    for _ in range(n_moves):
        x, lp, log_acc = mcmc.rwmh_step(x, lp, lambda v: E.dist_eval(target, v, want_score=False)[0], step)
        if target_acceptance > 0.0:
            step = mcmc.heuristics_step_size(step, log_acc, target_acceptance=target_acceptance)
        xs.append(x.clone())
    return torch.stack(xs) if xs else x0.new_empty(0, *x0.shape), x, lp, step.reshape(-1)


def _compare(tag, target, x0, step0, n_moves, target_acceptance, max_flipped, keep_from=0, seed=11):
    """Both arms from the same state with the same torch noise; the criteria of test_native_langevin_moves_equal_the_host_composition."""
    from sde_sampler_lrds_amd import engine as E
    B, d = x0.shape
    lp0 = E.dist_eval(target, x0, want_score=False)[0].flatten()
    torch.manual_seed(seed)
    xs_ref, x_ref, lp_ref, step_ref = _host_arm(target, x0, lp0, step0, n_moves, target_acceptance)
    torch.manual_seed(seed)
    xn, lpn, stn = x0.clone(), lp0.clone(), step0.reshape(-1).clone()
    got, acc, last = E.rwmh_moves(target, xn, lpn, stn, n_moves, keep_from=keep_from, target_acceptance=target_acceptance)
    assert got.shape == (n_moves - keep_from, B, d) and acc.shape == (B,) and last.shape == (B,)
    err = (got - xs_ref[keep_from:]).abs().amax(dim=(0, 2)) if keep_from < n_moves else torch.zeros(B, device=x0.device)
    err = torch.maximum(err, (xn - x_ref).abs().amax(dim=1))
    same = err <= FLIP
    flipped = int((~same).sum())
    finite = torch.isfinite(lp_ref)
    dx = float(err[same].max())
    dstep = float((stn - step_ref)[same].abs().max())
    dlp = float((lpn - lp_ref)[same & finite].abs().max()) if bool((same & finite).any()) else 0.0
    print(f"{tag}: {flipped} of {B} chains flipped a decision; same-decision chains: max |dx| {dx:.2e}, |dstep| {dstep:.2e}, |dlp| {dlp:.2e}; "
          f"chains with a non-finite lp {int((~finite).sum())}")
    assert flipped <= max_flipped
    assert dx < 2e-5 and dstep < 1e-7 and dlp < 1e-3
    assert torch.equal(torch.isfinite(lpn)[same], finite[same]) and torch.equal(lpn[same & ~finite], lp_ref[same & ~finite])  # (-inf stays -inf)
    if keep_from < n_moves:
        assert torch.equal(got[-1], xn)
    return got, acc, last


def _gmm24(gpu):
    from sde_sampler_lrds_amd.distr.gauss import GMM
    g = torch.Generator().manual_seed(4)
    d = 24
    return GMM(dim=d, loc=2.0 * torch.randn(3, d, generator=g), scale=0.5 + 0.3 * torch.rand(3, d, generator=g),
               mixture_weights=torch.tensor([0.5, 0.3, 0.2])).to(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("target_acceptance", [0.75, 0.0])
@pytest.mark.parametrize("tname", ["rings", "checkerboard", "gmm24"])
def test_one_launch_equals_the_host_composition(gpu, tname, target_acceptance):
    """600 chains, 16 moves, per-chain step sizes, adaptation on and off: at most 2 chains flip a decision, the others agree to round-off.
    The checkerboard's chains include 32 that start outside every square (lp = -inf), a few hundredths from one, so that some walk in.
    Step sizes are those of the MALA test (0.02 .. 0.07): the 1e-7 on the adapted step is absolute, and torch on the GPU divides by the
    scalar 1.01 through its reciprocal where the kernel -- and the reference's CPU run -- divides, so the arms may part by an ulp per
    shrink; 16 ulps of a step below 0.09 are 1.2e-7, two or three (what a run shows) 2e-8."""
    from sde_sampler_lrds_amd.distr.checkerboard import Checkerboard
    from sde_sampler_lrds_amd.distr.rings import Rings
    torch.manual_seed(5)
    B = 600
    step0 = 0.02 + 0.05 * torch.rand(B, device=gpu)
    if tname == "rings":
        target = Rings(dim=2, n_reference_samples=10).to(gpu)
        x0 = 3.0 * torch.randn(B, 2, device=gpu)
    elif tname == "checkerboard":
        target = Checkerboard().to(gpu)
        x0 = target.sample((B,)).float().contiguous()
        u = torch.rand(32, 2, device=gpu)  # left of the square [-2, 0] x [2, 4], in the empty cell [-4, -2] x [2, 4]
        x0[:32] = torch.stack([-2.0 - 0.03 * u[:, 0] - 1e-4, 2.2 + 1.6 * u[:, 1]], dim=-1)
    else:
        target = _gmm24(gpu)
        x0 = 2.0 * torch.randn(B, 24, device=gpu)
    _, acc, _ = _compare(f"{tname} acc={target_acceptance}", target, x0, step0, 16, target_acceptance, max_flipped=2)
    print(f"{tname}: mean acceptance {float(acc.mean()) / 16:.3f}; chains with a rejection {int((acc < 16).sum())}, with an acceptance {int((acc > 0).sum())}")
    assert int((acc < 16).sum()) >= 20 and int((acc > 0).sum()) >= 20  # both decisions were taken


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("d", [1, 3, 5, 255])
def test_edge_shapes(gpu, d, B):
    """d around the four-wide noise loop and at the LDS bound, B below / above one block's 64 chains, keep_from at both ends.  With at most
    65 chains the cap of 2 flips in 600 leaves room for none.  Targets of width ~0.1 with steps of 0.02 .. 0.06 / sqrt(d) -- a third of the
    width, so that moves are rejected and steps shrink -- keep the adapted step where 1e-7 absolute is several ulps (see above)."""
    from sde_sampler_lrds_amd.distr.gauss import Gauss, IsotropicGauss
    g = torch.Generator().manual_seed(100 * d + B)
    targets = [IsotropicGauss(dim=d, scale=0.13).to(gpu),
               Gauss(dim=d, loc=0.05 * torch.randn(d, generator=g), scale=0.07 + 0.06 * torch.rand(d, generator=g)).to(gpu)]
    x0 = (0.15 * torch.randn(B, d, generator=g)).to(gpu)
    step0 = ((0.02 + 0.04 * torch.rand(B, generator=g)) / math.sqrt(d)).to(gpu)
    for ti, target in enumerate(targets):
        for keep_from in (0, 2, 4):
            got, _, _ = _compare(f"d={d} B={B} target {ti} keep_from={keep_from}", target, x0, step0, 4, 0.75, max_flipped=0, keep_from=keep_from)
            assert got.shape == (4 - keep_from, B, d)


def _philox_run(target, x0, step, n_moves, seed, chain0=0, keep_from=0, target_acceptance=0.0, want_samples=True):
    from sde_sampler_lrds_amd import engine as E
    x = x0.clone()
    lp = E.dist_eval(target, x, want_score=False)[0].flatten().contiguous()
    st = torch.full((x.shape[0],), step, device=x.device)
    got, acc, last = E.rwmh_moves(target, x, lp, st, n_moves, keep_from=keep_from, target_acceptance=target_acceptance, noise="philox", seed=seed,
                                  chain0=chain0, want_samples=want_samples)
    return got, acc, last, x, lp, st


@pytest.mark.gpu
def test_philox_noise_is_reproducible_and_independent_of_the_split(gpu):
    target = _gmm24(gpu)
    B = 130
    x0 = 2.0 * torch.randn(B, 24, generator=torch.Generator().manual_seed(1)).to(gpu)
    a = _philox_run(target, x0, 0.1, 12, seed=77, target_acceptance=0.75)
    b = _philox_run(target, x0, 0.1, 12, seed=77, target_acceptance=0.75)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    h = B // 2
    lo = _philox_run(target, x0[:h].contiguous(), 0.1, 12, seed=77, chain0=0, target_acceptance=0.75)
    hi = _philox_run(target, x0[h:].contiguous(), 0.1, 12, seed=77, chain0=h, target_acceptance=0.75)
    for full, p, q in zip(a, lo, hi):
        assert torch.equal(full, torch.cat([p, q], dim=1 if full.dim() == 3 else 0))
    c = _philox_run(target, x0, 0.1, 12, seed=78, target_acceptance=0.75)
    assert not torch.equal(a[3], c[3])
    assert 0.02 < float(a[1].mean()) / 12 < 0.98


@pytest.mark.gpu
def test_philox_normals_are_stream_6_of_the_step_noise(gpu):
    """On a target so wide that every proposal is accepted, x_K - x_0 = step * sum_m z_m with z from sdeng_philox_normal_steps(stream_id=6)."""
    from sde_sampler_lrds_amd import _lib as L
    from sde_sampler_lrds_amd import engine as E
    from sde_sampler_lrds_amd.distr.gauss import IsotropicGauss
    B, d, K, seed, chain0 = 300, 5, 8, 1234, 40
    target = IsotropicGauss(dim=d, scale=1e6).to(gpu)
    x0 = torch.randn(B, d, generator=torch.Generator().manual_seed(2)).to(gpu)
    got, acc, _, x, _, st = _philox_run(target, x0, 0.5, K, seed=seed, chain0=chain0)
    z = torch.empty(K, B, d, dtype=torch.float32, device=gpu)
    L.check(L.lib().sdeng_philox_normal_steps(seed, 0, K, chain0, B, d, 6, z.data_ptr(), E._stream_ptr(gpu)))
    want = x0.clone()
    for m in range(K):
        want = want + 0.5 * z[m]
    all_accepted = acc == float(K)
    print(f"philox replay: {int(all_accepted.sum())} of {B} chains accepted every move; max |dx| {float((x - want)[all_accepted].abs().max()):.2e}")
    assert int(all_accepted.sum()) >= math.ceil(0.99 * B)
    assert float((x - want)[all_accepted].abs().max()) < 1e-5
    assert torch.equal(st, torch.full((B,), 0.5, device=gpu))  # adaptation off


@pytest.mark.gpu
def test_the_sampler_samples_a_gaussian(gpu):
    """4096 chains from zero, 512 moves at fixed step 0.8 on N(0, 1.5^2 I_4): the pooled final states (16384 values) have mean within 0.06
    (five standard errors of 0.012) and variance within 5 % of 2.25 (standard error 1.1 %)."""
    from sde_sampler_lrds_amd.distr.gauss import IsotropicGauss
    target = IsotropicGauss(dim=4, scale=1.5).to(gpu)
    K = 512
    _, acc, _, x, _, _ = _philox_run(target, torch.zeros(4096, 4, device=gpu), 0.8, K, seed=9, want_samples=False)
    mean, var, rate = float(x.mean()), float(x.var()), float(acc.mean()) / K
    print(f"rwmh on N(0, 2.25 I): mean {mean:+.4f}, variance {var:.4f}, mean acceptance {rate:.3f}")
    assert abs(mean) < 0.06 and abs(var - 2.25) < 0.05 * 2.25 and 0.2 < rate < 0.9


def _per_chain(samples, n_chains):
    return samples.view(-1, n_chains, samples.shape[-1])


@pytest.mark.gpu
def test_mcmc_sample_takes_the_native_route_on_the_checkerboard(gpu):
    from sde_sampler_lrds_amd.additions import ebm_mle
    from sde_sampler_lrds_amd.distr.checkerboard import Checkerboard
    from sde_sampler_lrds_amd.experiments.benchmark_utils import mcmc_sample
    target = Checkerboard()
    kw = dict(mcmc_type="rwmh", n_chains_per_mode=16, dataset_length=4096, n_warmup_steps=64, shuffle=False)
    n_chains = target.loc.shape[0] * 16
    calls = ebm_mle._native_calls[0]
    torch.manual_seed(21)
    native = mcmc_sample(gpu, target, target.loc, **kw)
    assert ebm_mle._native_calls[0] == calls + 1
    assert native.shape == (4096 // n_chains * n_chains, 2) and native.device.type == "cpu"
    assert bool(torch.isfinite(Checkerboard().unnorm_log_prob(native)).all())
    ebm_mle.NATIVE_MOVES = False
    try:
        torch.manual_seed(21)
        host = mcmc_sample(gpu, target, target.loc, **kw)
    finally:
        ebm_mle.NATIVE_MOVES = True
    assert ebm_mle._native_calls[0] == calls + 1 and host.shape == native.shape
    err = (_per_chain(native, n_chains) - _per_chain(host, n_chains)).abs().amax(dim=(0, 2))
    flipped = int((err > FLIP).sum())
    print(f"mcmc_sample rwmh, native vs host loop: {flipped} of {n_chains} chains flipped; max |dx| of the others {float(err[err <= FLIP].max()):.2e}")
    assert flipped * 600 <= 2 * n_chains and float(err[err <= FLIP].max()) < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.RWMH_CASES)
def test_rwmh_fixtures_through_the_native_route(gpu, name):
    """The reference's own chains (tests/golden/rwmh_*.npz), reproduced by ONE launch fed the CPU generator's numbers in the reference's order."""
    from sde_sampler_lrds_amd.additions import ebm_mle
    from sde_sampler_lrds_amd.experiments.benchmark_utils import mcmc_sample
    from tests.test_rwmh_cpu import _rwmh_target
    c = gc.load(name)
    m = c.meta
    target = _rwmh_target(m)
    n_chains = m["n_init"] * m["n_chains_per_mode"]
    calls = ebm_mle._native_calls[0]
    x_init = rc.rwmh_x_init(m, target)  # (outside the patch: it draws from a generator of its own)
    torch.manual_seed(m["seed"])
    with CpuGenerator():
        out = mcmc_sample(gpu, target, x_init, **rc.rwmh_kwargs(m))
    assert ebm_mle._native_calls[0] == calls + 1 and out.shape == c["samples"].shape
    err = (_per_chain(out, n_chains) - _per_chain(c["samples"], n_chains)).abs().amax(dim=(0, 2))
    flipped = int((err > FLIP).sum())
    print(f"{name}: {flipped} of {n_chains} chains flipped; max |dx| of the others {float(err[err <= FLIP].max()):.2e}")
    assert flipped * 600 <= 2 * n_chains and float(err[err <= FLIP].max()) < 2e-5


def _three_modes(gpu):
    from sde_sampler_lrds_amd.distr.gauss import GMM
    loc = torch.tensor([[3.0, 0, 0, 0], [-3.0, 0, 0, 0], [0, 3.0, 0, 0]])
    wts = torch.tensor([0.5, 0.3, 0.2])
    return GMM(dim=4, loc=loc, scale=0.6 * torch.ones(3, 4), mixture_weights=wts.clone()).to(gpu), loc, wts


@pytest.mark.gpu
def test_run_smc_sampler_takes_native_moves_and_recovers_the_mode_weights(gpu):
    """The 3-mode mixture of test_native_moves_with_in_kernel_noise_sample_the_target through the reference's entry point: the bound
    unnorm_log_prob resolves to the mixture, so the levels run as native moves from N(0, 9 I)."""
    from sde_sampler_lrds_amd.additions import ebm_mle
    from sde_sampler_lrds_amd.experiments.benchmark_utils import run_smc_sampler
    torch.manual_seed(0)
    target, loc, wts = _three_modes(gpu)
    B, calls = 8192, ebm_mle._native_calls[0]
    out = run_smc_sampler(torch.zeros(4, device=gpu), 9.0 * torch.ones(4, device=gpu), n_steps=12, step_size=0.05, n_particles=B, n_mcmc_steps=4,
                          n_warmup_mcmc_steps=8, target_log_prob=target.unnorm_log_prob, target_score=target.score)
    assert ebm_mle._native_calls[0] == calls + 12 and out.shape == (4, B, 4) and out.is_cuda
    frac = torch.bincount(torch.cdist(out[-1], loc.to(gpu)).argmin(dim=1), minlength=3).float() / B
    print("run_smc_sampler mode fractions", frac.tolist())
    assert float((frac.cpu() - wts).abs().max()) < 0.05


@pytest.mark.gpu
def test_run_re_sampler_takes_native_moves(gpu):
    from sde_sampler_lrds_amd.additions import ebm_mle
    from sde_sampler_lrds_amd.experiments.benchmark_utils import run_re_sampler
    torch.manual_seed(1)
    target, _, _ = _three_modes(gpu)
    cov = 9.0 * torch.eye(4, device=gpu) + 0.5 * torch.ones(4, 4, device=gpu)  # a full-covariance prior
    calls = ebm_mle._native_calls[0]
    out = run_re_sampler(torch.zeros(4, device=gpu), cov, n_steps=6, step_size=0.05, batch_size=512, swap_frequency=4, n_mcmc_steps=4,
                         n_warmup_mcmc_steps=8, target_log_prob=target.unnorm_log_prob, target_score=target.score)
    assert ebm_mle._native_calls[0] > calls
    assert out.shape == (4, 512, 4) and bool(torch.isfinite(out).all())  # the target level: [n_mcmc_steps, batch_size, d]
    assert out[-1].shape == (512, 4)


@pytest.mark.gpu
def test_run_smc_sampler_on_the_checkerboard_composes_on_the_host(gpu):
    """The one-launch moves refuse the checkerboard, so its path is the reference's closure over sdeng_dist_eval and the moves are composed
    on the host.  The closure keeps the reference's arithmetic: at the prior's level 0 * (-inf) is NaN for a particle outside every
    square, which then never moves (and no level resamples).  The prior therefore sits on a square -- N((-1, 3), 0.09 I), 3.3 standard
    deviations from its edges -- and the particles spread over it as the levels approach the target."""
    from sde_sampler_lrds_amd.additions import ebm_mle
    from sde_sampler_lrds_amd.distr.checkerboard import Checkerboard
    from sde_sampler_lrds_amd.experiments.benchmark_utils import run_smc_sampler
    torch.manual_seed(2)
    target = Checkerboard().to(gpu)
    calls = ebm_mle._native_calls[0]
    out = run_smc_sampler(torch.tensor([-1.0, 3.0], device=gpu), 0.09 * torch.ones(2, device=gpu), n_steps=8, step_size=0.02, n_particles=512,
                          n_mcmc_steps=2, n_warmup_mcmc_steps=4, target_log_prob=target.unnorm_log_prob, target_score=target.score)
    assert ebm_mle._native_calls[0] == calls
    assert out.shape == (2, 512, 2)
    inside = torch.isfinite(target.unnorm_log_prob(out.reshape(-1, 2))).float().mean()
    print(f"run_smc_sampler on the checkerboard: {float(inside):.3f} of the samples inside a square")
    assert float(inside) >= 0.9
