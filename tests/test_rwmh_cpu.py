"""Random-walk Metropolis moves in one launch (sdeng_rwmh_moves) and the run_smc_sampler / run_re_sampler entry points, without a GPU:
every refusal of the C entry point (validation comes before any HIP call, so nothing is launched), the shape checks
of engine.rwmh_moves, and the host paths against the reference's own output (tests/golden/rwmh_*.npz, run_*_d3.npz)."""
import ctypes

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from tests import golden_cases as gc
from tests import rwmh_cases as rc
from tests.test_dispatch_cpu import P, _dist


def _call(kind=L.DIST_CHECKERBOARD, target=True, B=8, d=2, n_moves=4, keep_from=0, x=P, lp=P, step=P, z=None, u=None, ws=None, ws_bytes=0):
    lib = L.lib()
    ds = L.Dist()
    _dist(ds, kind)
    rc_ = lib.sdeng_rwmh_moves(ctypes.byref(ds) if target else None, B, d, n_moves, keep_from, 0.75, x, lp, step, z, u, 1, 0, None, None, None,
                               ws, ws_bytes, None)
    return rc_, lib.sdeng_last_error().decode()


@pytest.mark.parametrize("kw", [dict(target=False), dict(x=None), dict(lp=None), dict(step=None), dict(B=-1), dict(d=0), dict(n_moves=-1),
                                dict(keep_from=-1), dict(keep_from=5), dict(z=P), dict(u=P)])
def test_invalid_arguments_are_refused_before_any_launch(kw):
    code, msg = _call(**kw)
    assert code == L.E_INVALID, (kw, code, msg)


def test_refusals_and_the_workspace_stop():
    code, msg = _call(kind=L.DIST_GMM_DIAG, d=256)
    assert code == L.E_UNSUPPORTED and "d <= 255" in msg and "256" in msg
    code, msg = _call(kind=L.DIST_CHECKERBOARD, d=3)  # the target is validated before anything runs
    assert code == L.E_INVALID and "two-dimensional" in msg
    code, msg = _call(kind=L.DIST_NONE)
    assert code == L.E_INVALID
    assert _call(B=0)[0] == 0 and _call(n_moves=0)[0] == 0  # nothing to do: no workspace needed
    # a valid call stops at the workspace: NULL, or shorter than sdeng_rwmh_moves_workspace_bytes
    for kind, d in ((L.DIST_CHECKERBOARD, 2), (L.DIST_RINGS, 2), (L.DIST_GMM_DIAG, 24), (L.DIST_ISO_GAUSS, 255), (L.DIST_GAUSS_DIAG, 5)):
        ds = L.Dist()
        _dist(ds, kind)
        need = L.lib().sdeng_rwmh_moves_workspace_bytes(ctypes.byref(ds), d)
        assert need >= 256
        for z, u in ((None, None), (P, P)):
            code, msg = _call(kind=kind, d=d, z=z, u=u, keep_from=4)
            assert code == L.E_WORKSPACE and str(need) in msg, (kind, d, code, msg)
        code, msg = _call(kind=kind, d=d, ws=P, ws_bytes=need - 1)
        assert code == L.E_WORKSPACE and str(need - 1) in msg and str(need) in msg
    assert L.lib().sdeng_rwmh_moves_workspace_bytes(None, 2) == 0


def test_engine_rwmh_moves_checks_what_the_kernel_indexes(monkeypatch):
    from sde_sampler_lrds_amd.distr.gauss import IsotropicGauss
    monkeypatch.setattr(E, "require_gpu", lambda x: None)
    monkeypatch.setattr(E, "_stream_ptr", lambda device: None)
    target = IsotropicGauss(dim=3, scale=1.0)
    B, d = 6, 3
    x, lp, step = torch.zeros(B, d), torch.zeros(B), torch.ones(B)
    with pytest.raises(ValueError, match=r"x must be \[B, d\]"):
        E.rwmh_moves(target, torch.zeros(B, d, 1), lp, step, 4)
    with pytest.raises(ValueError, match=r"x must be \[B, d\]"):
        E.rwmh_moves(target, torch.zeros(B), lp, step, 4)
    with pytest.raises(ValueError, match="one value per chain"):
        E.rwmh_moves(target, x, torch.zeros(B - 1), step, 4)
    with pytest.raises(ValueError, match="one value per chain"):
        E.rwmh_moves(target, x, lp, torch.ones(B, 2), 4)
    for keep_from in (-1, 5):
        with pytest.raises(ValueError, match="keep_from"):
            E.rwmh_moves(target, x, lp, step, 4, keep_from=keep_from)
    with pytest.raises(ValueError, match="noise"):
        E.rwmh_moves(target, x, lp, step, 4, noise="numpy")
    with pytest.raises(ValueError, match="lp must be a contiguous float32"):
        E.rwmh_moves(target, x, lp.double(), step, 4)
    with pytest.raises(ValueError, match="x must be a contiguous float32"):
        E.rwmh_moves(target, torch.zeros(d, B).T, lp, step, 4)
    with pytest.raises(ValueError, match="x must be a contiguous float32 CUDA"):  # well-formed host tensors: still no launch
        E.rwmh_moves(target, x, lp, step, 4)
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="MI355X"):
        E.rwmh_moves(target, x, lp, step, 4)


def _rwmh_target(m):
    from sde_sampler_lrds_amd.distr.checkerboard import Checkerboard
    from sde_sampler_lrds_amd.distr.rings import Rings
    return Rings(dim=2, n_reference_samples=10) if m["target"] == "rings" else Checkerboard(dim=2, width=4)


@pytest.mark.parametrize("name", rc.RWMH_CASES)
def test_rwmh_data_set_matches_the_reference_fixture(name):
    """mcmc_sample(mcmc_type='rwmh') on the CPU (the host loop): same inputs, same seed of torch's global generator, same consumption
    order -> the reference's chains; 1e-5 as test_annealed_samplers_match_reference_fixture."""
    from sde_sampler_lrds_amd.experiments.benchmark_utils import mcmc_sample
    c = gc.load(name)
    m = c.meta
    target = _rwmh_target(m)
    x_init = rc.rwmh_x_init(m, target)
    assert torch.equal(x_init, c["x_init"])
    torch.manual_seed(m["seed"])
    out = mcmc_sample("cpu", target, x_init.clone(), target_log_prob_and_grad=lambda y: (target.unnorm_log_prob(y).flatten(), target.score(y)),
                      **rc.rwmh_kwargs(m))
    assert out.shape == c["samples"].shape == (m["n_keep"] * m["n_init"] * m["n_chains_per_mode"], 2) and out.device.type == "cpu"
    assert float((out - c["samples"]).abs().max()) < 1e-5
    if m["target"] == "checkerboard":  # the fixture holds chains that started outside: some walked in, the far ones never moved
        lp = c["logp"].view(m["n_keep"], -1)
        n = m["n_chains_per_mode"]
        assert bool(torch.isfinite(lp[:, :-4 * n]).all()) and bool(torch.isfinite(lp[-1, -4 * n:-n]).any()) and bool(torch.isinf(lp[:, -n:]).all())
        assert torch.equal(c["samples"].view(m["n_keep"], -1, 2)[:, -n:], torch.tensor(rc.CHECKERBOARD_OUTSIDE[-1]).expand(m["n_keep"], n, 2))


@pytest.mark.parametrize("name", rc.RUN_CASES)
def test_run_samplers_match_the_reference_fixture(name):
    """run_smc_sampler / run_re_sampler with the target as plain callables (the host path: the reference's closure)."""
    from sde_sampler_lrds_amd.additions import ebm_mle
    from sde_sampler_lrds_amd.experiments import benchmark_utils as bu
    c = gc.load(name)
    m = c.meta
    mean, var, kw = rc.run_inputs(m)
    assert torch.equal(mean, c["mean"]) and torch.equal(var, c["var"])
    calls = ebm_mle._native_calls[0]
    torch.manual_seed(m["seed"])
    out = (bu.run_smc_sampler if m["sampler"] == "smc" else bu.run_re_sampler)(mean.clone(), var.clone(), **kw)
    assert out.shape == c["samples"].shape == (m["n_steps"], m["B"], m["d"])
    assert float((out - c["samples"]).abs().max()) < 1e-5
    assert ebm_mle._native_calls[0] == calls


@pytest.mark.parametrize("name", rc.RUN_CASES)
def test_define_tempering_utils_ends_are_the_target_and_the_prior(name):
    from sde_sampler_lrds_amd.experiments.benchmark_utils import define_tempering_utils
    c = gc.load(name)
    m = c.meta
    mean, var, kw = rc.run_inputs(m)
    prior, path = define_tempering_utils(mean, var, kw["target_log_prob"], target_score=kw["target_score"])
    assert type(prior).__name__ == ("GaussFull" if m["full"] else "Gauss") and not hasattr(path, "hip_pair")
    x = c["probe"]
    lp0, g0 = path(torch.zeros(x.shape[0], 1), x)
    lp1, g1 = path(torch.ones(x.shape[0], 1), x)
    # t = 0: the target; t = 1: the prior
    # (the score: autograd or the closed form, two roundings of mode terms of size (x -+ 2) / 0.3 ~ 20 -- 1e-5 relative to those)
    assert torch.equal(lp0, rc.two_mode_log_prob(x)) and gc.rel_err(g0, rc.two_mode_score(x)) < 1e-5
    assert torch.equal(lp1, prior.log_prob(x).flatten()) and torch.equal(g1, prior.score(x))
    for got, key in ((lp0, "path_lp_t0"), (g0, "path_grad_t0"), (lp1, "path_lp_t1"), (g1, "path_grad_t1")):
        assert gc.rel_err(got, c[key]) < 1e-5, key
