"""The 2-D toy suite on the engine (experiments/sample_toy_competing.py): the Checkerboard target in every forward form, CMCD on Rings
and Checkerboard, and the estimators on log-weights that are +inf for particles outside the checkerboard's squares.  Fixtures come
from the real reference (tests/golden/gen_golden_toy.py); the evaluation cases inject the normals the reference drew."""
import ctypes as C
import math

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.distr.checkerboard import Checkerboard
from sde_sampler_lrds_amd.distr.gauss import Gauss, GaussFull, IsotropicGauss
from sde_sampler_lrds_amd.distr.rings import Rings
from sde_sampler_lrds_amd.eq.sdes import VP, ControlledLangevinSDE, ScaledBM
from sde_sampler_lrds_amd.losses import oc
from sde_sampler_lrds_amd.models.reparam import ClippedCtrl, ScoreCtrl
from sde_sampler_lrds_amd.reference import MarginalReference
from tests import build_cases as bc
from tests import golden_cases as gc

TOL = 1e-4  # x_N and finite rnd, max |a - b| / max(1, |b|), injected noise

EVAL_CASES = ["toy_pis_checkerboard", "toy_dds_checkerboard", "toy_dis_checkerboard", "toy_rds_em_diag_checkerboard",
              "toy_rds_ei_diag_checkerboard", "toy_rds_em_full_checkerboard", "toy_rds_ei_full_checkerboard", "toy_cmcd_rings",
              "toy_cmcd_checkerboard"]


def _ctrl(c, target):
    m = c.meta
    if c.meta.get("target") == "rings":
        ctrl = ScoreCtrl(base_model=bc._mlp(2), score_model=bc._score_model(), target_score=target.score, detach_score=False,
                         clip_score=m["clip_score"], clip_model=m["clip_model"], scale_score=m["scale_score"])
    else:
        ctrl = ClippedCtrl(base_model=bc._mlp(2), clip_model=m["clip_model"])
    ctrl.load_state_dict(c.params("ctrl."))
    return ctrl


def _cmcd(c, dev, max_rnd=1e8):
    m = c.meta
    if m["target"] == "rings":
        target = Rings(dim=2, lower_rad=m["lower_rad"], upper_rad=m["upper_rad"], num_rad=m["num_rad"], scale=m["scale"], n_reference_samples=10)
        prior = IsotropicGauss(dim=2, scale=m["prior_scale"])
    else:
        target = Checkerboard(dim=2, width=4)
        prior = GaussFull(dim=2, loc=c["prior_loc"], cov=c["prior_cov"])
    sde = ControlledLangevinSDE(target_score=target.score, prior_score=prior.score, diff_coeff=m["diff_coeff"], terminal_t=m["T"],
                                clip_score=m["clip_langevin"])
    ctrl = _ctrl(c, target)
    for mod in (target, prior, sde, ctrl):
        mod.to(dev)
    loss = oc.ControlledLangevinSDELoss(ctrl, ctrl, sde=sde, method="lv", max_rnd=max_rnd)
    loss.seed = m["seed"]
    return loss, target, prior


def _run(c, dev):
    """The case's simulate() on the engine with the reference's normals injected -> (x_N, rnd)."""
    m, kind = c.meta, c.meta["kind"]
    ts, x0, noise = c["ts"].to(dev), c["x0"].to(dev), c["noise"].to(dev)
    if kind == "toy_cmcd":
        loss, target, prior = _cmcd(c, dev)
        x, rnd, _ = loss.simulate(ts, x0, target.unnorm_log_prob, initial_log_prob=prior.log_prob, train=False, noise=noise)
        return x, rnd
    target = Checkerboard(dim=2, width=4).to(dev)
    ctrl = _ctrl(c, target).to(dev)
    if kind == "toy_pis":
        sde = ScaledBM(diff_coeff=m["diff_coeff"], terminal_t=m["T"]).to(dev)
        refd = Gauss(dim=2, loc=c["ref_loc"], scale=c["ref_scale"]).to(dev)
        loss = oc.EMReferenceSDELoss(ctrl, ctrl, sde=sde, method="kl")
        x, rnd, _ = loss.simulate(ts, x0, target.unnorm_log_prob, refd.log_prob, noise=noise)
    elif kind == "toy_dds":
        prior = IsotropicGauss(dim=2, scale=m["sigma"]).to(dev)
        loss = oc.ExponentialIntegratorSDELoss(ctrl, ctrl, sde=None, method="kl", alpha=m["alpha"], sigma=m["sigma"])
        x, rnd, _ = loss.simulate(ts, x0, target.unnorm_log_prob, prior.log_prob, compute_ito_int=True, noise=noise)
    elif kind == "toy_dis":
        sde = VP(m["beta_min"], m["beta_max"], m["sigma"], terminal_t=m["T"]).to(dev)
        prior = IsotropicGauss(dim=2, scale=m["sigma"]).to(dev)
        loss = oc.TimeReversalLoss(ctrl, ctrl, sde=sde, method="kl", inference_ctrl=None)
        x, rnd, _ = loss.simulate(ts, x0, target.unnorm_log_prob, initial_log_prob=prior.log_prob, train=False, compute_ito_int=True, noise=noise)
    elif kind == "toy_rds":
        sde = VP(m["beta_min"], m["beta_max"], m["sigma"], terminal_t=m["T"])
        ref = MarginalReference(sde, "gmm", means_init=c["ref_means"], variances_init=c["ref_vars"], weights_init=c["ref_w"].clone())
        sde.to(dev)
        ref.to(dev)
        cls = {"ei": oc.EIReferenceSDELoss, "em": oc.EMReferenceSDELoss}[m["integrator"]]
        loss = cls(ctrl, ctrl, sde=sde, method="kl", reference_ctrl=ref)
        x, rnd, _ = loss.simulate(ts, x0, target.unnorm_log_prob, ref.reference_distr.to(dev).log_prob, noise=noise)
    else:
        raise KeyError(kind)
    return x, rnd


def _torch_results(rnd):
    """BaseOCLoss.compute_results (losses/oc.py:150-161) + the normalised ESS, in torch on the same rnd."""
    neg = -rnd.double().view(-1, 1)
    w = torch.nn.functional.softmax(neg, dim=0)
    return dict(elbo=float(neg.mean()), logz=float(torch.logsumexp(neg, dim=0) - math.log(neg.shape[0])), var=float(rnd.double().var()),
                ess=float(w.sum() ** 2 / (w ** 2).sum() / neg.shape[0]), weights=w.view(-1))


def _same(a, b, tol):
    if math.isinf(b) or math.isnan(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= tol * max(1.0, abs(b))


def _check_estimators(rnd, ref_results=None):
    stats, w = E.logz_stats(rnd)
    s = stats.double().cpu()
    t = _torch_results(rnd.cpu())
    assert _same(float(s[0]), t["elbo"], 1e-5) and _same(float(s[1]), t["logz"], 1e-5) and _same(float(s[3]), t["ess"], 1e-4), (s[:4], t)
    assert math.isnan(float(s[2])) == math.isnan(t["var"])
    wt, wk = t["weights"], w.double().cpu().view(-1)
    assert torch.equal(torch.isnan(wk), torch.isnan(wt))
    fin = ~torch.isnan(wt)
    out = torch.isinf(rnd.cpu().view(-1)) & fin
    assert (wk[out] == 0).all() and (wt[out] == 0).all()  # particles outside the target's support get exactly zero weight
    assert float((wk[fin] - wt[fin]).abs().max()) <= 1e-5 * float(wt[fin].abs().max())
    if ref_results is not None:  # the reference's own compute_results on ITS rnd (same -inf pattern, fp32 round-off apart)
        for key, got in (("elbo", float(s[0])), ("log_norm_const_is", float(s[1])), ("ess", float(s[3]))):
            assert _same(got, ref_results[key], 1e-3), (key, got, ref_results[key])
    return s


@pytest.mark.gpu
def test_checkerboard_dist_eval_is_exact(gpu):
    c = gc.load("toy_checkerboard_logp")
    for obj in (Checkerboard(), Checkerboard().to(gpu)):
        lp, sc = E.dist_eval(obj, c["x"].to(gpu))
        lp = lp.cpu()
        assert torch.equal(lp, c["logp"]), "log-density differs from the reference"  # -inf in the same places, finite values bit for bit
        assert torch.equal(sc.cpu(), torch.zeros_like(c["x"]))
    x = c["x"].to(gpu)
    assert torch.equal(E.dist_eval(Checkerboard(), x)[0], E.dist_eval(Checkerboard(), x)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", EVAL_CASES)
def test_eval_parity_with_injected_noise(gpu, name):
    c = gc.load(name)
    x, rnd_dev = _run(c, gpu)
    torch.cuda.synchronize()
    x, rnd = x.cpu(), rnd_dev.cpu()
    ex = gc.rel_err(x, c["out_x"])
    assert torch.equal(torch.isinf(rnd), torch.isinf(c["rnd"])), "+inf log-weights (end points outside the squares) differ"
    assert not torch.isnan(rnd).any() and not (rnd == -math.inf).any()
    fin = torch.isfinite(c["rnd"])
    er = gc.rel_err(rnd[fin], c["rnd"][fin])
    print(f"{name}: x_N {ex:.2e}, finite rnd {er:.2e}, {int((~fin).sum())} of {fin.numel()} at +inf")
    assert ex < TOL and er < TOL
    if "checkerboard" in name:
        assert c.meta["n_inf"] > 0
    _check_estimators(rnd_dev, c.meta)
    x2, rnd2 = _run(c, gpu)  # bit-identical when repeated
    assert torch.equal(x2.cpu(), x) and torch.equal(rnd2.cpu(), rnd)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy_cmcd_rings", "toy_cmcd_checkerboard"])
def test_cmcd_eubo(gpu, name):
    c = gc.load(name)
    loss, target, prior = _cmcd(c, gpu)
    args = (c["ts"].to(gpu), c["x_tgt"].to(gpu), target.unnorm_log_prob)
    rnd = loss.compute_eubo(*args, initial_log_prob=prior.log_prob, noise=c["eubo_noise"].to(gpu)).cpu()
    assert torch.isfinite(rnd).all() and torch.isfinite(c["eubo_rnd"]).all()
    err = gc.rel_err(rnd, c["eubo_rnd"])
    print(f"{name} eubo: rnd {err:.2e}")
    assert err < TOL
    again = loss.compute_eubo(*args, initial_log_prob=prior.log_prob, noise=c["eubo_noise"].to(gpu)).cpu()
    assert torch.equal(again, rnd)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy_train_cmcd_rings", "toy_train_cmcd_checkerboard"])
def test_cmcd_lv_training_step(gpu, name):
    c = gc.load(name)
    loss, target, prior = _cmcd(c, gpu, max_rnd=c.meta["max_rnd"])
    ctrl = loss.generative_ctrl
    for p in ctrl.parameters():
        p.grad = None
    value, metrics = loss(c["ts"].to(gpu), c["x0"].to(gpu), target.unnorm_log_prob, initial_log_prob=prior.log_prob)
    value.backward()
    assert math.isfinite(float(value.detach()))
    loss_err = abs(float(value.detach()) - c.meta["loss"]) / max(1.0, abs(c.meta["loss"]))
    tol = max(5e-5, 10 * c.meta["grad_sensitivity"])
    worst, n = 0.0, 0
    for k, p in ctrl.named_parameters():
        if "grad." + k not in c.a:
            continue
        ref = c["grad." + k]
        assert torch.isfinite(p.grad).all(), k
        worst, n = max(worst, float((p.grad.cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)), n + 1
    print(f"{name}: loss {float(value.detach()):.6f} vs {c.meta['loss']:.6f} (rel {loss_err:.1e}); worst gradient error {worst:.2e} "
          f"over {n} parameters (tolerance {tol:.1e}); filtered {metrics.get('train/n_filtered_cumulative')}")
    assert n >= 8 and loss_err < 1e-5 and worst < tol
    if "checkerboard" in name:
        assert metrics["train/n_filtered_cumulative"] > 0  # particles outside the squares: rnd = +inf, dropped by rnd.isfinite()


@pytest.mark.gpu
def test_large_batch_with_leading_blocks_outside(gpu):
    """65 536 particles whose first 16 blocks of 256 are all outside every square: the estimators take the global maximum first."""
    torch.manual_seed(0)
    cb = Checkerboard().to(gpu)
    x = cb.sample((65536,))
    x[:4096] = torch.tensor([5.0, 5.0], device=gpu)  # outside the domain
    x[4096::7] = torch.tensor([-3.0, 3.0], device=gpu)  # outside: the lower-left quarter of cell (-4, 2)..(-2, 4) holds no square
    lp, _ = E.dist_eval(cb, x, want_score=False)
    assert torch.equal(lp, cb.unnorm_log_prob(x))
    rnd = (-lp + 0.3 * torch.randn_like(lp)).contiguous()
    n_out = int(torch.isinf(rnd).sum())
    assert n_out > 4096 and n_out < 65536
    s = _check_estimators(rnd)
    assert math.isfinite(float(s[1])) and float(s[0]) == -math.inf and math.isfinite(float(s[3]))
    _, w = E.logz_stats(rnd)
    assert torch.isfinite(w).all() and float(w[:4096].abs().max()) == 0.0 and abs(float(w.double().sum()) - 1.0) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 300, 65536])
def test_all_outside_gives_minus_inf_log_z_and_nan_weights(gpu, B):
    rnd = torch.full((B, 1), math.inf, device=gpu)
    stats, w = E.logz_stats(rnd)
    s = stats.cpu()
    t = _torch_results(rnd.cpu())
    assert t["logz"] == -math.inf and float(s[1]) == -math.inf  # torch.logsumexp of all -inf is -inf, not NaN
    assert float(s[0]) == -math.inf and t["elbo"] == -math.inf
    assert math.isnan(float(s[3])) and math.isnan(t["ess"])
    assert torch.isnan(w).all() and torch.isnan(t["weights"]).all()


@pytest.mark.gpu
def test_finite_estimators_unchanged_by_the_infinite_max_rule(gpu):
    torch.manual_seed(1)
    rnd = (3.0 * torch.randn(10000, 1, device=gpu)).contiguous()
    _check_estimators(rnd)


@pytest.mark.gpu
def test_langevin_moves_and_kl_adjoint_refuse_the_checkerboard(gpu):
    cb = Checkerboard().to(gpu)
    B, d = 16, 2
    x = cb.sample((B,)).contiguous()
    lp, grad = torch.zeros(B, device=gpu), torch.zeros(B, d, device=gpu)
    step = torch.full((B,), 0.01, device=gpu)
    with pytest.raises(E.UnsupportedByEngine):
        E.langevin_moves(cb, None, x, lp, grad, step, 4, noise="philox")
    with pytest.raises(E.UnsupportedByEngine):
        E.langevin_moves(IsotropicGauss(dim=2).to(gpu), cb, x, lp, grad, step, 4, noise="philox")
    # the C entry point itself: SDENG_E_UNSUPPORTED, not a launch
    keep = []
    ds = E.dist_desc(cb, gpu, keep)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=gpu)
    rc = L.lib().sdeng_langevin_moves(None, C.byref(ds), B, d, 4, 0, 0, 0.0, None, x.data_ptr(), lp.data_ptr(), grad.data_ptr(),
                                      step.data_ptr(), None, None, 0, 0, None, None, None, ws.data_ptr(), ws.numel(), E._stream_ptr(gpu))
    assert rc == L.E_UNSUPPORTED
    ctrl = ScoreCtrl(base_model=bc._mlp(d), score_model=bc._score_model(), target_score=cb.score, detach_score=False, clip_score=1e4,
                     clip_model=1e4, scale_score=1.0).to(gpu)
    N = 4
    coef = torch.zeros(N, L.NCOEF, device=gpu)
    xs = torch.zeros(N, B, d, device=gpu)
    with pytest.raises(E.UnsupportedByEngine):
        E.kl_adjoint(ctrl, coef, xs, None, torch.full((B, 1), 1.0 / B, device=gpu), torch.zeros(B, d, device=gpu), lin=False, ito=False)
