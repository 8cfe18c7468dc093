"""The fixtures of tests/golden/gen_golden_rds_score.py -- reference samplers with a target-informed control over Gaussian, diagonal and
full-covariance mixture references -- rebuilt on top of the CPU oracle (``run_oracle``) and of the product classes (``build``).  The
committed oracle restates every case as it is: its ``simulate_*_ref`` / ``eubo_*_ref`` loops take any ``Ctrl``."""
from __future__ import annotations

import torch

from oracle import sde_oracle as orc
from sde_sampler_lrds_amd.distr.gauss import GMM
from sde_sampler_lrds_amd.distr.phi_four import PhiFour
from sde_sampler_lrds_amd.eq.sdes import VP
from sde_sampler_lrds_amd.losses import oc
from sde_sampler_lrds_amd.models.reparam import CancelDriftCtrl, RemoveReferenceCtrl, ScoreCtrl
from sde_sampler_lrds_amd.reference import MarginalReference
from tests import build_cases as bc
from tests import golden_cases as gc

SIM_CASES = ["rds_ei_score_gmm_fullcov_d40_k3", "rds_em_score_phi4_fullcov_d100_k2", "rds_em_remove_ref_fullcov_d72_k2"]
EUBO_CASES = ["eubo_ei_score_gauss_d8", "eubo_ei_score_gmm_d16_k4", "eubo_em_score_phi4_d100_k16", "eubo_ei_score_gmm_fullcov_d40_k3",
              "eubo_em_score_phi4_fullcov_d100_k2"]
TRAIN_LV, TRAIN_KL = "train_lv_rds_ei_score_gmm_fullcov_d40_k3", "train_kl_rds_em_score_gmm_fullcov_d16_k2"
CTRL_PERTURB = "ctrl_perturb_ei_score_gmm_fullcov_d40_noise_dropout"

load = gc.load


def oracle_tol(name):
    """The rule of tests/test_oracle_golden.py: TOL_SIM, and 1e-5 for full-covariance references (the terminal log p_ref is torch's
    Cholesky-based MultivariateNormal mixture upstream and a restated quadratic form in the oracle: |log p| ~ 100-200, ulp 1.5e-5)."""
    from tests.test_oracle_golden import TOL_SIM
    return 1e-5 if ("fullcov" in name or "eigen" in name) else TOL_SIM


def _oracle_parts(c):
    m = c.meta
    sde = orc.VP(m["beta_min"], m["beta_max"], m["sigma"], m["T"])
    tgt = orc.PhiFour(m["a"], m["b"], m["d"], m["beta"]) if m["target"] == "phi4" else orc.GMMDiag(c["tgt_loc"], c["tgt_scale"], c["tgt_w"])
    if m["ref"] == "gauss":
        xi, vi = c["ref_x_init"], c["ref_var_init"]
        ref_score = lambda t, x: orc.gauss_score(x, *sde.marginal_diag(t, xi, vi))  # noqa: E731
        loc0, v0 = sde.marginal_diag(torch.tensor(0.0), xi, vi)
        refd = orc.GaussDiag(loc0, v0.sqrt())
    else:
        means, w = c["ref_means"], c["ref_w"]
        if m["cov"] == "full":
            cov = c["ref_cov"]
            ref_score = lambda t, x: orc.mog_score_full(x, w, *sde.marginal_full(t, means, cov))  # noqa: E731
            refd = orc.GMMFullCov(*sde.marginal_full(torch.tensor(0.0), means, cov), w)
        elif m["cov"] == "eigen":
            D, P = c["ref_D"], c["ref_P"]
            ref_score = lambda t, x: orc.mog_score_full_prec(x, w, *sde.marginal_eigen(t, means, D, P))  # noqa: E731
            refd = orc.GMMFullPrec(*sde.marginal_eigen(torch.tensor(0.0), means, D, P), w)
        else:
            var = c["ref_vars"]
            ref_score = lambda t, x: orc.mog_score(x, w, *sde.marginal_diag(t, means, var))  # noqa: E731
            loc0, v0 = sde.marginal_diag(torch.tensor(0.0), means, var)
            refd = orc.GMMDiag(loc0, torch.sqrt(v0), w)
    kind = "score" if m["ctrl"] == "score" else "cancel_drift"
    ctrl = orc.Ctrl(c.params("ctrl."), kind, clip_model=m["clip_model"], target_score=tgt.score, clip_score=m["clip_score"],
                    scale_score=m["scale_score"], sde=sde)
    if m["ctrl"] != "score":  # RemoveReferenceCtrl(CancelDriftCtrl, ref_score, use_rescaling=False)
        ctrl = orc.RemoveReference(ctrl, ref_score)
    return sde, tgt, refd, ref_score, ctrl


def run_oracle(c, noise=None, x0=None):
    """The oracle's restatement of a simulate / EUBO case -> (x_N or the noised x, rnd).  ``noise`` defaults to the counter-based replay
    the fixture was generated with, ``x0`` to the fixture's."""
    m = c.meta
    sde, tgt, refd, ref_score, ctrl = _oracle_parts(c)
    noise = noise or orc.PhiloxNoise(m["seed"])
    x0 = c["x0"] if x0 is None else x0
    with torch.no_grad():
        if m["kind"] == "eubo_score":
            if m["integrator"] == "ei":
                return orc.eubo_ei_ref(c["ts"], x0, ctrl, sde, tgt.logp, refd.logp, ref_score, noise)
            return orc.eubo_em_ref(c["ts"], x0, ctrl, sde, tgt.logp, refd.logp, ref_score, noise, use_rescaling=m["use_rescaling"])
        if m["integrator"] == "ei":
            out = orc.simulate_ei_ref(c["ts"], x0, ctrl, sde, tgt.logp, refd.logp, ref_score, noise)
        else:
            out = orc.simulate_em_ref(c["ts"], x0, ctrl, sde, tgt.logp, refd.logp, ref_score, noise, use_rescaling=m["use_rescaling"])
    return out[0], out[1]


def build(c, device):
    """-> dict(loss, ts, x0, args) from the product classes, every module on ``device`` (as tests/build_cases.py)."""
    m, d = c.meta, c.meta["d"]
    sde = VP(m["beta_min"], m["beta_max"], m["sigma"], terminal_t=m["T"])
    if m["target"] == "phi4":
        target = PhiFour(a=m["a"], b=m["b"], dim=d, beta=m["beta"])
    else:
        target = GMM(dim=d, loc=c["tgt_loc"], scale=c["tgt_scale"], mixture_weights=c["tgt_w"].clone())
    kw = dict(base_model=bc._mlp(d), score_model=bc._score_model(), target_score=target.score, detach_score=False, clip_score=m["clip_score"],
              clip_model=m["clip_model"], scale_score=m["scale_score"])
    ctrl = ScoreCtrl(**kw) if m["ctrl"] == "score" else CancelDriftCtrl(sde=sde, **kw)
    ctrl.load_state_dict(c.params("ctrl."))
    if m["ref"] == "gauss":
        ref = MarginalReference(sde, "gaussian", x_init=c["ref_x_init"], var_init=c["ref_var_init"])
    else:
        variances = c["ref_cov"] if m["cov"] == "full" else ((c["ref_D"], c["ref_P"]) if m["cov"] == "eigen" else c["ref_vars"])
        ref = MarginalReference(sde, "gmm", means_init=c["ref_means"], variances_init=variances, weights_init=c["ref_w"].clone())
    for mod in (sde, target, ctrl, ref):
        mod.to(device)
    if m["ctrl"] != "score":
        ctrl = RemoveReferenceCtrl(ctrl, ref, use_rescaling=False)
    if m["integrator"] == "ei":
        loss = oc.EIReferenceSDELoss(ctrl, ctrl, sde=sde, method=m["method"], reference_ctrl=ref)
    else:
        loss = oc.EMReferenceSDELoss(ctrl, ctrl, sde=sde, method=m["method"], reference_ctrl=ref, use_rescaling=m["use_rescaling"])
    loss.seed = m["seed"]
    return dict(loss=loss, ts=c["ts"].to(device), x0=c["x0"].to(device), args=(target.unnorm_log_prob, ref.reference_distr.to(device).log_prob),
                target=target, ref=ref, sde=sde)


def rnd_scale(c, b_cpu=None):
    """The largest summand of each particle's log-weight (tests/test_gpu_parity.py rnd_scale): the terminal log-densities at the point the
    loss evaluates them -- x_N, or the data x0 for the noising direction -- and the total."""
    b = b_cpu or build(c, "cpu")
    x = c["x0"] if c.meta["kind"] == "eubo_score" else c["out_x"]
    mags = [c["rnd"].abs()] + [fn(x).view(-1, 1).abs() for fn in b["args"]]
    return torch.stack([v.float() for v in mags]).max(dim=0).values.clamp(min=1.0)


def ulp_sensitivity(c, scale):
    """How far the REFERENCE's own fp32 result moves under a one-ulp relative change of x0 (stored in the fixture)."""
    ex = gc.rel_err(c["out_x_ulp"], c["out_x"])
    er = float(((c["rnd_ulp"].double() - c["rnd"].double()).abs().view(-1, 1) / scale.double().view(-1, 1)).max())
    return max(ex, er)
