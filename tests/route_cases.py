"""The models whose training routes ``tests/golden/training_routes.json`` records: every ``make_model`` combination the reference accepts
(``make_model_grid.json``: "ok") with both ``force_vp*`` flags off, on six targets, built on the CPU with four steps -- construction launches
nothing.  ``time_type`` and ``loss_type`` are collapsed to one value each (no route reads the time grid or the loss's method; the generator
checked that on the full product before it wrote the fixture); a Gaussian / mixture reference (CMCD: the Gaussian prior) is built once with
diagonal variances and once with full covariances.  Shared by ``tests/golden/gen_training_routes.py`` and ``tests/test_routes_cpu.py``."""
import itertools
import json
import os

import torch

from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.distr.logistic_regression import register_dataset
from sde_sampler_lrds_amd.experiments import benchmark_utils as bu
from sde_sampler_lrds_amd.models.reparam import RemoveReferenceCtrl

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TARGETS = {"many_modes": dict(dim=4, n_modes=3), "two_modes_full": dict(dim=4), "phi_four": dict(dim=8), "rings": {}, "checkerboard": {}, "sonar": {}}
TRAIN = dict(train_steps=10, train_batch_size=8, eval_batch_size=16)
AXES = ("target", "solver_type", "ref_type", "cov", "integrator_type", "model_type", "force_base_zero_init")
SETTINGS = [(False, False), (False, True), (True, False), (True, True)]  # (native_adjoint, fused_training) for KL; (fused_training, graph_training) for log-variance


def register_sonar():
    g = torch.Generator().manual_seed(0)
    register_dataset("sonar", torch.randn(166, 60, generator=g), (torch.rand(166, generator=g) < 0.5).float())


def details(dim, cov, k=3):
    """``solver_details`` of ``make_model``: a reference (CMCD: a prior) with diagonal variances or full covariances."""
    g = torch.Generator().manual_seed(0)
    var, var_k = torch.rand(dim, generator=g) + 0.5, torch.rand(k, dim, generator=g) + 0.5
    if cov == "full":
        var, var_k = torch.diag_embed(var) + 0.1, torch.diag_embed(var_k) + 0.1
    return dict(sigma=1.3, mean_ref=torch.randn(dim, generator=g), var_ref=var, weights_ref=torch.ones(k) / k,
                means_ref=torch.randn(k, dim, generator=g), variances_ref=var_k, mean=torch.zeros(dim), var=var)


def grid_ok(collapse=True):
    """The accepted argument combinations, force_vp* off: dicts of make_model's keywords plus ``cov``.  ``collapse``: the first accepted
    (loss_type, time_type) of each combination only."""
    grid = json.load(open(os.path.join(GOLDEN, "make_model_grid.json")))
    axes = grid["axes"]
    seen, out = set(), []
    for combo, ch in zip(itertools.product(*axes.values()), grid["index"]):
        kw = dict(zip(axes, combo))
        if grid["outcomes"][ord(ch) - ord("a")] != "ok" or kw["force_vp20"] or kw["force_vp_cosine"]:
            continue
        key = tuple(kw[a] for a in AXES if a in kw)
        if collapse and key in seen:
            continue
        seen.add(key)
        with_cov = kw["ref_type"] in ("gaussian", "gmm")  # the only arguments that carry variances
        out += [dict(kw, cov=cov) for cov in (("diag", "full") if with_cov else ("diag",))]
    return out


def build(target, kw):
    """The solver of one combination on ``target``, or None where ``make_model`` has no kernel to offer (UNet nets, 'nn' references)."""
    tdet = bu.make_target_details(target, **TARGETS[target])
    model_kw = {k: v for k, v in kw.items() if k != "cov"}
    dim = {"rings": 2, "checkerboard": 2, "sonar": 61}.get(target) or TARGETS[target]["dim"]
    try:
        return bu.make_model(**model_kw, solver_details=details(dim, kw["cov"]), target_details=tdet, training_details=TRAIN, n_steps=4,
                             device="cpu", compute_samples_based_metrics=False)
    except E.UnsupportedByEngine:
        return None


def key_of(target, kw):
    return (target,) + tuple(kw[a] for a in AXES[1:])


def wrapped_cases():
    """(name, loss) with a wrapped control as ``loss.generative_ctrl``, which no ``make_model`` combination produces (it rebinds the solver's
    attribute after the loss was built): a RemoveReferenceCtrl in the form upstream can evaluate, one around an EMA copy, and a bare EMA copy,
    around the Clipped / Score / CancelDrift control of an RDS solver on the mixture and on logistic regression (graph-less score), and a bare EMA
    copy on CMCD."""
    ema = torch.optim.swa_utils.AveragedModel
    wraps = {"remove_ref": lambda c, ref: RemoveReferenceCtrl(c, ref, use_rescaling=False),
             "remove_ref_ema": lambda c, ref: RemoveReferenceCtrl(ema(c), ref, use_rescaling=False), "ema": lambda c, ref: ema(c)}
    for target, solver, model_type in itertools.product(("many_modes", "sonar"), ("vp-ref", "cmcd"), ("base_zero_init", "target_informed_zero_init",
                                                                                                      "target_informed_langevin_init")):
        ref_solver = solver == "vp-ref"
        if not ref_solver and model_type == "base_zero_init":
            continue  # (make_model refuses it)
        for wname, wrap in wraps.items():
            if not ref_solver and wname != "ema":
                continue  # (CMCD has no reference to remove)
            kw = dict(solver_type=solver, ref_type="gmm" if ref_solver else "default", loss_type="lv", integrator_type="em", model_type=model_type,
                      time_type="uniform", force_base_zero_init=False, force_vp20=False, force_vp_cosine=False, cov="diag")
            model = build(target, kw)
            model.loss.generative_ctrl = wrap(model.loss.generative_ctrl, getattr(model, "reference_score_t", None))
            yield f"{target}/{solver}/{model_type}/{wname}", model.loss
