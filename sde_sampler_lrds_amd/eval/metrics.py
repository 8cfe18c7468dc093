"""Sample metrics of the reference's evaluation layer (``sde_sampler/eval/metrics.py:12-198``): same keys, same rules.  Host-side
torch on the samples' device; the quadratic sample losses a model carries (``eval_sample_losses``: Sinkhorn, MMD) are HIP kernels."""
from __future__ import annotations

import logging
from numbers import Number
from typing import Callable

import torch

from ..distr.base import EXPECTATION_FNS


def abs_and_rel_error(prediction: Number, target: Number, suffix: str = "", eps: float = 1e-8) -> dict[str, float]:
    assert isinstance(prediction, Number)
    assert isinstance(target, Number)
    error = abs(prediction - target)
    return {f"error{suffix}": error, f"rel_error{suffix}": error / (abs(target) + eps)}


def compute_errors(prediction, target=None, name: str = "error", weights: torch.Tensor | None = None, eps: float = 1e-8) -> dict[str, float]:
    """``eval/<name>`` (+ ``_is`` with importance weights for per-sample predictions [B,1]) and, given a target value, the absolute
    and relative error of each (eval/metrics.py:26-63)."""
    out = {}
    if isinstance(prediction, Number):
        out[f"eval/{name}"] = prediction
    else:
        assert isinstance(prediction, torch.Tensor)
        if prediction.ndim == 0:
            out[f"eval/{name}"] = prediction.item()
        else:
            assert prediction.ndim == 2 and prediction.shape[-1] == 1
            out[f"eval/{name}"] = prediction.mean().item()
            if weights is not None:
                assert weights.shape == prediction.shape
                out[f"eval/{name}_is"] = ((prediction * weights).sum() / weights.sum()).item()
    if target is not None:
        if not isinstance(target, Number):
            assert target.ndim == 0
            target = target.item()
        for key, pred in list(out.items()):
            out.update(abs_and_rel_error(prediction=pred, target=target, suffix=key.replace("eval", ""), eps=eps))
    return out


def frac_inside_domain(samples, domain):
    assert samples.shape[-1] == domain.shape[0]
    inside = (domain[:, 0] <= samples) & (samples <= domain[:, 1])
    return inside.all(dim=-1).float().mean().item()


def get_metrics(distr, samples: torch.Tensor, weights: torch.Tensor | None = None, log_norm_const_preds: dict | None = None,
                expectation_preds: dict | None = None, marginal_dims: list[int] | None = None,
                sample_losses: dict[str, Callable] | None = None) -> dict[str, float]:
    """eval/metrics.py:70-198."""
    marginal_dims = marginal_dims or []  # (upstream iterates first and so fails on None; an empty list is what its solvers pass)
    if not all(d < distr.dim for d in marginal_dims):
        logging.warning("Removing non-existent marginal dims for metrics.")
        marginal_dims = [d for d in marginal_dims if d < distr.dim]
    metrics = {}
    expectation_preds = expectation_preds or {}
    log_norm_const_preds = log_norm_const_preds or {}

    fns = dict(EXPECTATION_FNS)  # :88-101: the hooks a target has decide what else is reported
    if hasattr(distr, "compute_mode_weight"):
        fns["mode_weight"] = lambda s: distr.compute_mode_weight(s).item()
    if hasattr(distr, "compute_phi_four_weight"):
        fns["weight"] = lambda s: distr.compute_phi_four_weight(s).item()
    if distr.has_entropy():
        fns["emc"] = lambda s: distr.entropy(s).item()
        fns["kl_weights"] = lambda s: distr.kl_weights(s).item()
        fns["tv_weights"] = lambda s: distr.tv_weights(s).item()
        fns["num_forgotten_modes"] = lambda s: distr.compute_forgotten_modes(s).item()
    if hasattr(distr, "compute_predictive_log_prob"):
        fns["avg_predictive_log_prob"] = lambda s: distr.compute_predictive_log_prob(s).item()

    for name, fn in fns.items():
        target = distr.expectations.get(name)
        metrics.update(compute_errors(prediction=fn(samples), target=target, name=name, weights=weights))
        if name in expectation_preds:
            metrics.update(compute_errors(prediction=expectation_preds[name], target=target, name=name + "_direct", weights=weights))

    for name, pred in log_norm_const_preds.items():
        metrics.update(compute_errors(prediction=pred, target=distr.log_norm_const, name=name))

    if weights is not None:
        assert weights.shape == (samples.shape[0], 1)
        ess = (weights.sum() ** 2 / (weights ** 2).sum()).item()
        metrics["eval/effective_sample_size"] = ess
        metrics["eval/norm_effective_sample_size"] = ess / len(weights)

    stddevs, means = samples.std(dim=0), samples.mean(dim=0)
    avg_stddev = stddevs.mean().item()
    metrics["eval/avg_stddev"] = avg_stddev
    for dim in marginal_dims:
        metrics[f"eval/stddev_{dim}"] = stddevs[dim].item()
        metrics[f"eval/avg_{dim}"] = means[dim].item()
    if getattr(distr, "stddevs", None) is not None:
        ref = distr.stddevs.to(stddevs.device)
        assert ref.shape == stddevs.shape
        metrics["error/avg_marginal_stddev"] = (stddevs - ref).abs().mean().item()
        metrics.update(compute_errors(prediction=avg_stddev, target=ref.mean(), name="avg_stddev"))

    if distr.domain is not None:
        metrics["eval/frac_pred_in_domain"] = frac_inside_domain(samples, distr.domain.to(samples.device))

    if sample_losses is not None:  # :173-191
        if hasattr(distr, "sample"):
            gt_samples = distr.sample((samples.shape[0],)).to(samples.device)
            assert gt_samples.shape == samples.shape
            if distr.domain is not None:
                metrics["eval/frac_groundtruth_in_domain"] = frac_inside_domain(gt_samples, distr.domain.to(samples.device))
            metrics.update({"error/" + name: loss(samples, gt_samples).item() for name, loss in sample_losses.items()})
        else:
            logging.warning("Sampling not implemented for distribution %s.", distr.__class__.__name__)

    if hasattr(distr, "objective"):
        metrics["eval/obj_avg"] = distr.objective(samples.mean(dim=0, keepdims=True)).item()
        metrics["eval/avg_obj"] = distr.objective(samples).mean().item()
        metrics["eval/min_obj"] = distr.objective(samples).min().item()
    return metrics
