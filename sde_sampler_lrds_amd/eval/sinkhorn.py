"""Entropy-regularised p-Wasserstein distance between two point clouds (``sde_sampler/eval/sinkhorn.py:11-194``: same class, same
arguments, same checks).  Upstream writes the iteration on pykeops lazy tensors, which compile CUDA at run time and have no ROCm
backend; here ``compute`` is one call of ``sdeng_sinkhorn`` (csrc/metric_kernels.hip): the cost matrix, every log-sum-exp pass,
the transport cost and the correspondences are HIP kernels, and nothing quadratic is built by torch.  Not differentiable (upstream's
can be back-propagated through; no caller in the package does)."""
from __future__ import annotations

import torch

from .. import engine as E


class Sinkhorn:
    def __init__(self, p: int = 2, eps: float = 1e-3, max_iters: int = 100, stop_thresh: float = 1e-5, verbose: bool = False,
                 n_max: int | None = None, **kwargs):
        # eval/sinkhorn.py:43-62
        if not isinstance(p, int):
            raise TypeError(f"p must be an integer greater than 0, got {p}")
        if p <= 0:
            raise ValueError(f"p must be an integer greater than 0, got {p}")
        if eps <= 0:
            raise ValueError("Entropy regularization term eps must be > 0")
        if not isinstance(max_iters, int) or max_iters <= 0:
            raise TypeError(f"max_iters must be an integer > 0, got {max_iters}")
        if not isinstance(stop_thresh, float):
            raise TypeError(f"stop_thresh must be a float, got {stop_thresh}")
        self.p, self.eps, self.max_iters, self.stop_thresh = p, eps, max_iters, stop_thresh
        self.n_max, self.verbose = n_max, verbose
        self.n_iters_ = None  # iterations run by the last call
        self.max_err_ = None  # (max |du|, max |dv|) of its last iteration

    @staticmethod
    def _check_weights(w, pts, name):
        # eval/sinkhorn.py:83-110
        if len(w.shape) > 1:
            w = w.squeeze()
        if len(w.shape) != 1:
            raise ValueError(f"{name} must have shape [n,] or [n, 1], got {tuple(w.shape)}")
        if w.shape[0] != pts.shape[0]:
            raise ValueError(f"{name} has {w.shape[0]} entries for {pts.shape[0]} points")
        return w

    def compute(self, x: torch.Tensor, y: torch.Tensor, w_x: torch.Tensor | None = None, w_y: torch.Tensor | None = None):
        """(distance, corr_x_to_y [n], corr_y_to_x [m])."""
        if len(x.shape) != 2:
            raise ValueError(f"x must be an [n, d] tensor but got shape {x.shape}")
        if len(y.shape) != 2:
            raise ValueError(f"y must be an [m, d] tensor but got shape {y.shape}")
        if x.shape[1] != y.shape[1]:
            raise ValueError(f"x and y must match in the last dimension, got x.shape = {x.shape}, y.shape = {y.shape}")
        if (w_x is None) != (w_y is None):
            raise ValueError("w_x and w_y must both be given, or neither")
        if w_x is None:  # uniform (:123-126; upstream rescales w_y by n / m, so unequal sizes need explicit weights there too)
            n, m = x.shape[0], y.shape[0]
            sum_w_x, sum_w_y = 1.0, n / m
        else:
            w_x, w_y = self._check_weights(w_x, x, "w_x"), self._check_weights(w_y, y, "w_y")
            sum_w_x, sum_w_y = w_x.sum().item(), w_y.sum().item()
        if abs(sum_w_x - sum_w_y) > 1e-5:  # :128-135
            raise ValueError(f"Weights w_x and w_y do not sum to the same value, got {sum_w_x} and {sum_w_y}")
        E.require_gpu(x)
        E.require_gpu(y)
        if self.p > 2:
            raise NotImplementedError(f"p = {self.p}: the kernels cover p in {{1, 2}} (upstream's cost is NaN for odd p > 1: it takes "
                                      "the root of a signed sum)")
        out = E.sinkhorn(x, y, w_x, w_y, p=self.p, eps=self.eps, max_iters=self.max_iters, stop_thresh=self.stop_thresh)
        self.n_iters_, self.max_err_ = out["iters"], (out["max_err_u"], out["max_err_v"])
        if self.verbose:
            print(f"sinkhorn: {self.n_iters_} iterations, max change {max(self.max_err_):.3e}")
        return out["distance"].to(x.dtype), out["corr_x_to_y"], out["corr_y_to_x"]

    def __call__(self, x: torch.Tensor, y: torch.Tensor, w_x: torch.Tensor | None = None, w_y: torch.Tensor | None = None):
        if self.n_max is not None:  # :186-193
            x, y = x[: self.n_max], y[: self.n_max]
            w_x = w_x if w_x is None else w_x[: self.n_max]
            w_y = w_y if w_y is None else w_y[: self.n_max]
        return self.compute(x, y, w_x=w_x, w_y=w_y)[0]
