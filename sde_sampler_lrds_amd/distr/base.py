"""Distribution base class (mirror of ``sde_sampler/distr/base.py:22-157``): parameter holder with a
torch implementation of log-density / score for host-side use (sampling targets, plotting, training with
autograd).  The simulate path never calls these: it reads the parameters through ``engine.dist_desc`` and
evaluates log-densities and scores in HIP (csrc/prep_kernels.hip, csrc/sim_device.hpp)."""
from __future__ import annotations

import math

import torch


# distr/base.py:13-18
EXPECTATION_FNS = {
    "square": lambda x: (x ** 2).sum(dim=-1, keepdims=True),
    "abs": lambda x: x.abs().sum(dim=-1, keepdims=True),
    "sum": lambda x: x.sum(dim=-1, keepdims=True),
    "square_minus_sum": lambda x: (x ** 2 - x).sum(dim=-1, keepdims=True),
}


class Distribution(torch.nn.Module):
    def __init__(self, dim: int, log_norm_const: float | None = None, domain=None, n_reference_samples=None,
                 grid_points=None, **kwargs):
        super().__init__()
        self.dim = dim
        self.log_norm_const = log_norm_const
        self.n_reference_samples = n_reference_samples
        self.grid_points = grid_points
        self.expectations = {}
        self.set_domain(domain)

    def set_domain(self, d=None):
        if d is not None:
            d = d if isinstance(d, torch.Tensor) else torch.tensor(d, dtype=torch.float)
            if d.ndim == 0:
                d = torch.stack([-d, d], dim=-1)
            if d.ndim == 1:
                d = d.unsqueeze(0)
            if d.shape == (1, 2):
                d = d.repeat(self.dim, 1)
            assert d.shape == (self.dim, 2)
        self.register_buffer("domain", d, persistent=False)

    def compute_stats(self):
        """Reference statistics need 1e7 samples / quadrature (distr/base.py:60-118): out of the hot path."""

    def has_entropy(self):
        return False

    def unnorm_log_prob(self, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        if self.log_norm_const is None:
            raise NotImplementedError
        return self.unnorm_log_prob(x) - self.log_norm_const

    def pdf(self, x):
        return self.log_prob(x).exp()

    def unnorm_pdf(self, x):
        return self.unnorm_log_prob(x).exp()

    def score(self, x: torch.Tensor, create_graph=False) -> torch.Tensor:
        """Autograd score (the reference's default, distr/base.py:146-154)."""
        flag = x.requires_grad
        x.requires_grad_(True)
        with torch.set_grad_enabled(True):
            total = self.unnorm_log_prob(x).sum()
            out = torch.autograd.grad(total, x, create_graph=create_graph)[0]
        x.requires_grad_(flag)
        return out

    def forward(self, x):
        return self.unnorm_log_prob(x)


class WrapperDistrNN(Distribution):
    """distr/base.py:186-198: an energy-based model at one time ``t`` as a distribution -- the reference distribution of RDS with
    ``ref_type='nn'`` (solver/oc.py:584), ``t`` = eps, the start of the time grid.  ``log_prob`` of a tilted potential of this package is
    one ``engine.tilted_eval`` launch; the time travels as the (1, 1) tensor made here once, so its table is read back once."""

    def __init__(self, dim, net, t):
        super().__init__(dim=dim, log_norm_const=0.0)
        self.net = net
        self.t = t
        self._t_row = torch.as_tensor(t).reshape(1, 1)

    def unnorm_log_prob(self, x: torch.Tensor) -> torch.Tensor:
        if hasattr(self.net, "_eval"):  # this package's potentials take one time for all rows
            return self.net.unnorm_log_prob(self._t_row.to(x.device) if self._t_row.device != x.device else self._t_row, x)
        return self.net.unnorm_log_prob(self.t * torch.ones((x.shape[0], 1), device=x.device), x)


class ModeWeightMetrics:
    """The sample-based diagnostics of the multi-modal targets (``distr/gauss.py:245-293``, ``distr/rings.py:111-160``,
    ``distr/checkerboard.py:93-140``): entropy of the empirical mode weights, their KL / TV distance to the true weights and the share
    of forgotten modes.  A class provides ``compute_mode_count(samples)`` and ``_true_mode_probs()``; ``_mode_hist`` turns the counts
    into the empirical weights.  Host-side torch on the samples' device."""

    def has_entropy(self):
        return True

    def _mode_hist(self, counts):
        return counts.flatten() / counts.sum()

    def _true_hist(self, like):
        probs = self._true_mode_probs().to(like.device).flatten()
        return probs / probs.sum()

    def entropy(self, samples, counts=None):
        if counts is None:
            counts = self.compute_mode_count(samples)
        hist = self._mode_hist(counts)
        return -torch.sum(hist * (torch.log(hist) / math.log(counts.shape[0])))

    def kl_weights(self, samples, counts=None):
        if counts is None:
            counts = self.compute_mode_count(samples)
        hist = self._mode_hist(counts)
        true_hist = self._true_hist(hist)
        return torch.sum(true_hist * torch.log(true_hist / hist))

    def tv_weights(self, samples, counts=None):
        if counts is None:
            counts = self.compute_mode_count(samples)
        hist = self._mode_hist(counts)
        return torch.sum(torch.abs(hist - self._true_hist(hist)))

    def compute_forgotten_modes(self, samples, tol=0.05, counts=None):
        if counts is None:
            counts = self.compute_mode_count(samples)
        hist = self._mode_hist(counts)
        return torch.sum(hist < tol * self._true_hist(hist).min()) / self.n_mixtures


def sample_uniform(domain: torch.Tensor, batchsize: int = 1) -> torch.Tensor:
    lo, hi = domain[:, 0], domain[:, 1]
    return lo + torch.rand(batchsize, domain.shape[0], device=domain.device) * (hi - lo)
