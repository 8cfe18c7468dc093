"""2-D checkerboard target (``sde_sampler/distr/checkerboard.py``, conf/target/checkerboard.yaml): a mixture of ``2 * width`` uniform
squares of side 2 on alternating cells of the domain [-4, -4 + 2 width] x [-4, 4], the even-numbered squares three times as likely as
the odd ones (``unequilibrated=True``).  Its log-density is -inf outside every square, and its score is zero everywhere (the
reference returns zeros instead of differentiating).  Host-side torch methods only; the simulate path reads the corner tables and
the per-square log-density through ``engine.dist_desc`` and evaluates both in HIP.  The sample-based diagnostics that
``eval/metrics.py`` reports (mode histogram, entropy, KL / TV of the mode weights, forgotten modes; reference :93-140) are host-side
torch on the samples' device."""
from __future__ import annotations

import torch

from .base import Distribution, ModeWeightMetrics


def square_corners(width: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(x_min, y_max) of every square: two rows of cells per band y_max in (4, 0) -- the upper row starts at x = -2, the lower one
    (y_max - 2) at x = -4 -- each row holding every other cell of the 2 * width wide domain."""
    xs, ys = [], []
    for top in (4, 0):
        for x0, y in ((-2, top), (-4, top - 2)):
            row = list(range(x0, -4 + 2 * width, 4))
            xs += row
            ys += [y] * len(row)
    return torch.tensor(xs, dtype=torch.float32), torch.tensor(ys, dtype=torch.float32)


class Checkerboard(ModeWeightMetrics, Distribution):
    def __init__(self, dim: int = 2, width: int = 4, unequilibrated: bool = True, n_reference_samples: int = int(1e5), **kwargs):
        if dim != 2:
            raise ValueError("The checkerboard is two-dimensional.")
        super().__init__(dim=2, log_norm_const=0.0, n_reference_samples=n_reference_samples, **kwargs)
        self.width = width
        x_min, y_max = square_corners(width)
        self.n_mixtures = int(x_min.numel())
        low = torch.stack([x_min, y_max - 2.0], dim=-1)
        high = torch.stack([x_min + 2.0, y_max], dim=-1)
        weights = torch.ones(self.n_mixtures)
        if unequilibrated:
            weights[0::2] = 3.0
        self.register_buffer("low", low, persistent=False)
        self.register_buffer("high", high, persistent=False)
        self.register_buffer("weights", weights, persistent=False)
        self.register_buffer("loc", (low + high) / 2.0, persistent=False)  # square centres
        if self.domain is None:
            self.set_domain(torch.tensor([[-4.0, -4.0 + 2 * width], [-4.0, 4.0]]))

    @property
    def distr(self) -> torch.distributions.MixtureSameFamily:
        """The mixture on the buffers' device (Uniform components are half-open: [low, high) per coordinate)."""
        comp = torch.distributions.Independent(torch.distributions.Uniform(self.low, self.high, validate_args=False), 1)
        return torch.distributions.MixtureSameFamily(torch.distributions.Categorical(self.weights), comp, validate_args=False)

    def sample(self, shape: tuple | None = None) -> torch.Tensor:
        return self.distr.sample(torch.Size(shape if shape is not None else ()))

    def unnorm_log_prob(self, x: torch.Tensor) -> torch.Tensor:
        return self.distr.log_prob(x).unsqueeze(-1)

    def score(self, x: torch.Tensor, create_graph=False) -> torch.Tensor:
        return torch.zeros_like(x)

    def compute_mode_count(self, samples):
        """Samples per cell of the 4 x ``width`` grid over the domain, rows = y bands from the bottom (reference :97-100: the
        transposed ``torch.histogramdd`` of the samples with bins (width, 4) over the domain; samples outside it are dropped)."""
        dom = self.domain.to(samples.device)
        lo, hi = dom[:, 0], dom[:, 1]
        bins = torch.tensor([self.width, 4], device=samples.device)
        inside = ((samples >= lo) & (samples <= hi)).all(dim=-1)
        cell = ((samples - lo) / (hi - lo) * bins).floor().long()
        cell = torch.minimum(cell.clamp_(min=0), bins - 1)  # the upper edges belong to the last cells
        flat = (cell[:, 1] * self.width + cell[:, 0])[inside]
        return torch.bincount(flat, minlength=4 * self.width).to(torch.float32).view(4, self.width)

    def _mode_hist(self, counts):
        """The cells that carry mass, in the reference's order (its ``hist_mask``, :52-57), over ALL counted samples."""
        cols = torch.arange(self.width, device=counts.device)
        mask = torch.stack([cols % 2 == 0, cols % 2 == 1, cols % 2 == 0, cols % 2 == 1], dim=0)
        return counts[mask].flatten() / counts.sum()

    def _true_mode_probs(self):
        return self.weights / self.weights.sum()
