"""Sliced Kolmogorov-Smirnov distance (``sde_sampler/additions/ks.py:9-71``).  Linear in the sample size, so a torch composition --
but on the samples' device and batched over the projections, where upstream copies the samples to the CPU and loops one
``torch.histogram`` per projection.  The binning restates ``torch.histogram``: ``n_bins`` uniform bins over [min, max] of the
first sample's projection, the last bin closed on the right, values outside dropped, each histogram normalised by its own sum."""
from __future__ import annotations

import torch


def compute_random_proj_cdf(samples, random_projs, n_bins, min_x=None, max_x=None, weights=None, return_min_max=False):
    """CDF [n_random_projections, n_bins] of the projected samples (additions/ks.py:9-38)."""
    proj = torch.matmul(random_projs, samples.T)  # [P, B]
    if min_x is None and max_x is None:
        min_x, max_x = proj.min(dim=-1).values, proj.max(dim=-1).values
    lo, hi = min_x.unsqueeze(-1), max_x.unsqueeze(-1)
    pos = (proj - lo) / (hi - lo) * n_bins
    inside = (proj >= lo) & (proj <= hi)
    idx = pos.floor().clamp_(0, n_bins - 1).long()  # pos == n_bins (the maximum) falls into the last bin
    w = inside.to(proj.dtype) if weights is None else inside.to(proj.dtype) * weights.flatten().to(proj.dtype).unsqueeze(0)
    hist = torch.zeros(proj.shape[0], n_bins, dtype=proj.dtype, device=proj.device).scatter_add_(1, idx, w)
    hist = hist / hist.sum(dim=-1, keepdim=True)
    cdf = hist.cumsum(dim=-1)
    return (cdf, min_x, max_x) if return_min_max else cdf


def compute_sliced_ks(samples1, samples2, weights=None, n_random_projections=128, n_bins=256, random_projs=None):
    """Mean over random 1-D projections of the largest CDF gap (additions/ks.py:41-71).  The projections are drawn on the CPU from
    torch's global generator exactly as upstream does (same seed, same projections) unless ``random_projs`` [P, dim] is given."""
    if random_projs is None:
        random_projs = torch.randn((n_random_projections, samples1.shape[-1]))
        random_projs /= torch.linalg.norm(random_projs, axis=-1)[..., None]
    random_projs = random_projs.to(samples1.device, samples1.dtype)
    samples2 = samples2.to(samples1.device)
    if weights is not None:
        weights = weights.to(samples1.device)
    cdf1, min_x, max_x = compute_random_proj_cdf(samples1, random_projs, n_bins=n_bins, return_min_max=True)
    cdf2 = compute_random_proj_cdf(samples2, random_projs, n_bins=n_bins, min_x=min_x, max_x=max_x, weights=weights)
    return torch.max(torch.abs(cdf1 - cdf2), dim=-1).values.mean()
