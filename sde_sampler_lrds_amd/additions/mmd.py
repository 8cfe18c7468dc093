"""Maximum mean discrepancy with a Gaussian kernel at the median bandwidth (``sde_sampler/additions/mmd.py:30-59``).  Upstream builds
three n x n matrices, an int64 ``triu_indices`` pair and their concatenation to take one median; here ``sdeng_mmd_median``
(csrc/metric_kernels.hip) finds the same lower median by radix selection and sums the kernels tile by tile: O(n) memory."""
from __future__ import annotations

import torch

from .. import engine as E


def mmd_median(X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    m, n = X.shape[0], Y.shape[0]
    assert n >= 2 and m >= 2
    assert n == m
    return E.mmd_median(X, Y)[0].to(X.dtype)
