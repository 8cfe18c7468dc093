"""Fixtures of training an energy-based reference, tests/golden/tilted_train_*.npz: the REAL reference's GMMTitledPotential
(models/reparam.py:277-482) around its FourierMLP(num_layers=6, channels=128, GELU), ``net.energy(t, x)`` differentiated by its own
autograd with respect to every parameter, on the CPU in float32 and in float64 (``gen_golden.py`` sets up the reference's import path).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_tilted_train.py [case ...]

Inputs, mixture and state dict are those of the evaluation fixture of the same case (tests/golden/tilted_<case>.npz, named in ``base``);
the loss is ``tests/tilted_train_ref.loss_of``: L = sum_r w_r E_r + 0.1 mean(E^2), w = randn(M, seed + 13) / M.  Stored: ``w``, the
float64 gradient of every parameter rounded to float32 (``grad.<name>``), and in ``meta`` per tensor the error of the reference's own
float32 run, err32 = |g32 - g64|_inf / |g64|_inf (0 where the float64 gradient is exactly zero: case f).
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (sets up the reference's import path and its stand-in modules)
import torch  # noqa: E402

from tests import tilted_cases as tc  # noqa: E402
from tests import tilted_train_ref as tr  # noqa: E402


def run(net, t, x, w, dtype):
    for p in net.parameters():
        p.grad = None
    E = net.energy(t.to(dtype), x.to(dtype)).flatten()
    tr.loss_of(E, w).backward()
    return {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def make(case):
    fx = tc.Fixture(case)
    net32 = fx.build(gg.r_mlp, gg.r_rep, gg.r_sdes)
    net64 = fx.build(gg.r_mlp, gg.r_rep, gg.r_sdes, torch.float64)
    t, x = fx["t"], fx["x"]
    w = tr.weights(case, x.shape[0])
    g32, g64 = run(net32, t, x, w, torch.float32), run(net64, t, x, w, torch.float64)
    err32 = {n: tr.tensor_err(g32[n], g64[n]) for n in g64}
    meta = dict(case=case, base=case, M=int(x.shape[0]), names=list(g64), err32=err32)
    gg.save("tilted_train_" + case, meta, {"w": w.numpy(), **{"grad." + n: g.float().numpy() for n, g in g64.items()}})
    print(f"tilted_train_{case}: M={x.shape[0]} d={fx.spec['d']} reference float32 vs float64 per tensor: "
          f"{min(err32.values()):.1e} .. {max(err32.values()):.1e} (largest: {max(err32, key=err32.get)})")


def main():
    for c in sys.argv[1:] or list(tr.CASES):
        make(c)


if __name__ == "__main__":
    main()
