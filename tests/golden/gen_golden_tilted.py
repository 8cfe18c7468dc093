"""Fixtures of the energy-based (tilted-potential) references, tests/golden/tilted_*.npz: the REAL reference's GMMTitledPotential /
GaussTiltedPotential (models/reparam.py:277-606) around its FourierMLP(num_layers=6, channels=128, GELU), run on the CPU in float32 and
in float64 on the same inputs (``gen_golden.py`` sets up the reference's import path).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_tilted.py [case ...]

The cases, their seeds and the way inputs and weights are drawn are in ``tests/tilted_cases.py``.  A fixture stores the inputs (t, x), the
constructor arguments of the prior, the state_dict (``sd.<key>``), the key list, and ``unnorm_log_prob_and_grad`` in both precisions
(``out.lp32``, ``out.grad32``, ``out.lp64``, ``out.grad64``).  The float64 run is the same object built from the same float32 numbers:
constructor arguments cast to double, the float32 state_dict loaded into it.
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (sets up the reference's import path and its stand-in modules)
import torch  # noqa: E402

from tests import tilted_cases as tc  # noqa: E402


def run(net, t, x, dtype):
    lp, grad = net.unnorm_log_prob_and_grad(t.to(dtype), x.to(dtype))
    return lp.detach(), grad.detach()


def make(case):
    spec = tc.CASES[case]
    if spec.get("zero_last"):  # inputs, mixture and weights of the base case; only the outputs are this fixture's own
        base = [c for c, s in tc.CASES.items() if s["seed"] == spec["seed"] and not s.get("zero_last")][0]
        fx = tc.Fixture(base)
        fx.spec = spec
        net32 = fx.build(gg.r_mlp, gg.r_rep, gg.r_sdes)
        net64 = fx.build(gg.r_mlp, gg.r_rep, gg.r_sdes, torch.float64)
        t, x = fx["t"], fx["x"]
        arrays, meta = {}, dict(case=case, base=base)
    else:
        g = torch.Generator().manual_seed(spec["seed"])
        args = tc.draw_mixture(spec, g)
        net32 = tc.build(spec, gg.r_mlp, gg.r_rep, gg.r_sdes)
        sd = {k: v.detach().clone() for k, v in net32.state_dict().items()}
        net64 = tc.build(spec, gg.r_mlp, gg.r_rep, gg.r_sdes, args, torch.float64)
        net64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
        t, x = tc.draw_inputs(spec, net32)
        arrays = dict(t=t, x=x, **tc.ctor_arrays(args), **{"sd." + k: v for k, v in sd.items()})
        meta = dict(case=case, keys=list(sd.keys()))
    lp32, g32 = run(net32, t, x, torch.float32)
    lp64, g64 = run(net64, t, x, torch.float64)
    meta.update({k: v for k, v in spec.items()}, M=int(x.shape[0]), err32_lp=tc.err(lp32, lp64), err32_grad=tc.err(g32, g64))
    arrays.update({"out.lp32": lp32, "out.grad32": g32, "out.lp64": lp64, "out.grad64": g64})
    gg.save("tilted_" + case, meta, {k: v.numpy() for k, v in arrays.items()})
    print(f"tilted_{case}: M={x.shape[0]} d={spec['d']} reference float32 vs float64: lp {meta['err32_lp']:.2e} grad {meta['err32_grad']:.2e}")


def main():
    for c in sys.argv[1:] or list(tc.CASES):
        make(c)


if __name__ == "__main__":
    main()
