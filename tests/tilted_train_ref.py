"""Training an energy-based reference: the fixtures tests/golden/tilted_train_*.npz (gen_golden_tilted_train.py), the loss they are
made with, and a float64 restatement WITHOUT autograd of the per-row arrays ``sdeng_tilted_vjp`` writes (include/sdeng.h), built on the
formulas of tests/tilted_ref.py.  Nothing here runs the reference."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from tests import tilted_cases as tc
from tests import tilted_ref
from tests.tilted_ref import F64, gelu, gelu_grad

CASES = ("a", "b", "c", "f")
REG = 0.1


def weights(case, M):
    """w = randn(M) / M from the case's seed + 13: the linear part of the loss."""
    return torch.randn(M, generator=torch.Generator().manual_seed(tc.CASES[case]["seed"] + 13)) / M


def loss_of(E, w):
    """L = sum_r w_r E_r + 0.1 mean(E^2): linear plus the trainer's ``reg_val`` term, so the cotangent depends on E itself."""
    return (w.to(E.dtype) * E).sum() + REG * torch.square(E).mean()


def cotangent(E, w):
    """dL/dE_r of ``loss_of``, written out."""
    return w.to(E.dtype) + 2.0 * REG * E / E.shape[0]


def path(case):
    return os.path.join(tc.GOLDEN_DIR, f"tilted_train_{case}.npz")


class TrainFixture:
    """w, the float64 parameter gradients rounded to float32 (``grad.<parameter name>``), and in ``meta`` the reference's own float32
    error per tensor; inputs, mixture and state dict are the evaluation fixture's of the same case (``base``)."""

    def __init__(self, case):
        z = np.load(path(case))
        self.case, self.meta = case, json.loads(bytes(z["meta"]).decode())
        self.base = tc.Fixture(self.meta["base"])
        self.w = torch.from_numpy(z["w"])
        self.grads = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("grad.")}
        self.err32 = self.meta["err32"]


def tensor_err(g, g64):
    """|g - g64|_inf / |g64|_inf of one parameter tensor (an all-zero g64: the absolute error)."""
    g, g64 = g.detach().double().cpu(), g64.double()
    scale = float(g64.abs().max())
    return float((g - g64).abs().max()) / (scale if scale > 0.0 else 1.0)


def rows64(R: tilted_ref.Restated, t, x):
    """(E [M], arrays) in float64: the energy and the per-row arrays of sdeng_tilted_vjp -- a[l] = gelu(h_l), d[l] = f dh_l with
    dh_4 = (W_out^T xs) gelu'(h_4), dh_l = (W_{l+1}^T dh_{l+1}) gelu'(h_l), xs, dv = f xs."""
    t, x = t.to(F64).reshape(-1, 1).expand(x.shape[0], 1), x.to(F64)
    s, sig = R.s_fn(t)
    xs = (x - s * R.p["mean_gauss"]) / (s * torch.sqrt(R.p["var_gauss"] + sig))
    ang = R.coeff * t.to(torch.float32).to(F64) + R.p["base_model.timestep_embed.timestep_phase"]
    e = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    e = R.lin("timestep_embed.out_layer", gelu(R.lin("timestep_embed.hidden_layer.0", e)))
    h = [R.lin("input_embed", xs) + e]
    for l in range(4):
        h.append(R.lin(f"hidden_layer.{l}", gelu(h[-1])))
    a = [gelu(v) for v in h]
    v = R.lin("out_layer", a[4])
    f = (s.flatten() if R.st else torch.ones_like(s.flatten())).unsqueeze(-1)
    dh = [None] * 5
    dh[4] = R.lin("out_layer", xs, transpose=True) * gelu_grad(h[4])
    for l in range(3, -1, -1):
        dh[l] = R.lin(f"hidden_layer.{l}", dh[l + 1], transpose=True) * gelu_grad(h[l])
    E = -R.prior(t, x)[0] + f.flatten() * (v * xs).sum(-1)
    return E, {"a": a, "d": [f * g for g in dh], "xs": xs, "dv": f * xs}


def layout(fx):
    """(N, B, t_unique [N] float32) of a case's rows."""
    spec = fx.spec
    return len(spec["times"]), spec["B"], torch.tensor(spec["times"], dtype=torch.float32)


def restated_param_grads(case, t=None, x=None, cot_fn=None):
    """{parameter name: float64 gradient} of ``loss_of`` at a case's rows (or at the given (t, x), one time per equal run, with
    ``cot_fn(E)`` the cotangent), through the float64 mirror and ``engine.tilted_param_grads`` -- no autograd but the time embedding's."""
    from sde_sampler_lrds_amd import engine as E_
    fx, net = tc.mirror(case, torch.float64)
    if t is None:
        t, x = fx["t"], fx["x"]
        N, B, tu = layout(fx)
        w = weights(case, x.shape[0])
        cot_fn = lambda E: cotangent(E, w)  # noqa: E731
    else:
        N, B, tinfo = E_.tilted_times(net, t, x.shape[0])
        tu = tinfo[:, 0]
    E, arrays = rows64(tilted_ref.from_fixture(fx), t, x)
    grads = E_.tilted_param_grads(net, arrays, cot_fn(E), N, B, tu)
    names = {p: n for n, p in net.named_parameters()}
    return E, {names[p]: g for p, g in grads.items()}
