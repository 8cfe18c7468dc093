"""The cases of the fixtures tests/golden/rds_nn_*.npz (RDS over an energy-based reference): which tilted fixture supplies the energy net,
the integrator, the time grid and how x0 is drawn; and how a fixture is turned back into objects of this package.  Nothing here runs the
reference (tests/golden/gen_golden_rds_nn.py does)."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from tests import tilted_cases as tc

B, N = 37, 8  # three 16-row tiles, 11 pad rows; the smallest grid that still has a first, an inner and a last step

# name -> tilted case (tests/tilted_cases.py), integrator, grid.  a: d = 2, diagonal K = 4, one feature tile.  b: d = 16, eigen-form prior,
# use_s_t_scaling.  c: d = 100 (seven tiles, the drift net staged in two pieces), full covariances, t_limit = 0.05 above the net time of
# the last step (0.03).  d: d = 61, one Gaussian on the PinnedBM, DDPM-like kernel; the grid runs from 0.1 (the PinnedBM's x gain t / s is infinite
# at s = 0, eq/sdes.py:658-678) to 0.9 and x0 has the PinnedBM's own scale at the first net time (from a unit normal on a grid that starts
# at 1e-4 the reference itself runs to |x| of a few hundred).
CASES = {
    "a_ei": dict(tilted="a", integrator="ei", seed=701),
    "b_ei": dict(tilted="b", integrator="ei", seed=702),
    "b_em": dict(tilted="b", integrator="em", seed=703),
    "c_ei": dict(tilted="c", integrator="ei", seed=704, grid=[0.0, 0.16, 0.32, 0.48, 0.64, 0.8, 0.9, 0.97, 1.0]),
    "d_ddpm": dict(tilted="d", integrator="ddpm_like", seed=705, start=0.1, end=0.9, x0="marginal"),
}
KIND = {"ei": "ei", "ddpm_like": "ddpm", "em": "em"}  # engine.coef_table's names


def grid(spec, steps=N):
    """float32 time grid [steps + 1]: the case's own, or uniform on [start, end] as get_timesteps (utils/common.py) makes it."""
    if "grid" in spec and steps == N:
        return torch.tensor(spec["grid"], dtype=torch.float32)
    return torch.linspace(spec.get("start", 0.0), spec.get("end", 1.0), steps + 1, dtype=torch.float32)


def draw_x0(spec, net, philox_normal, batch=B):
    """x0 [batch, d] float32 from the Philox normals of stream 1: unit normal, or (x0 = 'marginal') the Gaussian approximation of the
    prior noised to the first net time T - ts[0] -- ``net`` is the float32 potential."""
    z = philox_normal(spec["seed"], 0, 0, batch, net.dim, stream=1)
    if spec.get("x0") != "marginal":
        return z
    ts = grid(spec)
    t = (ts[-1] - ts[0]).reshape(1, 1)
    s, sig = net.sde.s(t), net.sde.sigma_sq(t)
    return (s * net.mean_gauss + s * torch.sqrt(net.var_gauss + sig) * z).to(torch.float32).contiguous()


def path(name):
    return os.path.join(tc.GOLDEN_DIR, (name if name.startswith("train_") else "rds_nn_" + name) + ".npz")


class Fixture:
    def __init__(self, name):
        z = np.load(path(name))
        self.name = name
        self.meta = json.loads(bytes(z["meta"]).decode())
        self.a = {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}
        self.spec = CASES[self.meta["case"]]

    def __getitem__(self, k):
        return self.a[k]

    def net(self, dtype=torch.float32):
        """The energy net: this package's mirror of the tilted fixture, parameters frozen as change_reference_type('nn') leaves them."""
        net = tc.mirror(self.spec["tilted"], dtype)[1]
        for p in net.parameters():
            p.requires_grad_(False)
        return net

    def ctrl(self, dtype=torch.float32):
        from sde_sampler_lrds_amd.models import mlp, reparam
        base = mlp.FourierMLP(dim=self.meta["d"], activation=torch.nn.GELU(), num_layers=4, channels=64)
        ctrl = reparam.ClippedCtrl(base_model=base, clip_model=self.meta["clip_model"])
        ctrl.load_state_dict({k[5:]: v for k, v in self.a.items() if k.startswith("ctrl.")})
        return ctrl.to(dtype)

    def target(self):
        from sde_sampler_lrds_amd.distr.gauss import GMM
        return GMM(dim=self.meta["d"], loc=self["tgt_loc"], scale=self["tgt_scale"], mixture_weights=self["tgt_w"])
