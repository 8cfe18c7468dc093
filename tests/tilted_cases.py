"""The cases of the tilted-potential (EBM) fixtures tests/golden/tilted_*.npz: their shapes, how their inputs are drawn and how a
fixture is turned back into an object -- of the reference's classes (tests/golden/gen_golden_tilted.py) or of this package's mirrors
(the tests).  Nothing here runs the reference."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# case -> d, prior ('diag' | 'eig' = the (D, P) tuple | 'cov' = [K,d,d] matrices | 'gauss'), K, times, rows per time, and what it reaches
CASES = {
    # d << 16, a 16-row tile spanning three times, pad rows
    "a": dict(d=2, prior="diag", K=4, times=[0.15, 0.5, 0.85], B=5, sde="vp", t_limit=0.0, st=False, seed=501),
    # a tile straddling a time boundary; use_s_t_scaling
    "b": dict(d=16, prior="eig", K=3, times=[0.3, 0.7], B=24, sde="vp", t_limit=0.0, st=True, seed=502),
    # the phi^4 recipe's shape class, d no multiple of 16; t_limit > 0 with one t below it and one t = 0
    "c": dict(d=100, prior="cov", K=2, times=[0.0, 0.02, 0.3, 0.8], B=33, sde="vp", t_limit=0.05, st=False, seed=503),
    # logistic-regression recipe: one Gaussian, a single time near the end of a PinnedBM
    "d": dict(d=61, prior="gauss", K=1, times=[0.9], B=70, sde="pbm", t_limit=0.0, st=False, seed=504),
    # every row its own time (N = M)
    "e": dict(d=16, prior="diag", K=16, times=[0.05 + 0.06 * i for i in range(16)], B=1, sde="vp", t_limit=0.0, st=False, seed=505),
    # b with the recipe's all-zero last layer: the net term contributes exactly 0
    "f": dict(d=16, prior="eig", K=3, times=[0.3, 0.7], B=24, sde="vp", t_limit=0.0, st=True, seed=502, zero_last=True),
}
WALK_PRIORS = ("diag", "eig")


def walk_spec(nt, prior):
    """A drawn (not stored) case per kernel instance: NT = ``nt`` feature tiles at d = 16 nt - 3 -- never a multiple of four, so the last quad
    of a row is partly pad --, K = 2 components, three times x 11 rows = 33 rows: three tiles whose boundaries straddle the times, the last
    with 15 pad rows.  The fixtures reach NT = 1, 4 and 7 only."""
    return dict(d=16 * nt - 3, prior=prior, K=2, times=[0.2, 0.5, 0.8], B=11, sde="vp", t_limit=0.0, st=prior == "eig", seed=600 + nt)


SDE_ARGS = {"vp": dict(diff_coeff_sq_min=0.1, diff_coeff_sq_max=10.0, scale_diff_coeff=1.0, terminal_t=1.0),
            "pbm": dict(diff_coeff=1.5, terminal_t=1.0)}


def make_sde(mod, kind):
    """``mod``: an eq.sdes module (the reference's or the mirror)."""
    return (mod.VP if kind == "vp" else mod.PinnedBM)(**SDE_ARGS[kind])


def draw_mixture(spec, g):
    """Constructor arguments of the prior, float32: (weights, means, variances) -- variances [K,d], the (D, P) tuple or [K,d,d];
    for 'gauss' (mean [d], variance [d])."""
    d, K = spec["d"], spec["K"]
    means = 1.5 * torch.randn(K, d, generator=g)
    weights = 0.5 + torch.rand(K, generator=g)
    if spec["prior"] in ("diag", "gauss"):
        var = 0.2 + 0.8 * torch.rand(K, d, generator=g)
    else:
        P = torch.linalg.qr(torch.randn(K, d, d, generator=g)).Q.contiguous()
        D = 0.1 + 0.9 * torch.rand(K, d, generator=g)
        if spec["prior"] == "eig":
            var = (D, P)
        else:  # covariance matrices, exactly symmetric in float32 (the einsum's two triangles round differently)
            cov = torch.einsum("kia,ka,kja->kij", P, D, P)
            var = (0.5 * (cov + cov.transpose(-1, -2))).contiguous()
    if spec["prior"] == "gauss":
        return None, means[0], var[0]
    return weights, means, var


def draw_net_(net, spec, g):
    """In place: every parameter from the seeded generator, at nn.Linear's own scale (uniform +-1/sqrt(fan_in)); the last layer at
    O(0.1) -- or zero (the recipe's initialisation) for the zero_last case."""
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name == "timestep_embed.timestep_phase":
                p.copy_(torch.randn(p.shape, generator=g))
            elif name.startswith("out_layer."):
                p.copy_(torch.zeros(p.shape) if spec.get("zero_last") else 0.1 * torch.randn(p.shape, generator=g))
            else:
                fan_in = p.shape[1] if p.dim() == 2 else net.channels
                if name == "input_embed.bias":
                    fan_in = spec["d"]
                if name == "timestep_embed.hidden_layer.0.bias":
                    fan_in = 2 * net.channels
                p.copy_((2.0 * torch.rand(p.shape, generator=g) - 1.0) / fan_in ** 0.5)
    return net


def build(spec, mlp_mod, rep_mod, sde_mod, args=None, dtype=torch.float32):
    """A tilted potential of the classes in ``rep_mod`` / ``mlp_mod`` / ``sde_mod`` for ``spec``; ``args``: the stored constructor
    arguments (else drawn from the case's seed)."""
    g = torch.Generator().manual_seed(spec["seed"])
    drawn = draw_mixture(spec, g)
    weights, means, var = args if args is not None else drawn
    cast = lambda v: tuple(u.to(dtype) for u in v) if isinstance(v, tuple) else (None if v is None else v.to(dtype))  # noqa: E731
    base = mlp_mod.FourierMLP(dim=spec["d"], activation=torch.nn.GELU(), num_layers=6, channels=128)
    draw_net_(base, spec, g)
    sde = make_sde(sde_mod, spec["sde"])
    if spec["prior"] == "gauss":
        net = rep_mod.GaussTiltedPotential(base, sde, cast(means), cast(var), t_limit=spec["t_limit"], tilt_type="dot",
                                           use_s_t_scaling=spec["st"])
    else:
        net = rep_mod.GMMTitledPotential(base, sde, cast(weights), cast(means), cast(var), t_limit=spec["t_limit"],
                                         use_s_t_scaling=spec["st"], tilt_type="dot")
    return net.to(dtype)


def draw_inputs(spec, net):
    """(t [M,1], x [M,d]): states spread like the noised prior's Gaussian approximation."""
    g = torch.Generator().manual_seed(spec["seed"] + 7)
    N, B, d = len(spec["times"]), spec["B"], spec["d"]
    t = torch.tensor(spec["times"], dtype=torch.float32).repeat_interleave(B).reshape(-1, 1)
    s, sig = net.sde.s(t), net.sde.sigma_sq(t)
    z = torch.randn(N * B, d, generator=g)
    x = s * net.mean_gauss + s * torch.sqrt(net.var_gauss + sig) * z
    return t, x.to(torch.float32).contiguous()


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def path(case):
    return os.path.join(GOLDEN_DIR, f"tilted_{case}.npz")


def ctor_arrays(args):
    weights, means, var = args
    out = {"ctor.means": means}
    if weights is not None:
        out["ctor.weights"] = weights
    if isinstance(var, tuple):
        out["ctor.cov_D"], out["ctor.cov_P"] = var
    else:
        out["ctor.variances"] = var
    return out


class Fixture:
    def __init__(self, case):
        z = np.load(path(case))
        self.case = case
        self.meta = json.loads(bytes(z["meta"]).decode())
        self.spec = CASES[case]
        self.a = {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}
        src = self.a
        if "base" in self.meta:  # inputs, mixture and weights are another case's (the last layer apart)
            src = Fixture(self.meta["base"]).a
            for k, v in src.items():
                if not k.startswith("out.") and k not in self.a:
                    self.a[k] = v

    def __getitem__(self, k):
        return self.a[k]

    def ctor_args(self):
        var = (self.a["ctor.cov_D"], self.a["ctor.cov_P"]) if "ctor.cov_D" in self.a else self.a["ctor.variances"]
        return self.a.get("ctor.weights"), self.a["ctor.means"], var

    def state_dict(self):
        sd = {k[3:]: v.clone() for k, v in self.a.items() if k.startswith("sd.")}
        if self.spec.get("zero_last"):
            for k in sd:
                if k.startswith("base_model.out_layer."):
                    sd[k].zero_()
        return sd

    def build(self, mlp_mod, rep_mod, sde_mod, dtype=torch.float32):
        net = build(self.spec, mlp_mod, rep_mod, sde_mod, self.ctor_args(), dtype)
        net.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in self.state_dict().items()})
        return net


def mirror(case, dtype=torch.float32):
    from sde_sampler_lrds_amd.eq import sdes
    from sde_sampler_lrds_amd.models import mlp, reparam
    fx = Fixture(case)
    return fx, fx.build(mlp, reparam, sdes, dtype)


def err(a, ref64):
    """max over rows of |a - f64|_inf / (1 + |f64|_inf), a and ref64 [M] or [M, d]."""
    a, r = a.double().reshape(ref64.shape[0], -1), ref64.double().reshape(ref64.shape[0], -1)
    return float(((a - r).abs().amax(dim=1) / (1.0 + r.abs().amax(dim=1))).max())
