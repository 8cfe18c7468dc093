"""Float64 restatement of what the tilted-potential kernel computes (csrc/tilted_kernel.hpp), from plain arrays: the FourierMLP forward
pass written out layer by layer, the ANALYTIC J^T xs (transposed weights, gelu' of the stored pre-activations -- no autograd) and the
noised-mixture prior in the eigen form.  tests/test_tilted_cpu.py holds it to the reference's own float64 outputs in the fixtures, which
pins the formulas; the sampler test uses it to choose a seed."""
from __future__ import annotations

import math

import torch

F64 = torch.float64


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def gelu_grad(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def sde_scalars(kind, args, t):
    """(s(t), sigma_sq(t)) of the VP (eq/sdes.py VP.s / sigma_sq) or the PinnedBM, in float64."""
    t = t.to(F64)
    args = {k: float(torch.tensor(v, dtype=torch.float32)) for k, v in args.items()}  # the SDE objects hold float32 buffers
    if kind == "vp":
        bmin, bmax, sc = args["diff_coeff_sq_min"], args["diff_coeff_sq_max"], args["scale_diff_coeff"]
        integral = 0.5 * (bmin * t + 0.5 * (bmax - bmin) * t * t / args["terminal_t"])  # int_0^t drift coefficient, sign dropped
        s = torch.exp(-integral)
        return s, sc ** 2 * (1.0 / (s * s) - 1.0)
    T, g = args["terminal_t"], args["diff_coeff"]
    return (T - t) / T, g ** 2 * t * T / (T - t)


class Restated:
    """sd: the state_dict of the potential (float tensors, any precision); mixture: (weights [K], means [K,d], variances) with variances
    [K,d], [K,d,d] or the tuple (D [K,d], P [K,d,d]); s_fn(t) -> (s, sigma_sq) float64 [M,1]."""

    def __init__(self, sd, mixture, s_fn, t_limit=0.0, use_s_t_scaling=False):
        self.p = {k: v.to(F64) for k, v in sd.items() if v.is_floating_point()}
        w, m, var = mixture
        self.w, self.m = w.to(F64), m.to(F64)
        if isinstance(var, tuple):
            self.D, self.P = var[0].to(F64), var[1].to(F64)
        elif var.dim() == 3:
            self.D, self.P = torch.linalg.eigh(var.to(F64))
        else:
            self.D, self.P = var.to(F64), None
        self.s_fn, self.t_limit, self.st = s_fn, t_limit, use_s_t_scaling
        self.coeff = torch.linspace(0.1, 100, 128).to(F64).unsqueeze(0)  # TimeEmbed.timestep_coeff: a float32 linspace (not persistent)

    def lin(self, name, v, transpose=False):
        W = self.p["base_model." + name + ".weight"]
        return v @ W if transpose else v @ W.T + self.p["base_model." + name + ".bias"]

    def net(self, t, xs, want_vjp):
        """v = FourierMLP(t, xs) and J^T xs."""
        ang = self.coeff * t.to(torch.float32).to(F64) + self.p["base_model.timestep_embed.timestep_phase"]
        e = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
        e = self.lin("timestep_embed.out_layer", gelu(self.lin("timestep_embed.hidden_layer.0", e)))
        h = [self.lin("input_embed", xs) + e]
        for l in range(4):
            h.append(self.lin(f"hidden_layer.{l}", gelu(h[-1])))
        v = self.lin("out_layer", gelu(h[-1]))
        if not want_vjp:
            return v, None
        dh = self.lin("out_layer", xs, transpose=True) * gelu_grad(h[4])
        for l in range(3, -1, -1):
            dh = self.lin(f"hidden_layer.{l}", dh, transpose=True) * gelu_grad(h[l])
        return v, self.lin("input_embed", dh, transpose=True)

    def prior(self, t, x):
        tl = torch.maximum(t, torch.full_like(t, self.t_limit))
        s, sig = self.s_fn(tl)  # [M,1]
        d = x.shape[1]
        w = self.w / self.w.sum()
        z = x.unsqueeze(1) - s.unsqueeze(1) * self.m.unsqueeze(0)  # [M,K,d]
        var = (s * s).unsqueeze(1) * (self.D.unsqueeze(0) + sig.unsqueeze(1))  # [M,K,d]
        if self.P is not None:
            y = torch.einsum("kij,mki->mkj", self.P, z)
            q = y / var
            maha, grad_k = (y * q).sum(-1), -torch.einsum("kij,mkj->mki", self.P, q)
        else:
            q = z / var
            maha, grad_k = (z * q).sum(-1), -q
        lps = torch.log(w).unsqueeze(0) - 0.5 * (d * math.log(2.0 * math.pi) + torch.log(var).sum(-1) + maha)
        return torch.logsumexp(lps, dim=-1), (torch.softmax(lps, dim=-1).unsqueeze(-1) * grad_k).sum(1)

    def __call__(self, t, x, want_grad=True):
        t, x = t.to(F64).reshape(-1, 1).expand(x.shape[0], 1), x.to(F64)
        s, sig = self.s_fn(t)
        ci = s * torch.sqrt(self.p["var_gauss"] + sig)
        xs = (x - s * self.p["mean_gauss"]) / ci
        v, jx = self.net(t, xs, want_grad)
        f = s.flatten() if self.st else torch.ones_like(s.flatten())
        plp, pgrad = self.prior(t, x)
        lp = plp + f * -(v * xs).sum(-1)
        if not want_grad:
            return lp, None
        return lp, pgrad + f.unsqueeze(-1) * (-(v + jx) / ci)


def from_fixture(fx):
    from tests import tilted_cases as tc
    spec = fx.spec
    w, m, var = fx.ctor_args()
    if spec["prior"] == "gauss":
        w, m, var = torch.ones(1), m.unsqueeze(0), var.unsqueeze(0)
    return Restated(fx.state_dict(), (w, m, var), lambda t: sde_scalars(spec["sde"], tc.SDE_ARGS[spec["sde"]], t), spec["t_limit"], spec["st"])
