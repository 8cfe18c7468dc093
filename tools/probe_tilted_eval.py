"""Time sdeng_tilted_eval (log-density and score of an energy-based reference, one launch) against the torch composition of the same
arithmetic on the same GPU, autograd for the gradient -- what a user had before the kernel.

    python tools/probe_tilted_eval.py [--reps 30] > profiles/tilted_eval.log

Shapes: the phi^4 replica-exchange move (100 levels x 256 chains, d = 100, K = 4 full covariances) and the logistic-regression
evaluation batch (6 000 rows at one time, d = 61, one Gaussian).  Warm-up, then the median of --reps timed calls (hip events around
each call, the packed images already cached -- as in a sampler's loop); both sides on the same device in the same process.  The torch
side works in the same eigen form (one [d,d] product per component and direction), float32, with the time scalars precomputed.
SDENG_LIB = another build of the library (tools/probe_lib.py); the "@time" lines (label | median q1 q3, ms) are for an A/B of two builds."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_lib  # noqa: E402

LIB = probe_lib.select()
from sde_sampler_lrds_amd import engine as E  # noqa: E402
from sde_sampler_lrds_amd.eq.sdes import VP  # noqa: E402
from sde_sampler_lrds_amd.models.mlp import FourierMLP  # noqa: E402
from sde_sampler_lrds_amd.models.reparam import GaussTiltedPotential, GMMTitledPotential  # noqa: E402


def torch_composition(net, D, P):
    """(t [M,1], x) -> (log_prob, grad) in torch: the arithmetic of models/reparam.py:354-476 with the prior in eigen form."""
    means = net.means if hasattr(net, "means") else net.mean.unsqueeze(0)
    w = net.weights if hasattr(net, "weights") else torch.ones(1, device=means.device)
    logw = torch.log(w / w.sum())

    def fn(t, x):
        with torch.enable_grad():
            x = x.detach().requires_grad_(True)
            s, sig = net.sde.s(t), net.sde.sigma_sq(t)
            xs = (x - s * net.mean_gauss) / (s * torch.sqrt(net.var_gauss + sig))
            base = -(net.base_model(t, xs) * xs).sum(-1)
            z = x.unsqueeze(1) - s.unsqueeze(1) * means.unsqueeze(0)
            var = (s * s).unsqueeze(1) * (D.unsqueeze(0) + sig.unsqueeze(1))
            y = torch.einsum("kij,mki->mkj", P, z) if P is not None else z
            lps = logw - 0.5 * (x.shape[1] * 1.8378770664093453 + torch.log(var).sum(-1) + (y * y / var).sum(-1))
            lp = torch.logsumexp(lps, dim=-1) + base
            return lp.detach(), torch.autograd.grad(lp.sum(), x)[0]
    return fn


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), min(ms), q[0], q[2]


def at_time(label, m):
    print(f"@time {label} | {m[0]:.4f} {m[2]:.4f} {m[3]:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    print(f"# device {torch.cuda.get_device_name(0)}; library {LIB}; median (min) of {a.reps} calls after 5 warm-up calls, ms")
    slower = []
    for name, d, K, N, B in (("phi4 replica-exchange move", 100, 4, 100, 256), ("logistic-regression evaluation", 61, 1, 1, 6000)):
        base = FourierMLP(dim=d, activation=torch.nn.GELU(), num_layers=6, channels=128)
        with torch.no_grad():
            base.out_layer.weight.copy_(0.1 * torch.randn(base.out_layer.weight.shape, generator=g))
        sde = VP(0.1, 10.0, 1.0, terminal_t=1.0)
        means = 1.5 * torch.randn(K, d, generator=g)
        if K > 1:
            Pm = torch.linalg.qr(torch.randn(K, d, d, generator=g)).Q.contiguous()
            Dm = 0.1 + 0.9 * torch.rand(K, d, generator=g)
            net = GMMTitledPotential(base, sde, 0.5 + torch.rand(K, generator=g), means, (Dm, Pm))
        else:
            Pm, Dm = None, 0.2 + 0.8 * torch.rand(1, d, generator=g)
            net = GaussTiltedPotential(base, sde, means[0], Dm[0])
        net = net.to(dev).requires_grad_(False)
        t = torch.linspace(0.05, 0.95, N).repeat_interleave(B).reshape(-1, 1).to(dev)
        x = (net.sde.s(t) * (net.mean_gauss + torch.sqrt(net.var_gauss + net.sde.sigma_sq(t)) * torch.randn(N * B, d, generator=g).to(dev))).contiguous()
        ref = torch_composition(net, Dm.to(dev), None if Pm is None else Pm.to(dev))
        lp_k, g_k = E.tilted_eval(net, t, x)
        lp_t, g_t = ref(t, x)
        agree = max(float(((lp_k - lp_t).abs() / (1 + lp_t.abs())).max()), float(((g_k - g_t).abs().amax(1) / (1 + g_t.abs().amax(1))).max()))
        k_both, t_both = timed(lambda: E.tilted_eval(net, t, x), a.reps), timed(lambda: ref(t, x), a.reps)
        k_lp = timed(lambda: E.tilted_eval(net, t, x, want_grad=False), a.reps)
        print(f"{name}: M = {N} x {B} = {N * B}, d = {d}, K = {K} ({'full covariances' if K > 1 else 'diagonal'}); kernel vs torch agree to {agree:.1e}")
        print(f"  log_prob + grad   sdeng_tilted_eval {k_both[0]:8.3f} ({k_both[1]:.3f})   torch + autograd {t_both[0]:8.3f} ({t_both[1]:.3f})   "
              f"torch / kernel = {t_both[0] / k_both[0]:.2f}")
        print(f"  log_prob only     sdeng_tilted_eval {k_lp[0]:8.3f} ({k_lp[1]:.3f})")
        at_time(f"eval {name}, log_prob + grad", k_both)
        at_time(f"eval {name}, log_prob only", k_lp)
        if k_both[0] > t_both[0]:
            slower.append(name)
    print("# the kernel is slower than the torch composition at: " + (", ".join(slower) if slower else "neither shape"))


if __name__ == "__main__":
    main()
