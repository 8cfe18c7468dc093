"""Time ``net.energy`` forward + backward of an energy-based reference with ``param_grads = True`` -- one sdeng_tilted_vjp launch, the
weight-gradient products of engine.tilted_param_grads and the time-embedding pass -- against the torch composition of the same
arithmetic with autograd on the same GPU: what a user had before the kernel.

    python tools/probe_tilted_train.py [--reps 30] > profiles/tilted_train.log

Shapes: those of tools/probe_tilted_eval.py -- the phi^4 trainer shape (100 levels x 256 rows, d = 100, K = 4 full covariances), also at
twice the rows (positives + negatives in one call), and the logistic-regression batch (6 000 rows at one time, d = 61, one Gaussian).
Loss: mean(E) + 0.1 mean(E^2) (the trainer's, with reg_val).  Warm-up, then the median and minimum of --reps timed calls (events around
each call, packed images cached); both sides in the same process.  The split: the launch alone (tilted_vjp), the evaluation launch
without the arrays (tilted_eval with grad: the same walk), the products alone (tilted_param_grads on arrays already there); the round
trip of the arrays is the launch minus the evaluation (written once) plus what the products spend reading them.
SDENG_LIB = another build of the library (tools/probe_lib.py); the "@time" lines are for an A/B of two builds, as in probe_tilted_eval.py."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probe_tilted_eval import LIB, at_time, timed  # noqa: E402
from sde_sampler_lrds_amd import engine as E  # noqa: E402
from sde_sampler_lrds_amd.eq.sdes import VP  # noqa: E402
from sde_sampler_lrds_amd.models.mlp import FourierMLP  # noqa: E402
from sde_sampler_lrds_amd.models.reparam import GaussTiltedPotential, GMMTitledPotential  # noqa: E402


def torch_energy(net, D, P):
    """(t [M,1], x) -> E [M] in torch with a graph to the parameters: models/reparam.py:354-451 with the prior in eigen form."""
    means = net.means if hasattr(net, "means") else net.mean.unsqueeze(0)
    w = net.weights if hasattr(net, "weights") else torch.ones(1, device=means.device)
    logw = torch.log(w / w.sum())

    def fn(t, x):
        s, sig = net.sde.s(t), net.sde.sigma_sq(t)
        xs = (x - s * net.mean_gauss) / (s * torch.sqrt(net.var_gauss + sig))
        base = -(net.base_model(t, xs) * xs).sum(-1)
        z = x.unsqueeze(1) - s.unsqueeze(1) * means.unsqueeze(0)
        var = (s * s).unsqueeze(1) * (D.unsqueeze(0) + sig.unsqueeze(1))
        y = torch.einsum("kij,mki->mkj", P, z) if P is not None else z
        lps = logw - 0.5 * (x.shape[1] * 1.8378770664093453 + torch.log(var).sum(-1) + (y * y / var).sum(-1))
        return -(torch.logsumexp(lps, dim=-1) + base)
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    print(f"# device {torch.cuda.get_device_name(0)}; library {LIB}; median (min) of {a.reps} calls after 5 warm-up calls, ms")
    slower = []
    for name, d, K, N, B in (("phi4 trainer, positives", 100, 4, 100, 256), ("phi4 trainer, positives + negatives", 100, 4, 100, 512),
                             ("logistic-regression batch", 61, 1, 1, 6000)):
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
        net = net.to(dev)
        net.param_grads = True
        params = list(net.parameters())
        t = torch.linspace(0.05, 0.95, N).repeat_interleave(B).reshape(-1, 1).to(dev)
        x = (net.sde.s(t) * (net.mean_gauss + torch.sqrt(net.var_gauss + net.sde.sigma_sq(t)) * torch.randn(N * B, d, generator=g).to(dev))).contiguous()
        ref = torch_energy(net, Dm.to(dev), None if Pm is None else Pm.to(dev))

        def step(energy):
            en = energy(t, x)
            return torch.autograd.grad(en.mean() + 0.1 * torch.square(en).mean(), params)
        g_k, g_t = step(net.energy), step(ref)
        agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(g_k, g_t))
        hip, tor = timed(lambda: step(net.energy), a.reps), timed(lambda: step(ref), a.reps)
        with torch.no_grad():
            _, _, arrays, (n, b, tu) = E.tilted_vjp(net, t, x)
            cot = torch.full((N * B,), 1.0 / (N * B), device=dev)
            launch = timed(lambda: E.tilted_vjp(net, t, x), a.reps)
            evalu = timed(lambda: E.tilted_eval(net, t, x), a.reps)
            prods = timed(lambda: E.tilted_param_grads(net, arrays, cot, n, b, tu), a.reps)
        mb = N * B * (1280 + 2 * d) * 4 / 1e6
        print(f"{name}: M = {N} x {B} = {N * B}, d = {d}, K = {K} ({'full covariances' if K > 1 else 'diagonal'}); parameter gradients agree to "
              f"{agree:.1e} of each tensor's largest entry; per-row arrays {mb:.0f} MB")
        print(f"  energy forward + backward   HIP path {hip[0]:8.3f} ({hip[1]:.3f})   torch + autograd {tor[0]:8.3f} ({tor[1]:.3f})   "
              f"torch / HIP = {tor[0] / hip[0]:.2f}")
        print(f"  split of the HIP path       sdeng_tilted_vjp launch {launch[0]:.3f} ({launch[1]:.3f})   [sdeng_tilted_eval with grad, no arrays: "
              f"{evalu[0]:.3f} ({evalu[1]:.3f}); writing the arrays: {launch[0] - evalu[0]:+.3f}]   products + time embedding {prods[0]:.3f} ({prods[1]:.3f})   "
              f"rest (loss, autograd bookkeeping) {hip[0] - launch[0] - prods[0]:.3f}")
        at_time(f"train {name}, sdeng_tilted_vjp launch", launch)
        if hip[0] > tor[0]:
            slower.append(name)
    print("# the HIP path is slower than the torch composition at: " + (", ".join(slower) if slower else "no shape"))


if __name__ == "__main__":
    main()
