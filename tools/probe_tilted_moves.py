"""Time the local moves of a sampler level over an energy-based reference as ONE launch (sdeng_tilted_moves) against the parent path --
the same sampler call with ``ebm_mle.NATIVE_MOVES = False``: one sdeng_tilted_eval launch and the dozen small torch kernels of mala_step /
heuristics_step_size per move.

    python tools/probe_tilted_moves.py [--reps 20] > profiles/tilted_moves.log

Shapes, 15 local moves each (the recipe's swap_frequency = 16):
  (i)   the phi^4 trainer's replica exchange: 100 levels x 256 chains, d = 100, K = 4 full covariances -- re_sampler, one swap step + 15 moves;
  (ii)  the toy recipes: d = 2, 3 levels x 128 chains, K = 4 diagonal                                   -- re_sampler, one swap step + 15 moves;
  (iii) 6 000 chains at one time, d = 61, one Gaussian                                                  -- smc_sampler, one level of 15 moves.
The swap step (two evaluations) and the samplers' bookkeeping are in every timing, equal on both sides.  Per shape three variants run
interleaved in the same process -- host loop, one launch with torch's noise, one launch with Philox noise -- after a warm-up of each;
a timing is a host clock around a call that ends in a device synchronise.  Reported: median, minimum and the quartiles of --reps calls;
a variant counts as slower than the host loop when its median exceeds the host loop's by more than the host loop's own interquartile
range.  SDENG_LIB = another build of the library (tools/probe_lib.py); the "@time" lines (label | median q1 q3, ms) are for an A/B of two
builds."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_lib  # noqa: E402

LIB = probe_lib.select()
from sde_sampler_lrds_amd.additions import ebm_mle  # noqa: E402
from sde_sampler_lrds_amd.eq.sdes import VP  # noqa: E402
from sde_sampler_lrds_amd.models.mlp import FourierMLP  # noqa: E402
from sde_sampler_lrds_amd.models.reparam import GaussTiltedPotential, GMMTitledPotential  # noqa: E402

MOVES = 15
SHAPES = (("(i) phi4 replica exchange", 100, 4, True, 100, 256), ("(ii) toy replica exchange", 2, 4, False, 3, 128),
          ("(iii) logistic-regression level", 61, 1, False, 1, 6000))
VARIANTS = (("host loop", False, False), ("one launch, torch noise", True, False), ("one launch, philox", True, True))


def make_net(d, K, full, g, dev):
    base = FourierMLP(dim=d, activation=torch.nn.GELU(), num_layers=6, channels=128)
    with torch.no_grad():
        base.out_layer.weight.copy_(0.1 * torch.randn(base.out_layer.weight.shape, generator=g))
    sde = VP(0.1, 10.0, 1.0, terminal_t=1.0)
    means = 1.5 * torch.randn(K, d, generator=g)
    if K == 1:
        net = GaussTiltedPotential(base, sde, means[0], 0.2 + 0.8 * torch.rand(d, generator=g))
    elif full:
        P = torch.linalg.qr(torch.randn(K, d, d, generator=g)).Q.contiguous()
        net = GMMTitledPotential(base, sde, 0.5 + torch.rand(K, generator=g), means, (0.1 + 0.9 * torch.rand(K, d, generator=g), P))
    else:
        net = GMMTitledPotential(base, sde, 0.5 + torch.rand(K, generator=g), means, 0.2 + 0.8 * torch.rand(K, d, generator=g))
    return net.to(dev).requires_grad_(False)


def quartiles(ms):
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), min(ms), q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    print(f"# device {torch.cuda.get_device_name(0)}; library {LIB}; {MOVES} local moves per call; median (min; quartiles) of {a.reps} interleaved calls after 3 warm-up calls each, ms")
    slower = []
    for name, d, K, full, N, B in SHAPES:
        net = make_net(d, K, full, g, dev)
        fn = ebm_mle.ebm_log_prob_and_grads(net)
        times = torch.linspace(0.05, 0.95, N).to(dev).view(-1, 1, 1).repeat(1, B, 1)
        t_rows = times.reshape(-1, 1)
        x_init = (net.sde.s(t_rows) * (net.mean_gauss + torch.sqrt(net.var_gauss + net.sde.sigma_sq(t_rows)) * torch.randn(N * B, d, generator=g).to(dev)))
        x_init = x_init.view(N, B, d).contiguous()

        def call(native, philox):
            ebm_mle.NATIVE_MOVES, ebm_mle.NATIVE_NOISE = native, philox
            steps = 0.02 * torch.ones(N, B, 1, device=dev)
            if N > 1:
                out = ebm_mle.re_sampler(x_init, times, fn, MOVES + 1, 0, MOVES + 1, steps, per_noise_init=True)
            else:
                out = ebm_mle.smc_sampler(x_init[0], times, fn, 0, MOVES, steps, reweight_threshold=0.0)
            return out[0], out[2]["local_acc"]

        ms = {v[0]: [] for v in VARIANTS}
        acc = {}
        for rep in range(-3, a.reps):
            for vname, native, philox in VARIANTS:
                torch.manual_seed(100 + max(rep, 0))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                samples, local_acc = call(native, philox)
                torch.cuda.synchronize()
                if rep >= 0:
                    ms[vname].append(1e3 * (time.perf_counter() - t0))
                acc[vname] = (samples, float(local_acc.mean()))
        same = float((acc["host loop"][0] - acc["one launch, torch noise"][0]).abs().max())
        print(f"{name}: {N} x {B} = {N * B} chains, d = {d}, K = {K} ({'full covariances' if full else 'diagonal'}); host loop and one launch under the "
              f"same seed differ by at most {same:.1e}; local acceptance {acc['host loop'][1]:.3f} / {acc['one launch, torch noise'][1]:.3f} / "
              f"{acc['one launch, philox'][1]:.3f}")
        host = quartiles(ms["host loop"])
        for vname, _, _ in VARIANTS:
            med, lo, q1, q3 = quartiles(ms[vname])
            print(f"  {vname:26s} {med:9.3f} ({lo:.3f}; {q1:.3f} .. {q3:.3f})   host loop / this = {host[0] / med:.2f}")
            if vname != "host loop":
                print(f"@time moves {name}, {vname} | {med:.4f} {q1:.4f} {q3:.4f}")
            if med > host[0] + (host[3] - host[2]):
                slower.append(f"{name} [{vname}]")
    ebm_mle.NATIVE_MOVES, ebm_mle.NATIVE_NOISE = True, False
    print("# the one launch is slower than the host loop, beyond the host loop's interquartile range, at: " + (", ".join(slower) if slower else "no shape"))


if __name__ == "__main__":
    main()
