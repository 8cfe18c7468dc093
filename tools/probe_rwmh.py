"""Random-walk Metropolis in one launch (sdeng_rwmh_moves) against the host loop it replaces, in the reference's toy set-up
(experiments/sample_toy_gmm_mcmc.py:112-115): Checkerboard, x_init = target.loc, 16 chains per mode, 2048 warm-up moves, a data set of
50 000 points -- 128 chains, 2438 moves.  Three routes of ``mcmc_sample(mcmc_type='rwmh')`` in one process, alternating, host clock around
the whole call (it ends in the copy of the data set to the host): the host loop (``ebm_mle.NATIVE_MOVES = False``), one launch fed by
torch's generator (two small generator launches per move remain), one launch with Philox noise drawn in the kernel.  Then the call time of
``engine.rwmh_moves`` alone with Philox noise (device events; the k_dist_tables launch of a mixture target included) at B = 128, d = 2
and at B = 4096, d = 24 on a 3-component mixture.

    python tools/probe_rwmh.py [--reps 5]
    rocprofv3 --kernel-trace --stats ... -- python tools/probe_rwmh.py --kernel-only      (kernel time alone: k_chain_moves<1> in the stats)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sde_sampler_lrds_amd import engine as E  # noqa: E402
from sde_sampler_lrds_amd.additions import ebm_mle  # noqa: E402
from sde_sampler_lrds_amd.distr.checkerboard import Checkerboard  # noqa: E402
from sde_sampler_lrds_amd.distr.gauss import GMM  # noqa: E402
from sde_sampler_lrds_amd.experiments.benchmark_utils import mcmc_sample  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def data_set(dev, reps):
    target = Checkerboard()
    kw = dict(mcmc_type="rwmh", n_chains_per_mode=16, n_warmup_steps=2048, dataset_length=50000, shuffle=False)
    routes = {"host loop (NATIVE_MOVES = False)": (False, False), "one launch, torch noise": (True, False), "one launch, Philox noise": (True, True)}
    times, inside = {k: [] for k in routes}, {}
    for rep in range(reps + 1):  # pass 0 warms every route up
        for label, (native, philox) in routes.items():
            ebm_mle.NATIVE_MOVES, ebm_mle.NATIVE_NOISE = native, philox
            torch.manual_seed(rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = mcmc_sample(dev, target, target.loc, **kw)
            dt = time.perf_counter() - t0
            if rep:
                times[label].append(dt * 1e3)
            inside[label] = (tuple(out.shape), float(torch.isfinite(Checkerboard().unnorm_log_prob(out)).float().mean()))
    ebm_mle.NATIVE_MOVES, ebm_mle.NATIVE_NOISE = True, False
    print(f"# mcmc_sample(mcmc_type='rwmh'): checkerboard, 128 chains, 2048 + 390 moves; ms per call, median (min, max) of {reps} after one warm-up pass")
    base = median(times["host loop (NATIVE_MOVES = False)"])[0]
    for label in routes:
        med, lo, hi = median(times[label])
        print(f"{label:36s} {med:10.2f} ({lo:.2f}, {hi:.2f})   x{base / med:8.1f}   data set {inside[label][0]}, inside a square {inside[label][1]:.3f}")


def kernel_cases(dev):
    g = torch.Generator().manual_seed(4)
    cb = Checkerboard().to(dev)
    gmm = GMM(dim=24, loc=2.0 * torch.randn(3, 24, generator=g), scale=0.5 + 0.3 * torch.rand(3, 24, generator=g),
              mixture_weights=torch.tensor([0.5, 0.3, 0.2])).to(dev)
    return [("checkerboard B=128 d=2, 2438 moves", cb, cb.loc.repeat_interleave(16, dim=0).contiguous(), 1e-3, 2438),
            ("3-component mixture B=4096 d=24, 256 moves", gmm, (2.0 * torch.randn(4096, 24, generator=g)).to(dev), 0.1, 256)]


def kernel_alone(dev, reps):
    print(f"# engine.rwmh_moves, Philox noise, adaptation on, no samples kept; ms per call, median (min, max) of {reps} after 2 warm-ups; us per move")
    for label, target, x0, step, K in kernel_cases(dev):
        lp0 = E.dist_eval(target, x0, want_score=False)[0].flatten().contiguous()
        out = []
        for rep in range(reps + 2):
            x, lp, st = x0.clone(), lp0.clone(), torch.full((x0.shape[0],), step, device=dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _, acc, _ = E.rwmh_moves(target, x, lp, st, K, target_acceptance=0.75, noise="philox", seed=rep, want_samples=False)
            b.record()
            b.synchronize()
            if rep >= 2:
                out.append(a.elapsed_time(b))
        med, lo, hi = median(out)
        print(f"{label:46s} {med:9.3f} ({lo:.3f}, {hi:.3f})   {1e3 * med / K:8.3f} us/move   mean acceptance {float(acc.mean()) / K:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if not a.kernel_only:
        data_set(dev, a.reps)
    kernel_alone(dev, a.reps)


if __name__ == "__main__":
    main()
