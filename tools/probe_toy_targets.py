"""Step-loop timing of the 2-D toy targets next to the d = 16 CMCD mixture kernel: CMCD on Rings and Checkerboard, PIS on Checkerboard,
CMCD on cmcd_gmm_iso_d16's mixture, all at B particles x N steps with in-kernel Philox noise (the ClippedCtrl / ScoreCtrl nets of the
fixtures).  Median of 10 timed passes after 3 warm-ups, CUDA events around the whole simulate() call.

    python tools/probe_toy_targets.py [--B 65536] [--N 256]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tests import build_cases as bc  # noqa: E402
from tests import golden_cases as gc  # noqa: E402
from tests import test_gpu_toy_targets as tt  # noqa: E402
from sde_sampler_lrds_amd.distr.checkerboard import Checkerboard  # noqa: E402
from sde_sampler_lrds_amd.eq.sdes import ScaledBM  # noqa: E402
from sde_sampler_lrds_amd.distr.gauss import Gauss  # noqa: E402
from sde_sampler_lrds_amd.losses import oc  # noqa: E402


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--N", type=int, default=256)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N = a.B, a.N
    ts = torch.linspace(0.0, 1.0, N + 1, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for name in ("toy_cmcd_rings", "toy_cmcd_checkerboard"):
        c = gc.load(name)
        loss, target, prior = tt._cmcd(c, dev)
        x0 = prior.sample((B,)).to(dev)
        res = {}

        def run():
            res["x"], res["rnd"], _ = loss.simulate(ts, x0, target.unnorm_log_prob, initial_log_prob=prior.log_prob, train=False)
        rows.append((f"CMCD {c.meta['target']} d=2 ({'ScoreCtrl' if c.meta['target'] == 'rings' else 'ClippedCtrl, GaussFull prior'})",
                     timed(run), int(torch.isinf(res["rnd"]).sum())))
    c = gc.load("toy_pis_checkerboard")
    target = Checkerboard().to(dev)
    ctrl = tt._ctrl(c, target).to(dev)
    sde = ScaledBM(diff_coeff=c.meta["diff_coeff"], terminal_t=c.meta["T"]).to(dev)
    refd = Gauss(dim=2, loc=c["ref_loc"], scale=c["ref_scale"]).to(dev)
    loss = oc.EMReferenceSDELoss(ctrl, ctrl, sde=sde, method="kl")
    tsp = torch.linspace(0.0, c.meta["T"], N + 1, device=dev)
    x0 = torch.zeros(B, 2, device=dev)
    res = {}

    def run_pis():
        res["x"], res["rnd"], _ = loss.simulate(tsp, x0, target.unnorm_log_prob, refd.log_prob)
    rows.append(("PIS checkerboard d=2 (ClippedCtrl)", timed(run_pis), int(torch.isinf(res["rnd"]).sum())))
    c = gc.load("cmcd_gmm_iso_d16")
    b = bc.build(c, dev)
    x0 = c.meta["prior_scale"] * torch.randn(B, c.meta["d"], device=dev, generator=g)

    def run_gmm():
        res["x"], res["rnd"], _ = b["loss"].simulate(ts, x0, *b["args"], **b["kwargs"])
    rows.append(("CMCD cmcd_gmm_iso_d16 mixture d=16 (ScoreCtrl)", timed(run_gmm), int(torch.isinf(res["rnd"]).sum())))
    print(f"# B = {B}, N = {N}; ms per simulate() call: median (min, max) of 10; particles at rnd = +inf")
    for label, (med, lo, hi), n_inf in rows:
        print(f"{label:52s} {med:8.3f} ({lo:.3f}, {hi:.3f})  inf {n_inf}")


if __name__ == "__main__":
    main()
