"""One rank of a sharded training run on the GPU (tests/test_gpu_sharded_training.py starts ``world`` of these under
``python -m torch.distributed.run``, gloo backend, all on the one device), and the collective counter the CPU and GPU tests share.

Every rank builds the golden training cases through tests/build_cases.py exactly as tests/test_gpu_training.py does, keeps rows
``parallel.shard_bounds(B, world, rank)`` of the fixture's x0, sets ``loss.particle0`` / ``loss.dist``, then calls ``loss(...)``,
``backward()`` and ``parallel.all_reduce_grads``.  Rank 0 writes values, gradients and collective counts to one ``.npz``.  With ``--solver``
it also trains and evaluates a small ``make_model`` RDS for three steps through ``TrainableDiff.set_distributed``."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COLLECTIVES = ("all_reduce", "all_gather", "all_gather_into_tensor", "all_gather_object", "all_to_all", "all_to_all_single", "broadcast",
               "broadcast_object_list", "reduce", "reduce_scatter", "reduce_scatter_tensor", "gather", "scatter", "barrier", "send", "recv")

LV_CASES = ["train_lv_ei_gmm_d16", "train_lv_cmcd_gmm_d16", "train_lv_pis_phi4_d100"]
KL_CASES = ["train_kl_ei_gmm_d16", "train_kl_cmcd_gmm_d16"]
CASES = LV_CASES + KL_CASES


class CountingDist:
    """``torch.distributed`` as the product sees it (a module-like object), counting every collective issued through it."""

    def __init__(self, dist):
        self._dist, self.calls = dist, []

    def __getattr__(self, name):
        attr = getattr(self._dist, name)
        if name not in COLLECTIVES:
            return attr

        def counted(*a, **k):
            self.calls.append(name)
            return attr(*a, **k)
        return counted


def solver_model(device="cuda"):
    """The small RDS of the solver-level test: EI, log-variance, d = 2 mixture, 64 training particles, eight optimiser steps configured on a
    16-step grid, the standard step-loop kernel on both sides (``split_tiles`` off), an EMA copy updated every step, and a drift net
    that does something (make_model zero-initialises the last layer)."""
    import torch

    from sde_sampler_lrds_amd.experiments.benchmark_utils import make_model, make_target_details
    tgt = make_target_details("many_modes", dim=2, n_modes=4)
    model = make_model("vp-ref", "default", "lv", "ei", "base_zero_init", "uniform", dict(sigma=2.0), tgt,
                       dict(train_steps=8, train_batch_size=64, eval_batch_size=200), optim_details=dict(lr=1e-3), n_steps=16, use_ema=True,
                       device=device)
    model.loss.split_tiles = False
    model.ema_steps = 1
    with torch.no_grad():
        g = torch.Generator(device="cpu").manual_seed(1)
        w = model.generative_ctrl.base_model.out_layer.weight
        w.copy_(0.05 * torch.randn(w.shape, generator=g))
    return model


def solver_state(model, prefix, out):
    """Parameters, EMA copy and evaluation estimators of ``model`` into ``out`` (numpy arrays keyed ``prefix + name``)."""
    for k, p in model.generative_ctrl.named_parameters():
        out[f"{prefix}param.{k}"] = p.detach().cpu().numpy()
    for k, p in model.generative_ctrl_ema.module.named_parameters():
        out[f"{prefix}ema.{k}"] = p.detach().cpu().numpy()
    res = model.evaluate(use_ema=True)
    import numpy as np
    out[f"{prefix}eval"] = np.array([res.log_norm_const_preds["log_norm_const_is"], res.metrics["eval/elbo"],
                                     res.metrics["eval/norm_effective_sample_size"],
                                     res.metrics.get("eval/n_particles", res.samples.shape[0])], dtype=np.float64)
    return res


def run_solver(steps=3, dist=None):
    """``steps`` optimiser steps of ``solver_model`` (sharded over ``dist`` when given) -> (model, losses of the steps)."""
    model = solver_model()
    if dist is not None:
        model.set_distributed(dist)
    model.setup_optim()
    return model, [model.step(i)["train/loss"] for i in range(steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", nargs="*", default=CASES)
    ap.add_argument("--solver", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo")  # (rank, world size and the rendezvous come from the launcher's environment)
    rank, world = dist.get_rank(), dist.get_world_size()
    gpu = torch.device("cuda:0")

    from sde_sampler_lrds_amd import parallel
    from tests import build_cases as bc
    from tests import golden_cases as gc
    from tests.test_gpu_training import KINDS

    out = {}
    for name in args.cases:
        c = gc.load(name)
        c.meta["kind"] = KINDS[c.meta["kind"]]
        b = bc.build(c, gpu)
        loss = b["loss"]
        if name in KL_CASES:
            loss.method, loss.max_rnd = "kl", None
        else:
            loss.method = "lv"
        ctrl = loss.generative_ctrl
        for p in ctrl.parameters():
            p.grad = None
        lo, hi = parallel.shard_bounds(b["x0"].shape[0], world, rank)
        counting = CountingDist(dist)
        loss.particle0, loss.dist = lo, counting
        kw = {k: v for k, v in b["kwargs"].items() if k == "initial_log_prob"}
        value, _ = loss(b["ts"], b["x0"][lo:hi].clone(), *b["args"], **kw)
        value.backward()
        parallel.all_reduce_grads([p for p in ctrl.parameters() if p.requires_grad], counting)
        values = [None] * world
        dist.all_gather_object(values, float(value.detach()))
        filtered = [None] * world
        dist.all_gather_object(filtered, int(loss.n_filtered))
        if rank == 0:
            out[f"{name}/values"] = np.array(values, dtype=np.float64)
            out[f"{name}/n_filtered"] = np.array(filtered)
            out[f"{name}/collectives"] = np.array(len(counting.calls))
            out[f"{name}/shard"] = np.array([lo, hi])
            for k, p in ctrl.named_parameters():
                if p.grad is not None:
                    out[f"{name}/grad.{k}"] = p.grad.detach().cpu().numpy()

    if args.solver:
        model, losses = run_solver(3, dist)
        mine = {}
        res = solver_state(model, "", mine)
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        if rank == 0:
            out["solver/losses"] = np.array(losses, dtype=np.float64)
            out["solver/local_samples"] = np.array(res.samples.shape[0])
            for r, state in enumerate(gathered):
                for k, v in state.items():
                    out[f"solver/rank{r}/{k}"] = v

    if rank == 0:
        np.savez(args.out, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
