"""Sharded training on the GPU: ``world`` fresh worker processes (tests/sharded_training_worker.py under ``python -m
torch.distributed.run``, gloo backend, all on the one device) each run their shard of a golden training case -- ``loss.particle0`` at the
shard's first row, ``loss.dist`` set -- then ``backward()`` and ``parallel.all_reduce_grads``.  A training step on N ranks must equal the
single-process step on the concatenated batch, hence the reference-generated ``train_lv_*`` / ``train_kl_*`` fixtures, to the bounds
tests/test_gpu_training.py holds the single-process run to (loss 1e-5 relative; gradients 5e-5 of the largest entry, or 10 x the
fixture's ``grad_sensitivity`` for KL).  World 2 gives whole 16-particle tiles; world 3 gives shards of 22/21/21 (11/11/10 at B = 32):
partial tiles and a ``particle0`` that is no multiple of 16.  One launch per world size serves all cases; nothing is retried.

The solver-level test trains a small ``make_model`` RDS for three ``step()``s on two ranks through ``TrainableDiff.set_distributed``
and compares with the same three steps in this process.  Its bound is summation-order round-off through three Adam steps: the
single-process run against itself under permuted batch orders spreads by at most 7.356e-7 of a tensor's largest entry (measured on MI355X,
profiles/sharded_training.log), and 10 x that is allowed."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import golden_cases as gc
from tests import sharded_training_worker as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREAD = 7.356e-7  # worst relative difference, single-process run vs itself under a permuted batch order (profiles/sharded_training.log)
_RUNS = {}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def sharded(world, tmp_path_factory):
    """What rank 0 of a ``world``-rank run wrote (one launch per world size, shared by the tests; a failed launch fails them all)."""
    if world not in _RUNS:
        out = str(tmp_path_factory.mktemp(f"sharded{world}") / "out.npz")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "sharded_training_worker.py"), "--out", out]
        if world == 2:
            cmd.append("--solver")
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
            _RUNS[world] = dict(np.load(out)) if r.returncode == 0 else AssertionError(f"exit {r.returncode}\n{r.stderr[-3000:]}")
        except subprocess.TimeoutExpired as e:
            _RUNS[world] = AssertionError(f"timed out\n{(e.stderr or b'')[-3000:]}")
    if isinstance(_RUNS[world], Exception):
        raise _RUNS[world]
    return _RUNS[world]


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", W.CASES)
def test_sharded_training_step_matches_the_reference_fixture(gpu, tmp_path_factory, name, world):
    got = sharded(world, tmp_path_factory)
    c = gc.load(name)
    B = c["x0"].shape[0]
    values = got[f"{name}/values"]
    assert len(values) == world and all(v == values[0] for v in values), f"the value differs between ranks: {values}"
    assert all(f == got[f"{name}/n_filtered"][0] for f in got[f"{name}/n_filtered"])
    assert int(got[f"{name}/collectives"]) <= 2
    loss_err = abs(values[0] - c.meta["loss"]) / max(1.0, abs(c.meta["loss"]))
    worst, n = 0.0, 0
    for k in c.a:
        if not k.startswith("grad."):
            continue
        ref = c[k]
        grad = got.get(f"{name}/{k}")
        assert grad is not None, k
        worst, n = max(worst, float((torch.from_numpy(grad) - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)), n + 1
    tol = max(5e-5, 10 * c.meta.get("grad_sensitivity", 0.0)) if name in W.KL_CASES else 5e-5
    print(f"{name} on {world} ranks (B = {B}, rank 0 rows {got[f'{name}/shard'].tolist()}): loss {values[0]:.6f} vs {c.meta['loss']:.6f} (rel {loss_err:.1e}); "
          f"worst relative gradient error {worst:.2e} over {n} parameters (tolerance {tol:.1e}); {int(got[f'{name}/collectives'])} collectives")
    assert n >= 8 and loss_err < 1e-5 and worst < tol


@pytest.mark.gpu
def test_sharded_solver_steps_equal_the_single_process_run(gpu, tmp_path_factory):
    got = sharded(2, tmp_path_factory)
    keys = [k[len("solver/rank0/"):] for k in got if k.startswith("solver/rank0/") and not k.endswith("eval")]
    assert len(keys) >= 16
    for k in keys:  # every parameter and the EMA copy: the same bits on both ranks
        assert np.array_equal(got[f"solver/rank0/{k}"], got[f"solver/rank1/{k}"]), k
    assert np.array_equal(got["solver/rank0/eval"], got["solver/rank1/eval"])
    model, losses = W.run_solver(3)
    single = {}
    with torch.no_grad():
        W.solver_state(model, "", single)
    worst, where = 0.0, None
    for k in keys:
        e = float(np.abs(got[f"solver/rank0/{k}"] - single[k]).max()) / max(float(np.abs(single[k]).max()), 1e-12)
        if e > worst:
            worst, where = e, k
    loss_err = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(got["solver/losses"], losses))
    ev, ref = got["solver/rank0/eval"], single["eval"]
    print(f"3 steps on 2 ranks vs single process: worst relative parameter / EMA difference {worst:.2e} (at {where}; bound {10 * SPREAD:.1e} = 10 x the "
          f"single-process spread under a permuted batch order), losses within {loss_err:.1e}; evaluate(): log Z {ev[0]:.6f} vs {ref[0]:.6f}, "
          f"ELBO {ev[1]:.6f} vs {ref[1]:.6f}, ESS {ev[2]:.6f} vs {ref[2]:.6f}, n {int(ev[3])} (shard of {int(got['solver/local_samples'])})")
    assert worst < 10 * SPREAD
    # tolerances of tests/test_parallel_cpu.py
    assert abs(ev[0] - ref[0]) < 1e-5 and abs(ev[1] - ref[1]) < 1e-5 and abs(ev[2] - ref[2]) < 1e-6
    assert int(ev[3]) == model.eval_batch_size and int(got["solver/local_samples"]) == model.eval_batch_size // 2
