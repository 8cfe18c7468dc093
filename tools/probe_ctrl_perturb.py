"""What do sde_ctrl_noise / sde_ctrl_dropout cost a log-variance training step?  RDS-EI on ManyModes d=128 with a 4-component reference,
512 particles x 100 steps (make_model, split-tile step loop): the options off, noise, noise + dropout -- interleaved rounds on one box,
the whole training step and the step-loop launch alone (simulate with the trajectory, as the training call runs it)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sde_sampler_lrds_amd.experiments.benchmark_utils import make_model, make_target_details  # noqa: E402

d, B, N, ROUNDS, STEPS = 128, 512, 100, 5, 20
MODES = {"off": (None, None), "noise 0.1": (0.1, None), "noise 0.1 + dropout 0.9": (0.1, 0.9)}
tgt = make_target_details("many_modes", dim=d, n_modes=4)
g = torch.Generator().manual_seed(0)
model = make_model("vp-ref", "gmm", "lv", "ei", "base_zero_init", "uniform",
                   dict(means_ref=4 * torch.rand(4, d, generator=g) - 2, variances_ref=0.5 * torch.ones(4, d), weights_ref=torch.ones(4)),
                   tgt, dict(train_steps=10, train_batch_size=B, eval_batch_size=B), optim_details=dict(lr=1e-3), n_steps=N)
model.setup_optim()
loss = model.loss
print(f"RDS-EI ManyModes d={d}, {B} x {N}, split_tiles={loss.split_tiles}", flush=True)


def set_mode(mode):
    loss.sde_ctrl_noise, loss.sde_ctrl_dropout = MODES[mode]


def time_steps(mode):
    set_mode(mode)
    for i in range(3):
        model.step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(STEPS):
        model.step(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / STEPS


def time_loop(mode):
    """The step-loop launch of a training call alone (BaseOCLoss._lv_loss hands the table options to its launch)."""
    set_mode(mode)
    x = model.prior.sample((B,)).to(model.device)

    def launch():
        with torch.no_grad():
            loss._launch(loss._step_loop(train=True), model.train_ts, x, terminal_unnorm_log_prob=model.clipped_target_unnorm_log_prob,
                         reference_log_prob=model.reference_distr.log_prob, return_traj=True, perturb=loss._ctrl_perturbation())
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        launch()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / STEPS


res = {m: ([], []) for m in MODES}
for r in range(ROUNDS):
    for m in MODES:
        res[m][0].append(time_steps(m))
        res[m][1].append(time_loop(m))
    print(f"round {r}: " + "  ".join(f"{m}: step {res[m][0][-1] * 1e3:.2f} ms, loop {res[m][1][-1] * 1e3:.3f} ms" for m in MODES), flush=True)
med = {m: (sorted(v[0])[ROUNDS // 2], sorted(v[1])[ROUNDS // 2]) for m, v in res.items()}
for m in MODES:
    print(f"median of {ROUNDS} rounds, {m:24s}: training step {med[m][0] * 1e3:.2f} ms ({med[m][0] / med['off'][0]:.3f} x off), "
          f"step loop {med[m][1] * 1e3:.3f} ms ({med[m][1] / med['off'][1]:.3f} x off)", flush=True)
