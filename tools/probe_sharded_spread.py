"""Spread of the single-process 3-step training run of tests/sharded_training_worker.solver_model against itself under a permuted batch
order: the rows handed to the batched control pass (forward + backward) and to compute_loss are permuted -- the same particles, the same
mathematics, another summation order.  Prints the worst relative difference (of a tensor's largest entry) over all parameters and the
EMA copy; 10 x that is the bound tests/test_gpu_sharded_training.py allows between a sharded and a single-process run
(profiles/sharded_training.log)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.sharded_training_worker import solver_model  # noqa: E402


def run(perm=None, steps=3):
    model = solver_model()
    loss = model.loss
    if perm is not None:
        perm = perm.to(model.device)
        inv = torch.argsort(perm)
        orig_ip, orig_cl = loss._integral_pass, loss.compute_loss

        def ip(t, xs, zc):
            N, B, d = xs.shape
            s = orig_ip(t, xs[:, perm].contiguous(), zc.view(N, B, d)[:, perm].reshape(N * B, d).contiguous())
            return s[inv]

        def cl(rnd, samples=None):
            return orig_cl(rnd[perm], samples=None if samples is None else samples[perm])
        loss._integral_pass, loss.compute_loss = ip, cl
    model.setup_optim()
    losses = [model.step(i)["train/loss"] for i in range(steps)]
    state = {"param." + k: p.detach().clone() for k, p in model.generative_ctrl.named_parameters()}
    state.update({"ema." + k: p.detach().clone() for k, p in model.generative_ctrl_ema.module.named_parameters()})
    return losses, state


def spread(a, b):
    worst, where = 0.0, None
    for k in a:
        e = float((a[k] - b[k]).abs().max()) / max(float(b[k].abs().max()), 1e-12)
        if e > worst:
            worst, where = e, k
    return worst, where


def main():
    base_l, base = run()
    again_l, again = run()
    print(f"rerun, same order: spread {spread(again, base)[0]:.3e}; losses {base_l} vs {again_l}")
    g = torch.Generator().manual_seed(0)
    B = 64
    perms = {"random": torch.randperm(B, generator=g), "halves swapped": torch.cat([torch.arange(B // 2, B), torch.arange(B // 2)]),
             "reversed": torch.arange(B - 1, -1, -1), "random 2": torch.randperm(B, generator=g)}
    worst = 0.0
    for name, perm in perms.items():
        losses, st = run(perm)
        s, where = spread(st, base)
        worst = max(worst, s)
        print(f"permutation '{name}': spread {s:.3e} (at {where}); loss differences {[abs(x - y) / max(1.0, abs(y)) for x, y in zip(losses, base_l)]}")
    print(f"worst spread over the permutations: {worst:.3e}; bound = 10 x = {10 * worst:.3e}")


if __name__ == "__main__":
    main()
