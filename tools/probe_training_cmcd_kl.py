"""KL training of CMCD: wall time of one full training step (compute_loss + backward, synchronised; warm; median of 20) with the one-launch
adjoint (loss.native_adjoint = True, sdeng_cmcd_kl_adjoint) and with the per-step adjoint it replaces (False: one torch vector-Jacobian
product per SDE step, replayed as a hipGraph where capture is possible), same process, same model.  Workloads: a mixture at d = 16,
2048 x 100; logistic regression at d = 61 (the shape of BASELINE config 4; a synthetic design matrix of sonar's shape), 2048 x 100; a mixture at
d = 128, 512 x 100."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sde_sampler_lrds_amd.distr.logistic_regression import register_dataset  # noqa: E402
from sde_sampler_lrds_amd.experiments.benchmark_utils import make_model, make_target_details  # noqa: E402


def step_ms(model, native, warm=3, n=20):
    model.loss.native_adjoint = native
    times = []
    for i in range(warm + n):
        for p in model.generative_ctrl.parameters():
            p.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss, _ = model.compute_loss()
        loss.backward()
        torch.cuda.synchronize()
        if i >= warm:
            times.append((time.perf_counter() - t0) * 1e3)
    assert model.loss.last_adjoint_path == ("native" if native else "stepwise")
    return statistics.median(times), min(times), max(times)


def bench(label, details, B, N):
    torch.manual_seed(0)
    model = make_model("cmcd", "default", "kl", "em", "target_informed_zero_init", "uniform", {}, details,
                       dict(train_steps=10, train_batch_size=B, eval_batch_size=B), optim_details=dict(lr=1e-3), n_steps=N)
    with torch.no_grad():  # a drift net that does something (make_model zero-initialises the last layer)
        w = model.generative_ctrl.base_model.out_layer.weight
        w.copy_(0.05 * torch.randn(w.shape, generator=torch.Generator().manual_seed(1)))
    model.setup_optim()
    nat, step = step_ms(model, True), step_ms(model, False)
    print(f"{label}, {B} x {N}: native {nat[0]:.2f} ms (min {nat[1]:.2f}, max {nat[2]:.2f}); stepwise {step[0]:.2f} ms (min {step[1]:.2f}, max {step[2]:.2f}); "
          f"ratio {step[0] / nat[0]:.1f}x", flush=True)


if __name__ == "__main__":
    g = torch.Generator().manual_seed(7)
    register_dataset("sonar", (1e-4 + (1 - 1e-4) * torch.rand(166, 60, generator=g) ** 2).float(), (torch.rand(166, generator=g) < 0.47).float())
    print(f"device: {torch.cuda.get_device_name(0)}; medians of 20 synchronised steps after 3 warm-up steps", flush=True)
    bench("CMCD, ManyModes d=16", make_target_details("many_modes", dim=16, n_modes=4), 2048, 100)
    bench("CMCD, logistic regression d=61", make_target_details("sonar"), 2048, 100)
    bench("CMCD, ManyModes d=128", make_target_details("many_modes", dim=128, n_modes=4), 512, 100)
