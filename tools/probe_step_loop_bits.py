"""What the loss classes compute on the GPU, written to a file by one tree's Python package and compared by another's over the same
libsdeng.so: what a refactor of the host side of the step loops (losses/oc.py, losses/training.py, engine.py) has to leave as it is.

    python tools/probe_step_loop_bits.py --package /path/to/parent/checkout --write bits.pt
    python tools/probe_step_loop_bits.py --compare bits.pt            # exit status 1 on any difference

``--package``: the directory that holds the ``sde_sampler_lrds_amd`` to import (default: this checkout); the fixtures and their builders
(tests/) are this checkout's either way.  Per case, at the fixture's own small size: x_N and rnd of ``simulate`` and the samples, weights and
estimators of ``eval``; rnd of ``compute_eubo``; the loss value and every parameter gradient of two consecutive log-variance training
calls and of two consecutive KL training calls under each (native_adjoint, fused_training) setting.  A refusal is recorded as such."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = ["rds_ei_gmm_d8_k4", "rds_em_remove_ref_d16", "dds_two_modes_d2", "dis_orig_lerp_d8", "dis_ei_cancel_drift_d8", "pis_em_phi4_d100",
       "cmcd_gmm_iso_d16", "cmcd_logreg_d61"]
EUBO = ["eubo_ei_gmm_d16_k4", "eubo_cmcd_gmm_d16"]


def train(out, key, b, E):
    """Two consecutive training calls + backward(): value and gradients, or the refusal."""
    loss = b["loss"]
    loss.train_calls, ctrl = 0, b["loss"].generative_ctrl
    kw = {k: v for k, v in b.get("kwargs", {}).items() if k == "initial_log_prob"}
    for call in range(2):
        for p in ctrl.parameters():
            p.grad = None
        try:
            value, _ = loss(b["ts"], b["x0"], *b["args"], **kw)
        except E.UnsupportedByEngine:
            out[f"{key}.{call}.refused"] = torch.zeros(1)
            return
        value.backward()
        out[f"{key}.{call}.value"] = value.detach().reshape(1)
        if getattr(loss, "last_adjoint_path", None) and "kl" in key:
            out[f"{key}.{call}.path"] = torch.tensor([ord(c) for c in loss.last_adjoint_path], dtype=torch.int32)
        for name, p in ctrl.named_parameters():
            if p.grad is not None:
                out[f"{key}.{call}.grad.{name}"] = p.grad.clone()


def train_all(out, name, b, E, kl=True):
    loss = b["loss"]
    loss.graph_adjoint, loss.method = False, "lv"
    train(out, f"{name}/lv", b, E)
    for native in (False, True) if kl else ():
        for fused in (False, True):
            loss.method, loss.native_adjoint, loss.fused_training = "kl", native, fused
            train(out, f"{name}/kl.native{int(native)}.fused{int(fused)}", b, E)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=ROOT)
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--write", metavar="FILE")
    mode.add_argument("--compare", metavar="FILE")
    a = ap.parse_args()
    sys.path[:0] = [os.path.abspath(a.package)] + ([ROOT] if os.path.abspath(a.package) != ROOT else [])
    import sde_sampler_lrds_amd
    from sde_sampler_lrds_amd import engine as E
    from sde_sampler_lrds_amd.experiments import benchmark_utils as bu
    from tests import build_cases as bc
    from tests import golden_cases as gc
    from tests import tilted_cases as tc
    dev = torch.device("cuda:0")
    print(f"# package {os.path.relpath(os.path.dirname(sde_sampler_lrds_amd.__file__), ROOT)}; device {torch.cuda.get_device_name(0)}")
    out = {}
    for name in SIM:
        b = bc.build(gc.load(name), dev)
        kw = {k: v for k, v in b["kwargs"].items() if k == "initial_log_prob"}
        out[f"{name}/simulate.x"], out[f"{name}/simulate.rnd"], _ = b["loss"].simulate(b["ts"], b["x0"], *b["args"], **b["kwargs"])
        res = b["loss"].eval(b["ts"], b["x0"], *b["args"], **kw)
        out[f"{name}/eval.samples"], out[f"{name}/eval.weights"], out[f"{name}/eval.xs"] = res.samples, res.weights, res.xs
        out[f"{name}/eval.logz"] = torch.tensor([float(res.log_norm_const_preds["log_norm_const_is"]), float(res.metrics["eval/elbo"])], dtype=torch.float64)
        train_all(out, name, b, E)
    for name in EUBO:
        b = bc.build(gc.load(name), dev)
        kw = {k: v for k, v in b["kwargs"].items() if k == "initial_log_prob"}
        x = b["x0"].clone()
        out[f"{name}/eubo.rnd"], out[f"{name}/eubo.x"] = b["loss"].compute_eubo(b["ts"], x, *b["args"], **kw), x
    net = tc.mirror("b")[1]  # RDS over an energy-based reference (tests/test_gpu_tilted_rds.py make())
    model = bu.make_model("vp-ref", "nn", "lv", "ei", "base_zero_init", "uniform", dict(net=net, sigma=1.0), bu.make_target_details("many_modes", dim=net.dim, n_modes=3),
                          dict(train_steps=10, train_batch_size=64, eval_batch_size=96), n_steps=8, compute_samples_based_metrics=False, device=dev)
    torch.manual_seed(4)
    for p in model.generative_ctrl.parameters():  # (zero-initialised last layer: give the control something to do)
        p.data.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(dev))
    b = dict(loss=model.loss, ts=model.train_timesteps(device=dev), x0=torch.randn(64, net.dim, generator=torch.Generator().manual_seed(3)).to(dev),
             args=(model.clipped_target_unnorm_log_prob, model.reference_distr.log_prob))
    res = model.loss.eval(b["ts"], b["x0"], *b["args"])
    out["rds_nn_b/eval.samples"], out["rds_nn_b/eval.weights"] = res.samples, res.weights
    train_all(out, "rds_nn_b", b, E, kl=False)
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().contiguous() for k, v in out.items()}
    finite = [k for k, v in out.items() if v.is_floating_point() and not bool(torch.isfinite(v).all())]
    out = {k: v.view(torch.int32) if v.dtype == torch.float32 else v for k, v in out.items()}  # bits: a NaN equals the same NaN
    refused = sorted(k for k in out if k.endswith(".refused"))
    print(f"# {len(out)} arrays, {sum(v.numel() for v in out.values())} values; not finite: {', '.join(finite) or 'none'}; refused: {', '.join(refused) or 'none'}")
    if a.write:
        torch.save(out, a.write)
        print(f"# written to {a.write}")
        return 0
    ref = torch.load(a.compare)
    differ = [k for k in sorted(set(out) | set(ref)) if k not in out or k not in ref or out[k].shape != ref[k].shape or not torch.equal(out[k], ref[k])]
    for k in differ:
        print(f"DIFFERS {k}" + (f": {int((out[k] != ref[k]).sum())} of {out[k].numel()} values" if k in out and k in ref and out[k].shape == ref[k].shape else ": missing on one side, or another shape"))
    print(f"# compared with {a.compare}: {len(out) - len(differ)} of {len(out)} arrays torch.equal" + ("" if differ else " -- every value, gradient and output bit is the same"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
