"""Every output bit of the tilted-potential entry points and of the chain-move kernels, written to a file by one build of the library and
compared by another (SDENG_LIB, tools/probe_lib.py): what a refactor of the kernels has to leave as it is.

    SDENG_LIB=/path/to/parent/libsdeng.so python tools/probe_tilted_bits.py --write bits.pt
    python tools/probe_tilted_bits.py --compare bits.pt            # exit status 1 on any difference

Inputs: the fixture cases a-f (tests/golden/tilted_*.npz) and the sixteen drawn cases of tests/tilted_cases.walk_spec (NT = 1 .. 8, a
diagonal and an eigen-form prior).  Outputs per case: tilted_eval (log-density and score, and the log-density-only form), tilted_vjp (energy,
score and the twelve row arrays), tilted_moves (5 MALA and 5 ULA moves with injected noise, 5 MALA moves with Philox: x, lp, grad, step,
samples, acc_sum, acc_last).  Then langevin_moves (MALA, ULA) and rwmh_moves on a 24-dimensional mixture target, 5 moves each.  Every input
is drawn on the CPU from a seeded generator.  Also printed per case: whether the state a move kernel carries is tilted_eval at that state."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_lib  # noqa: E402

LIB = probe_lib.select()
from sde_sampler_lrds_amd import engine as E  # noqa: E402
from sde_sampler_lrds_amd.additions import ebm_mle  # noqa: E402
from sde_sampler_lrds_amd.eq import sdes  # noqa: E402
from sde_sampler_lrds_amd.models import mlp, reparam  # noqa: E402
from tests import tilted_cases as tc  # noqa: E402

K_MOVES, STEP, TARGET = 5, 0.02, 0.75
MOVE_KEYS = ("x", "lp", "grad", "step", "samples", "acc_sum", "acc_last")


def tilted_case(name, net, t, x, dev, out):
    net, t, x = net.to(dev).requires_grad_(False), t.to(dev), x.to(dev).contiguous()
    M, d = x.shape
    lp, grad = E.tilted_eval(net, t, x)
    out[f"{name}/eval.lp"], out[f"{name}/eval.grad"] = lp, grad
    out[f"{name}/eval.lp_only"] = E.tilted_eval(net, t, x, want_grad=False)[0]
    v_lp, v_grad, arrays, _ = E.tilted_vjp(net, t, x, want_grad=True)
    out[f"{name}/vjp.lp"], out[f"{name}/vjp.grad"] = v_lp, v_grad
    for l in range(5):
        out[f"{name}/vjp.a{l}"], out[f"{name}/vjp.d{l}"] = arrays["a"][l], arrays["d"][l]
    out[f"{name}/vjp.xs"], out[f"{name}/vjp.dv"] = arrays["xs"], arrays["dv"]
    g = torch.Generator().manual_seed(9000 + M + d)
    z, u = torch.randn(K_MOVES, M, d, generator=g).to(dev), torch.rand(K_MOVES, M, generator=g).to(dev)
    carried = True
    for tag, kw in (("mala", dict(noise=(z, u))), ("ula", dict(noise=(z, u), unadjusted=True)), ("philox", dict(noise="philox", seed=0xB175 + d))):
        s = dict(x=x.clone(), lp=lp.clone(), grad=grad.clone(), step=torch.full((M,), STEP, device=dev))
        s["samples"], s["acc_sum"], s["acc_last"] = E.tilted_moves(net, t, s["x"], s["lp"], s["grad"], s["step"], K_MOVES, target_acceptance=TARGET, **kw)
        for k in MOVE_KEYS:
            if s[k] is not None:
                out[f"{name}/moves.{tag}.{k}"] = s[k]
        lp_e, grad_e = E.tilted_eval(net, t, s["x"])
        carried = carried and torch.equal(s["lp"], lp_e) and torch.equal(s["grad"], grad_e)
    print(f"{name}: M = {M}, d = {d}; carried state of the moves bit-equal to tilted_eval at it: {carried}")
    return carried


def chain_moves(dev, out):
    from sde_sampler_lrds_amd.distr.gauss import GMM, IsotropicGauss
    g = torch.Generator().manual_seed(4)
    B, d = 130, 24
    loc, scale = 2.0 * torch.randn(3, d, generator=g), 0.5 + 0.3 * torch.rand(3, d, generator=g)
    comp = torch.randint(3, (B,), generator=g)
    x0 = (loc[comp] + scale[comp] * torch.randn(B, d, generator=g)).to(dev)
    w = torch.rand(B, generator=g).to(dev)
    z, u = torch.randn(K_MOVES, B, d, generator=g).to(dev), torch.rand(K_MOVES, B, generator=g).to(dev)
    target = GMM(dim=d, loc=loc, scale=scale, mixture_weights=torch.tensor([0.5, 0.3, 0.2])).to(dev)
    prior = IsotropicGauss(dim=d, scale=2.5).to(dev)
    lp0, grad0 = ebm_mle.hip_tempered_log_prob_and_grads(target, prior)(w.reshape(-1, 1), x0)
    for tag, kw in (("mala", dict(noise=(z, u))), ("ula", dict(noise=(z, u), unadjusted=True)), ("philox", dict(noise="philox", seed=77))):
        x, lp, grad, st = x0.clone(), lp0.contiguous().clone(), grad0.contiguous().clone(), torch.full((B,), 0.05, device=dev)
        res = E.langevin_moves(target, prior, x, lp, grad, st, K_MOVES, t=w, target_acceptance=TARGET, **kw)
        for k, v in zip(MOVE_KEYS, (x, lp, grad, st) + tuple(res)):
            if v is not None:
                out[f"langevin/{tag}.{k}"] = v
    lp0 = E.dist_eval(target, x0, want_score=False)[0].flatten().contiguous()
    for tag, kw in (("injected", dict(noise=(z, u))), ("philox", dict(noise="philox", seed=78))):
        x, lp, st = x0.clone(), lp0.clone(), torch.full((B,), 0.3, device=dev)
        res = E.rwmh_moves(target, x, lp, st, K_MOVES, target_acceptance=TARGET, **kw)
        for k, v in zip(("x", "lp", "step", "samples", "acc_sum", "acc_last"), (x, lp, st) + tuple(res)):
            if v is not None:
                out[f"rwmh/{tag}.{k}"] = v


def main():
    ap = argparse.ArgumentParser()
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--write", metavar="FILE")
    mode.add_argument("--compare", metavar="FILE")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"# library {LIB}; device {torch.cuda.get_device_name(0)}")
    out, carried = {}, {}
    for case in tc.CASES:
        fx, net = tc.mirror(case)
        carried[case] = tilted_case(case, net, fx["t"], fx["x"], dev, out)
    for nt in range(1, 9):
        for prior in tc.WALK_PRIORS:
            spec = tc.walk_spec(nt, prior)
            net = tc.build(spec, mlp, reparam, sdes)
            t, x = tc.draw_inputs(spec, net)
            carried[f"nt{nt}_{prior}"] = tilted_case(f"nt{nt}_{prior}", net, t, x, dev, out)
    chain_moves(dev, out)
    torch.cuda.synchronize()
    out = {k: v.detach().cpu() for k, v in out.items()}
    finite = all(bool(torch.isfinite(v).all()) for v in out.values())
    print(f"# {len(out)} arrays, {sum(v.numel() for v in out.values())} values, all finite: {finite}; carried state bit-equal in "
          f"{sum(carried.values())} of {len(carried)} tilted cases" + ("" if all(carried.values()) else " (not: " + ", ".join(k for k, v in carried.items() if not v) + ")"))
    if a.write:
        torch.save(out, a.write)
        print(f"# written to {a.write}")
        return 0
    ref = torch.load(a.compare)
    differ = [k for k in sorted(set(out) | set(ref)) if k not in out or k not in ref or not torch.equal(out[k], ref[k])]
    for k in differ:
        if k in out and k in ref and out[k].shape == ref[k].shape:
            print(f"DIFFERS {k}: {int((out[k] != ref[k]).sum())} of {out[k].numel()} values, max |difference| {float((out[k] - ref[k]).abs().max()):.3e}")
        else:
            print(f"DIFFERS {k}: missing on one side, or another shape")
    print(f"# compared with {a.compare}: {len(out) - len(differ)} of {len(out)} arrays torch.equal" + ("" if differ else " -- every output bit is the same"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
