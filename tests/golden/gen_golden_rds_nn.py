"""Fixtures of RDS over an energy-based ('nn') reference, tests/golden/rds_nn_*.npz and train_lv_rds_nn_b.npz: the REAL reference's
EIReferenceSDELoss / DDPMLikeReferenceSDELoss / EMReferenceSDELoss.simulate (losses/oc.py:218-296, :444-510, :584-651) on the CPU, with
``reference_ctrl`` the score of the reference's own tilted potential (solver/oc.py:577-585) and the terminal reference cost
``WrapperDistrNN(net, eps=ts[0]).log_prob`` (distr/base.py:186-198) -- run in float32 and in float64 built from the same float32 numbers
(``gen_golden.py`` sets up the reference's import path).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_rds_nn.py [case ...]

The energy net is NOT stored again: it is ``tilted_cases.Fixture(case).build(...)`` of the stored tilted fixtures.  The cases, their
grids and the way x0 is drawn are in ``tests/rds_nn_cases.py``.  A fixture stores ``ts``, ``x0``, the control's state_dict (``ctrl.<key>``),
the target mixture, ``x_N`` / ``rnd`` / the trajectory in both precisions (``out.x32`` ...) and, in the meta, the reference's own float32
error against its float64 run in the metric ``tilted_cases.err``.  The generator REFUSES a case whose float32 run is not within 1e-3 of
the float64 run or whose |x_N| exceeds 100: a bound of MARGIN x err32 means something only for a well-conditioned trajectory.
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (sets up the reference's import path and its stand-in modules)
import torch  # noqa: E402

from tests import rds_nn_cases as rc  # noqa: E402
from tests import tilted_cases as tc  # noqa: E402

class Replay(gg.Replay):
    """gen_golden.Replay in the precision of the run: the same float32 normals, cast like the state (a float32 tensor times the 0-dim
    float64 gain of the reference's step would be rounded to float32, and the float64 run with it)."""

    def __call__(self, x, *a, **kw):
        return super().__call__(x, *a, **kw).to(x.dtype)


def run_with_replay(seed, fn):
    orig, rep = torch.randn_like, Replay(seed)
    torch.randn_like = rep
    try:
        with torch.no_grad():
            out = fn()
    finally:
        torch.randn_like = orig
    return out, rep.k


LOSSES = {"ei": gg.r_oc.EIReferenceSDELoss, "ddpm_like": gg.r_oc.DDPMLikeReferenceSDELoss, "em": gg.r_oc.EMReferenceSDELoss}


def pieces(name, dtype):
    """(loss, ctrl, ts, x0, target, reference distribution) of one case in ``dtype``; the float32 numbers are drawn once (dtype float32)
    and cast."""
    spec = rc.CASES[name]
    fx = tc.Fixture(spec["tilted"])
    net = fx.build(gg.r_mlp, gg.r_rep, gg.r_sdes, dtype)
    for p in net.parameters():  # solver/oc.py:579-580
        p.requires_grad_(False)
    torch.manual_seed(spec["seed"])
    ctrl = gg.r_rep.ClippedCtrl(base_model=gg.liven(gg.fourier_mlp(fx.spec["d"])), clip_model=1e4).to(dtype)
    target = gg.r_gauss.ManyModes(n_modes=3, dim=fx.spec["d"], var=0.5, seed_loc=42, mixture_weight_factor=3.0, n_reference_samples=10)
    if dtype != torch.float32:  # the same mixture from its float32 parameters cast (Distribution.to returns nothing upstream)
        target = gg.r_gauss.GMM(dim=fx.spec["d"], loc=target.loc.to(dtype), scale=target.scale.to(dtype), mixture_weights=target.mixture_weights.to(dtype),
                                n_reference_samples=10)
    ts = rc.grid(spec).to(dtype)
    net32 = net if dtype == torch.float32 else fx.build(gg.r_mlp, gg.r_rep, gg.r_sdes, torch.float32)
    x0 = rc.draw_x0(spec, net32, gg.orc.philox_normal).to(dtype)
    reference_ctrl = lambda t, x: net(t=t.view((1, 1)).expand((x.shape[0], -1)), x=x)  # noqa: E731  (solver/oc.py:585)
    loss = LOSSES[spec["integrator"]](ctrl, ctrl, sde=net.sde, method="lv", reference_ctrl=reference_ctrl)
    # (eps as a (1, 1) tensor: ``t * torch.ones((B, 1))`` of distr/base.py:197 then keeps the precision of the run; a 0-dim float64 eps
    # times the float32 ones would hand the net a float32 time column)
    ref_distr = gg.r_base.WrapperDistrNN(dim=fx.spec["d"], net=net, t=ts[0].reshape(1, 1))
    return loss, ctrl, ts, x0, target, ref_distr


def simulate(name, dtype):
    loss, ctrl, ts, x0, target, ref_distr = pieces(name, dtype)
    (x, rnd, xs), draws = run_with_replay(rc.CASES[name]["seed"], lambda: loss.simulate(
        ts, x0.clone(), terminal_unnorm_log_prob=target.unnorm_log_prob, reference_log_prob=ref_distr.log_prob, return_traj=True))
    assert draws == ts.numel() - 1
    return dict(x=x.detach(), rnd=rnd.detach().reshape(-1), xs=xs.detach()), ctrl, ts, x0, target


def make(name):
    spec = rc.CASES[name]
    o32, ctrl, ts, x0, target = simulate(name, torch.float32)
    o64, _, _, _, _ = simulate(name, torch.float64)
    errs = {k: tc.err(o32[k].reshape(-1, 1) if k == "rnd" else o32[k].reshape(-1, o32["x"].shape[-1]),
                      o64[k].reshape(-1, 1) if k == "rnd" else o64[k].reshape(-1, o64["x"].shape[-1])) for k in ("x", "rnd", "xs")}
    xmax = float(o64["xs"].abs().max())
    print(f"rds_nn_{name}: err32 x {errs['x']:.2e} rnd {errs['rnd']:.2e} xs {errs['xs']:.2e}  max |x| {xmax:.1f}")
    assert max(errs.values()) <= 1e-3, f"{name}: the reference's float32 run is not within 1e-3 of its float64 run: {errs}"
    assert xmax <= 100.0, f"{name}: |x| reaches {xmax}"
    meta = dict(case=name, **{k: v for k, v in spec.items()}, d=int(x0.shape[1]), B=int(x0.shape[0]), N=int(ts.numel() - 1), clip_model=1e4,
                err32_x=errs["x"], err32_rnd=errs["rnd"], err32_xs=errs["xs"], keys=list(ctrl.state_dict().keys()))
    arrays = dict(ts=ts, x0=x0, tgt_loc=target.loc, tgt_scale=target.scale, tgt_w=target.mixture_weights, **gg.pack_params("ctrl.", gg.sd(ctrl)),
                  **{"out.x32": o32["x"], "out.rnd32": o32["rnd"], "out.xs32": o32["xs"], "out.x64": o64["x"], "out.rnd64": o64["rnd"],
                     "out.xs64": o64["xs"]})
    gg.save("rds_nn_" + name, meta, arrays)


def train(name="train_lv_rds_nn_b", case="b_ei"):
    """One log-variance training evaluation over the 'nn' reference (losses/oc.py:364-394, method='lv'): the loss and the gradient of
    every drift-net parameter under the replayed noise, in float32 and in float64."""
    out = {}
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        loss, ctrl, ts, x0, target, ref_distr = pieces(case, dtype)
        orig, rep = torch.randn_like, Replay(rc.CASES[case]["seed"])
        torch.randn_like = rep
        try:
            value, _ = loss(ts, x0.clone(), target.unnorm_log_prob, ref_distr.log_prob)
        finally:
            torch.randn_like = orig
        value.backward()
        out[tag] = (float(value), {k: p.grad.detach().clone() for k, p in ctrl.named_parameters() if p.grad is not None}, ctrl, ts, x0, target)
    v32, g32, ctrl, ts, x0, target = out["32"]
    v64, g64 = out["64"][:2]
    err = {k: float((g32[k].double() - g64[k]).abs().max() / (g64[k].abs().max() + 1e-300)) for k in g64}
    print(f"{name}: loss {v32:.6f} / {v64:.6f}; worst float32 gradient error {max(err.values()):.2e}")
    meta = dict(case=case, **rc.CASES[case], d=int(x0.shape[1]), B=int(x0.shape[0]), N=int(ts.numel() - 1), clip_model=1e4, loss32=v32, loss64=v64,
                err32_grad=err, keys=list(ctrl.state_dict().keys()))
    arrays = dict(ts=ts, x0=x0, tgt_loc=target.loc, tgt_scale=target.scale, tgt_w=target.mixture_weights, **gg.pack_params("ctrl.", gg.sd(ctrl)),
                  **{f"grad32.{k}": v for k, v in g32.items()}, **{f"grad64.{k}": v for k, v in g64.items()})
    gg.save(name, meta, arrays)


def main():
    names = sys.argv[1:] or list(rc.CASES) + ["train"]
    for n in names:
        train() if n == "train" else make(n)


if __name__ == "__main__":
    main()
