"""Every packed split-f16 image (csrc/image_format.hpp) and the outputs of one small run per step-loop family, written to a file by one build
of the library and compared by another (SDENG_LIB, tools/probe_lib.py): what a refactor of the packers has to leave as it is.

    SDENG_LIB=/path/to/parent/libsdeng.so python tools/probe_image_bits.py --write bits.pt
    python tools/probe_image_bits.py --compare bits.pt            # exit status 1 on any difference

Written: the raw words of the drift-net images, forward and transposed, in a VjpSession's workspace (NT = 1 .. 8; weights in range, at the
reference's near-zero last layer, and with one matrix times 3e4); the image slots and the constants of the tilted net in its cached
workspace (a diagonal and an eigen-form prior; the words a pack writes, not the rest of a slot); the CMCD prior's precision image and
padded mean; and x_N, rnd of one simulate per step-loop family at 64 particles x 4 steps -- sim with no reference, a Gaussian, K = 4,
K = 16 with shared and with separate variances, full covariances; split tiles; cmcd; euler -- next to ctrl_vjp, kl_adjoint,
cmcd_kl_adjoint and tilted_simulate.  Every input is drawn on the CPU from a seeded generator; the in-kernel noise is counter-based."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probe_lib  # noqa: E402

LIB = probe_lib.select()
from sde_sampler_lrds_amd import _lib as L  # noqa: E402
from sde_sampler_lrds_amd import engine as E  # noqa: E402
from sde_sampler_lrds_amd.distr.gauss import GMM, Gauss, ManyModes  # noqa: E402
from sde_sampler_lrds_amd.eq import sdes  # noqa: E402
from sde_sampler_lrds_amd.experiments import baseline_configs as cfgs  # noqa: E402
from sde_sampler_lrds_amd.losses import oc  # noqa: E402
from sde_sampler_lrds_amd.models import mlp, reparam  # noqa: E402
from sde_sampler_lrds_amd.models import utils as mutils  # noqa: E402
from sde_sampler_lrds_amd.reference import MarginalReference  # noqa: E402
from tests import tilted_cases as tc  # noqa: E402

B, N = 64, 4
BLOCK, SLOT = 512, 16384


def align64(n):
    return (n + 63) // 64 * 64


def words(ws):
    torch.cuda.synchronize()
    return ws.view(torch.float32).cpu().view(torch.int32)  # as integers: NaN payloads compare like any other bits


CMCD_WORKSPACE = {}
_engine_run = E.run


def run_and_keep_cmcd_workspace(desc, x, keep, **kw):
    """E.run; after a CMCD call, the words of the workspace that call asked for."""
    res = _engine_run(desc, x, keep, **kw)
    if desc.form == L.FORM_CMCD:
        CMCD_WORKSPACE["words"] = words(E._WS.buf[x.device])[:L.lib().sdeng_workspace_bytes(ctypes.byref(desc)) // 4]
    return res


def drift_net(d, state, g):
    """state 0: every matrix in the un-scaled range; 1: the reference's near-zero last layer; 2: matrix d % 4 times 3e4."""
    torch.manual_seed(1000 + d)
    net = mlp.FourierMLP(dim=d, activation=torch.nn.GELU(), num_layers=4, channels=64, last_bias_init=mutils.init_bias_uniform_zeros,
                         last_weight_init=mutils.kaiming_uniform_zeros_)
    with torch.no_grad():
        if state != 1:
            for p in net.parameters():
                if p.dim() == 2 and p.shape[0] > 1:
                    p.copy_(2.0 * torch.rand(p.shape, generator=g) - 1.0)
        if state == 2:
            mod = [net.input_embed, net.hidden_layer[0], net.hidden_layer[1], net.out_layer][d % 4]
            mod.weight.mul_(3e4)
            mod.bias.mul_(3e4)
    return net


def drift_images(dev, out):
    g = torch.Generator().manual_seed(11)
    for nt in range(1, 9):
        d = 16 * nt - 3
        weights = (4 * ((nt + 1) // 2) + 16 + 2 * nt) * BLOCK
        total = align64(weights + 3 * 64 + 16 * nt + 8) + weights  # the forward image, biases and scales; the transposed image behind them
        for state in range(3):
            ctrl = reparam.ClippedCtrl(base_model=drift_net(d, state, g), clip_model=1e4).to(dev)
            s = E.VjpSession(ctrl, torch.tensor([0.4]), torch.randn(1, 16, d, generator=g).to(dev))
            out[f"drift/nt{nt}.state{state}.u"] = s.forward_u()
            out[f"drift/nt{nt}.state{state}.images"] = words(s.ws)[:total]


def tilted_images(dev, out):
    for nt, prior in ((7, "diag"), (3, "eig")):
        spec = tc.walk_spec(nt, prior)
        net = tc.build(spec, mlp, reparam, sdes)
        t, x = tc.draw_inputs(spec, net)
        net = net.to(dev).requires_grad_(False)
        lp, grad = E.tilted_eval(net, t.to(dev), x.to(dev))
        out[f"tilted/{prior}.lp"], out[f"tilted/{prior}.grad"] = lp, grad
        ws = words(E._TILTED_PACKS[net][1])
        d, K = spec["d"], spec["K"]
        kbd = (d + 31) // 32
        blocks = [32, 32, 32, 8 * kbd] + [32] * 4 + [nt * 4, 8 * kbd] + [32] * 4 + [nt * 4] + ([nt * kbd] * (2 * K) if prior == "eig" else [])
        for slot, nb in enumerate(blocks):
            out[f"tilted/{prior}.slot{slot}"] = ws[slot * SLOT:slot * SLOT + nb * BLOCK]
        cs = ws[len(blocks) * SLOT:]
        out[f"tilted/{prior}.consts"] = torch.cat([cs[:1536], cs[1536:1536 + len(blocks)], cs[1600:1600 + len(blocks)], cs[1664:1680 + 2 * 16 * 128]])


def simulate(name, loss, ts, x0, args, kw, out):
    x, rnd, _ = loss.simulate(ts, x0, *args, **kw)
    out[f"sim/{name}.x"], out[f"sim/{name}.rnd"] = x, rnd


def reference_sampler(dev, d, K, ref_kind, ref_args, seed=1):
    torch.manual_seed(seed)
    sde = sdes.VP(0.1, 10.0, 1.0, terminal_t=1.0)
    target = ManyModes(n_modes=K, dim=d, var=0.5, seed_loc=42, mixture_weight_factor=3.0, n_reference_samples=10)
    ctrl = reparam.ClippedCtrl(base_model=cfgs._net(d), clip_model=1e4)
    ref = MarginalReference(sde, ref_kind, **ref_args(target))
    for m in (sde, target, ctrl, ref):
        m.to(dev)
    loss = oc.EIReferenceSDELoss(ctrl, ctrl, sde=sde, method="lv", reference_ctrl=ref)
    x0 = torch.randn(B, d, generator=torch.Generator().manual_seed(seed)).to(dev)
    return loss, torch.linspace(0.0, 1.0, N + 1, device=dev), x0, (target.unnorm_log_prob, ref.reference_distr.to(dev).log_prob)


def step_loops(dev, out):
    g = torch.Generator().manual_seed(5)
    loss, ts, x0, args, kw, _ = cfgs.build_pis_phi4(dev, B, N)
    simulate("no_reference", loss, ts, x0, args, kw, out)
    simulate("gauss", *reference_sampler(dev, 40, 1, "gaussian", lambda t: dict(x_init=t.loc[0].clone(), var_init=0.3 + torch.rand(40, generator=g))), {}, out)
    loss, ts, x0, args, kw, _ = cfgs.build_rds_gmm(dev, B, N, d=128, K=4)
    simulate("k4", loss, ts, x0, args, kw, out)
    loss.split_tiles = True
    simulate("split", loss, ts, x0, args, kw, out)
    loss, ts, x0, args, kw, _ = cfgs.build_rds_gmm(dev, B, N, d=100, K=16)
    simulate("k16_shared", loss, ts, x0, args, kw, out)
    loss, ts, x0, args, kw, _ = cfgs.build_rds_gmm(dev, B, N, d=100, K=16, ref_var=0.3 + torch.rand(16, 100, generator=g))
    simulate("k16_separate", loss, ts, x0, args, kw, out)
    A = torch.randn(3, 72, 72, generator=g) / 72 ** 0.5
    simulate("full_covariance", *reference_sampler(dev, 72, 3, "gmm", lambda t: dict(
        means_init=t.loc.clone(), variances_init=0.3 * A @ A.transpose(-1, -2) + 0.4 * torch.eye(72), weights_init=torch.ones(3))), {}, out)
    loss, ts, x0, args, kw, info = cfgs.build_cmcd_logreg(dev, B, N)
    simulate("cmcd", loss, ts, x0, args, kw, out)
    # the CMCD prior's precision image and padded mean: the last two pieces of that call's workspace (the caller gave x0)
    nt = (info["d"] + 15) // 16
    image, loc = align64(nt * ((nt + 1) // 2) * BLOCK), align64(16 * nt)
    start = CMCD_WORKSPACE["words"].numel() - loc - image
    out["cmcd/prior_image"] = CMCD_WORKSPACE["words"][start:start + image + 16 * nt]
    tgt = GMM(dim=24, loc=2.0 * torch.randn(3, 24, generator=g), scale=0.5 + 0.3 * torch.rand(3, 24, generator=g), mixture_weights=torch.tensor([0.5, 0.3, 0.2])).to(dev)
    out["sim/euler.xs"] = E.euler_states(sdes.LangevinSDE(tgt.score, 1.0, 100.0).to(dev), torch.linspace(0.0, 1.0, N + 1, device=dev),
                                         torch.randn(B, 24, generator=g).to(dev), seed=3)


def training(dev, out):
    g = torch.Generator().manual_seed(6)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    d = 72
    ctrl = reparam.ClippedCtrl(base_model=cfgs._net(d), clip_model=1e4).to(dev)
    arrays = E.ctrl_vjp(ctrl, torch.linspace(0.9, 0.1, N), rn(N, B, d), rn(N, B, d), want_gx=True)
    coef = torch.zeros(N, L.NCOEF)
    coef[:, 0] = torch.linspace(0.9, 0.1, N)
    for col, (lo, width) in {1: (0.9, 0.2), 2: (0.3, 0.5), 3: (0.2, 0.3), 4: (0.05, 0.1), 5: (0.2, 0.2)}.items():
        coef[:, col] = lo + width * torch.rand(N, generator=g)
    w = (torch.rand(B, 1, generator=g) / B).to(dev)
    kl, lam0 = E.kl_adjoint(ctrl, coef.to(dev), 1.2 * rn(N, B, d), rn(N, B, d), w, 0.1 * rn(B, d), lin=True, ito=True)
    target = GMM(dim=d, loc=1.5 * torch.randn(3, d, generator=g), scale=0.5 + torch.rand(3, d, generator=g), mixture_weights=0.5 + torch.rand(3, generator=g)).to(dev)
    prior = Gauss(dim=d, loc=0.3 * torch.randn(d, generator=g), scale=0.8 + torch.rand(d, generator=g)).to(dev)
    sde = sdes.ControlledLangevinSDE(target_score=target.score, prior_score=prior.score, diff_coeff=1.2, terminal_t=1.0, clip_score=None).to(dev)
    ccoef = E.coef_table("cmcd", torch.linspace(0.0, 1.0, N + 1), E._cpu_sde(sde)).to(dev)
    ckl, clam0 = E.cmcd_kl_adjoint(ctrl, sde, ccoef, 1.2 * rn(N + 1, B, d), 0.3 * rn(N, B, d), w, 0.1 * rn(B, d))
    for name, a in (("ctrl_vjp", arrays), ("kl_adjoint", kl), ("cmcd_kl_adjoint", ckl)):
        for k in ("a0", "a1", "a2", "d0", "d1", "d2", "dout", "gx"):
            if a.get(k) is not None:
                out[f"train/{name}.{k}"] = a[k]
    out["train/kl_adjoint.lam0"], out["train/cmcd_kl_adjoint.lam0"] = lam0, clam0


def tilted_rds(dev, out):
    spec = tc.walk_spec(6, "eig")
    net = tc.build(spec, mlp, reparam, sdes).to(dev).requires_grad_(False)
    d = spec["d"]
    torch.manual_seed(8)
    ctrl = reparam.ClippedCtrl(base_model=cfgs._net(d), clip_model=1e4).to(dev).requires_grad_(False)
    coef = E.coef_table("ei", torch.linspace(0.0, 1.0, N + 1), E._cpu_sde(net.sde), with_ref=True)
    tinfo = E.tilted_times(net, coef[:, 0], N, per_row=True)[2].to(dev)
    x0 = torch.randn(B, d, generator=torch.Generator().manual_seed(9)).to(dev)
    x, rnd, xs = E.tilted_simulate(net, ctrl, coef.to(dev), tinfo, x0, seed=3, return_traj=True)[:3]
    out["sim/tilted_simulate.x"], out["sim/tilted_simulate.rnd"], out["sim/tilted_simulate.xs"] = x, rnd, xs


def main():
    ap = argparse.ArgumentParser()
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--write", metavar="FILE")
    mode.add_argument("--compare", metavar="FILE")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"# library {LIB}; device {torch.cuda.get_device_name(0)}")
    E.run = run_and_keep_cmcd_workspace
    out = {}
    drift_images(dev, out)
    tilted_images(dev, out)
    step_loops(dev, out)
    training(dev, out)
    tilted_rds(dev, out)
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().contiguous() for k, v in out.items()}
    n_img = sum(v.numel() for k, v in out.items() if v.dtype == torch.int32)
    finite = [k for k, v in out.items() if v.is_floating_point() and not bool(torch.isfinite(v).all())]
    out = {k: v.view(torch.int32) if v.dtype == torch.float32 else v for k, v in out.items()}  # bits: a NaN equals the same NaN
    print(f"# {len(out)} arrays: {n_img} image words, {sum(v.numel() for v in out.values()) - n_img} output values; not finite: {', '.join(finite) or 'none'}")
    if a.write:
        torch.save(out, a.write)
        print(f"# written to {a.write}")
        return 0
    ref = torch.load(a.compare)
    differ = [k for k in sorted(set(out) | set(ref)) if k not in out or k not in ref or not torch.equal(out[k], ref[k])]
    for k in differ:
        if k in out and k in ref and out[k].shape == ref[k].shape:
            print(f"DIFFERS {k}: {int((out[k] != ref[k]).sum())} of {out[k].numel()} values")
        else:
            print(f"DIFFERS {k}: missing on one side, or another shape")
    print(f"# compared with {a.compare}: {len(out) - len(differ)} of {len(out)} arrays torch.equal" + ("" if differ else " -- every image word and output bit is the same"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
