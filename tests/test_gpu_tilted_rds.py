"""RDS over an energy-based ('nn') reference on the GPU: sdeng_tilted_simulate against the reference's own float64 runs with its own
float32 runs as the yardstick (tests/golden/rds_nn_*.npz, MARGIN x err32 as for every tilted kernel); the one-step residual of every
step against the launches that exist (E.tilted_eval, E.ctrl_forward, E.philox_noise); bit-exact properties; the launch geometries; the
public interface (make_model, evaluate, one log-variance training call against train_lv_rds_nn_b.npz) and its refusals."""
import math

import pytest
import torch

from oracle import sde_oracle as orc
from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.experiments import benchmark_utils as bu
from tests import rds_nn_cases as rc
from tests import tilted_cases as tc
from tests.test_gpu_tilted import MARGIN

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24  # unit round-off of float32
F64 = torch.float64
_CACHE = {}


def setup(name, gpu, steps=rc.N):
    """(fixture, net, control, coefficient table, time table, form) of a case on the GPU at ``steps`` steps, built once."""
    key = (name, steps)
    if key not in _CACHE:
        fx = rc.Fixture(name)
        net, ctrl = fx.net().to(gpu), fx.ctrl().to(gpu)
        coef = E.coef_table(rc.KIND[fx.spec["integrator"]], rc.grid(fx.spec, steps), E._cpu_sde(net.sde), with_ref=True)
        tinfo = E.tilted_times(net, coef[:, 0], steps, per_row=True)[2]
        _CACHE[key] = (fx, net, ctrl, coef.to(gpu), tinfo.to(gpu), L.FORM_EM if fx.spec["integrator"] == "em" else L.FORM_LIN)
    return _CACHE[key]


def x0_of(fx, batch, gpu):
    """x0 of the case at another batch size: the fixture's rule (rds_nn_cases.draw_x0) on the CPU copy of the net."""
    return rc.draw_x0(fx.spec, fx.net(), orc.philox_normal, batch).to(gpu)


# ---- 1. the fixtures -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_parity_with_the_reference(name, gpu):
    """x_N, rnd (terminal costs added with sdeng_tilted_eval at eps and sdeng_dist_eval, as the loss does) and the trajectory under the
    fixture's replayed noise against the reference's float64 run: err <= MARGIN x the reference's own float32 err."""
    fx, net, ctrl, coef, tinfo, form = setup(name, gpu)
    B, d = fx["x0"].shape
    z = torch.stack([orc.philox_normal(fx.spec["seed"], k, 0, B, d) for k in range(rc.N)]).to(gpu)
    x, rnd, xs, _ = E.tilted_simulate(net, ctrl, coef, tinfo, fx["x0"].to(gpu), form=form, noise=z, return_traj=True)
    assert torch.isfinite(xs).all() and torch.isfinite(rnd).all() and torch.equal(xs[-1], x) and torch.equal(xs[0], fx["x0"].to(gpu))
    rnd = rnd + E.tilted_eval(net, fx["ts"][:1], x, want_grad=False)[0].view(-1, 1) - E.dist_eval(fx.target().to(gpu), x, want_score=False)[0]
    got = dict(x=x.cpu(), rnd=rnd.cpu().reshape(-1, 1), xs=xs.cpu().reshape(-1, d))
    want = dict(x=fx["out.x64"], rnd=fx["out.rnd64"].reshape(-1, 1), xs=fx["out.xs64"].reshape(-1, d))
    errs = {k: tc.err(got[k], want[k]) for k in got}
    print(f"\ntilted_simulate parity case {name}: d={d} B={B} N={rc.N}  " + "  ".join(
        f"{k} err {errs[k]:.3e} (reference float32 {fx.meta['err32_' + k]:.3e}, ratio {errs[k] / fx.meta['err32_' + k]:.2f})" for k in errs))
    for k in errs:
        assert errs[k] <= MARGIN * fx.meta["err32_" + k], k


# ---- 2. one-step residual ----------------------------------------------------------------------------------------------------------------------
def residual(fx, net, ctrl, coef, form, xs, rnd, ref, z):
    """Every step of the kernel's own trajectory recomputed from xs[k] with the yardsticks.  The reference score must be E.tilted_eval's bit
    for bit.  With u = E.ctrl_forward (held to the float64 module: dev_k = MARGIN x its largest error at the step) the float64 value of
    the update's expression bounds the kernel's float32 evaluation elementwise by
        4 EPS x (sum of the magnitudes of the terms and of the result)  +  |control gain| x dev_k
    -- two roundings per fused term, the products of two coefficients formed in float32, as test_gpu_tilted_moves.proposal_bound -- and
    the running cost, recomputed in float64 from u and z, by n EPS x (the sums of the magnitudes), n = d + 8 terms per reduction,
    plus dev_k x sum_f (2 |c4 u_f| + |c5 z_f|), plus three roundings of the running value per step.  Returns the largest ratios."""
    N, (B, d) = coef.shape[0], xs.shape[1:]
    ctrl64 = fx.ctrl(F64).to(xs.device)
    lin = form == L.FORM_LIN
    rnd64, rnd_bound, worst_x = torch.zeros(B, dtype=F64, device=xs.device), torch.zeros(B, dtype=F64, device=xs.device), 0.0
    for k, row in enumerate(coef.cpu().double().tolist()):
        t, c1, c2, c3, c4, c5, c6 = row[:7]
        lp, g = E.tilted_eval(net, float(row[0]), xs[k])
        assert torch.equal(g, ref[k]), f"step {k}: the kernel's reference score is not E.tilted_eval's"
        u32 = E.ctrl_forward(ctrl, float(row[0]), xs[k])
        with torch.no_grad():
            dev = MARGIN * float((u32.double() - ctrl64(torch.tensor(row[0], dtype=F64, device=xs.device), xs[k].double())).abs().max())
        x, u, r, zz = xs[k].double(), u32.double(), g.double(), z[k].double()
        if lin:
            terms = [c1 * x, c2 * (u + r), c3 * zz]
            gain = abs(c2)
            rnd_k, mags = c4 * (u * u).sum(-1) + c5 * (u * zz).sum(-1) + c6, abs(c4) * (u * u).sum(-1) + abs(c5) * (u * zz).abs().sum(-1) + abs(c6)
            sens = (2 * abs(c4) * u.abs() + abs(c5) * zz.abs()).sum(-1)
        else:
            terms = [x, c4 * c1 * x, c4 * c3 * r, c4 * c2 * u, c2 * c5 * zz]
            gain = abs(c4 * c2)
            rnd_k = 0.5 * (u * u).sum(-1) * c4 + c5 * (u * zz).sum(-1) + c6
            mags = 0.5 * abs(c4) * (u * u).sum(-1) + abs(c5) * (u * zz).abs().sum(-1) + abs(c6)
            sens = (abs(c4) * u.abs() + abs(c5) * zz.abs()).sum(-1)
        new = sum(terms)
        bound = 4.0 * EPS * (sum(v.abs() for v in terms) + new.abs()) + gain * dev
        worst_x = max(worst_x, float(((xs[k + 1].double() - new).abs() / bound).max()))
        rnd64 = rnd64 + rnd_k
        rnd_bound = rnd_bound + (d + 8) * EPS * mags + dev * sens + 3.0 * EPS * rnd64.abs()
    return worst_x, float(((rnd.double().reshape(-1) - rnd64).abs() / rnd_bound).max())


@pytest.mark.parametrize("name", ["a_ei", "b_ei", "b_em", "c_ei"])
def test_every_step_against_the_launches_that_exist(name, gpu):
    """N = 12 on the cases a, b (both integrators) and c: catches a wrong time index, a stale image or a wrong noise counter at the step
    where it happens, with no chaotic amplification."""
    fx, net, ctrl, coef, tinfo, form = setup(name, gpu, 12)
    x0 = fx["x0"].to(gpu)
    x, rnd, xs, ref = E.tilted_simulate(net, ctrl, coef, tinfo, x0, form=form, seed=fx.spec["seed"], return_traj=True, want_ref=True)
    z = E.philox_noise(fx.spec["seed"], 12, x0.shape[0], x0.shape[1], 0, gpu)
    rx, rr = residual(fx, net, ctrl, coef, form, xs, rnd, ref, z)
    print(f"\ntilted_simulate one-step residual case {name}: worst state ratio {rx:.3f}, running-cost ratio {rr:.3f} (of the bound)")
    assert rx <= 1.0 and rr <= 1.0


# ---- 3. bit-exact properties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a_ei", "b_em", "c_ei"])
def test_bit_exact_properties(name, gpu):
    fx, net, ctrl, coef, tinfo, form = setup(name, gpu, 4)
    seed, B = fx.spec["seed"], 48
    x0 = x0_of(fx, B, gpu)
    run = lambda x, **kw: E.tilted_simulate(net, ctrl, coef, tinfo, x, form=form, seed=seed, **kw)  # noqa: E731
    x, rnd, xs, ref = run(x0, return_traj=True, want_ref=True)
    again = run(x0, return_traj=True, want_ref=True)
    assert all(torch.equal(a, b) for a, b in zip((x, rnd, xs, ref), again))  # a rerun
    plain = run(x0)  # no trajectory: the ping-pong rows of the workspace, the score rows of the workspace
    assert plain[2] is None and plain[3] is None and torch.equal(plain[0], x) and torch.equal(plain[1], rnd)
    lo, hi = run(x0[:16].contiguous(), return_traj=True), run(x0[16:].contiguous(), particle0=16, return_traj=True)  # 48 = 16 + 32
    assert torch.equal(torch.cat([lo[0], hi[0]]), x) and torch.equal(torch.cat([lo[1], hi[1]]), rnd) and torch.equal(torch.cat([lo[2], hi[2]], 1), xs)
    z = E.philox_noise(seed, 4, B, x0.shape[1], 0, gpu)
    inj = run(x0, noise=z, return_traj=True)  # the caller's noise = the kernel's own draw
    assert torch.equal(inj[0], x) and torch.equal(inj[1], rnd) and torch.equal(inj[2], xs)
    other = E.tilted_simulate(net, ctrl, coef, tinfo, x0, form=form, seed=seed + 1)
    assert not torch.equal(other[0], x)
    no_ito = E.tilted_simulate(net, ctrl, coef, tinfo, x0, form=form, seed=seed, flags=0)
    assert torch.equal(no_ito[0], x) and not torch.equal(no_ito[1], rnd)


# ---- 4. launch geometries --------------------------------------------------------------------------------------------------------------------------
GEOMETRIES = {"idle_wave": 8193, "second_round": 65537}  # test_gpu_tilted_moves.GEOMETRIES: two waves / one idle / 15 pad rows; eight waves, second round


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_launch_geometry(geo, gpu):
    """Case a's net (d = 2), N = 2, against the host composition with the one-step bound; every row moves and is finite."""
    fx, net, ctrl, coef, tinfo, form = setup("a_ei", gpu, 2)
    B = GEOMETRIES[geo]
    x0 = torch.randn(B, 2, generator=torch.Generator().manual_seed(5)).to(gpu)
    x, rnd, xs, ref = E.tilted_simulate(net, ctrl, coef, tinfo, x0, form=form, seed=9, return_traj=True, want_ref=True)
    assert torch.isfinite(x).all() and torch.isfinite(rnd).all() and not (x == x0).all(dim=1).any()
    rx, rr = residual(fx, net, ctrl, coef, form, xs, rnd, ref, E.philox_noise(9, 2, B, 2, 0, gpu))
    print(f"\ntilted_simulate geometry {geo}: B={B} worst state ratio {rx:.3f}, running-cost ratio {rr:.3f}")
    assert rx <= 1.0 and rr <= 1.0
    plain = E.tilted_simulate(net, ctrl, coef, tinfo, x0, form=form, seed=9)
    assert torch.equal(plain[0], x) and torch.equal(plain[1], rnd)


# ---- 5. through the public interface -----------------------------------------------------------------------------------------------------------------
TRAIN = dict(train_steps=10, train_batch_size=64, eval_batch_size=96)


def make(gpu, model_type="base_zero_init", loss_type="lv"):
    net = tc.mirror("b")[1]
    target = bu.make_target_details("many_modes", dim=net.dim, n_modes=3)
    return bu.make_model("vp-ref", "nn", loss_type, "ei", model_type, "uniform", dict(net=net, sigma=1.0), target, TRAIN, n_steps=8,
                         compute_samples_based_metrics=False, device=gpu), net


def test_make_model_evaluates_and_trains(gpu):
    model, net = make(gpu)
    first = model.evaluate()
    logz = first.log_norm_const_preds["log_norm_const_is"]
    assert math.isfinite(float(logz)) and torch.isfinite(first.samples).all() and first.xs.shape == (9, 96, net.dim)
    # one log-variance training call against the reference's loss + backward() under the replayed noise
    fx = rc.Fixture("train_lv_rds_nn_b")
    model.generative_ctrl.load_state_dict({k[5:]: v for k, v in fx.a.items() if k.startswith("ctrl.")})
    model.loss.seed, model.loss.train_calls = fx.spec["seed"], 0
    target = fx.target().to(gpu)
    value, _ = model.loss(fx["ts"].to(gpu), fx["x0"].to(gpu), target.unnorm_log_prob, model.reference_distr.log_prob)
    value.backward()
    print(f"\ntilted_simulate training case b: loss {float(value.detach()):.6f} (reference float32 {fx.meta['loss32']:.6f}, float64 {fx.meta['loss64']:.6f})")
    for k, p in model.generative_ctrl.named_parameters():
        if "grad64." + k not in fx.a:
            continue
        g64 = fx["grad64." + k]
        err = float((p.grad.cpu().double() - g64).abs().max() / (g64.abs().max() + 1e-300))
        print(f"  grad {k}: err {err:.3e} (reference float32 {fx.meta['err32_grad'][k]:.3e}, ratio {err / fx.meta['err32_grad'][k]:.2f})")
        assert err <= MARGIN * fx.meta["err32_grad"][k], k
    assert abs(float(value) - fx.meta["loss64"]) <= MARGIN * abs(fx.meta["loss32"] - fx.meta["loss64"])
    # another reference and back: the first evaluation's bits
    fresh, net2 = make(gpu)
    a = fresh.evaluate()
    fresh.change_reference_type("gmm", weights=torch.ones(2), means=torch.zeros(2, net.dim), variances=torch.ones(2, net.dim))
    b = fresh.evaluate()
    fresh.change_reference_type("nn", net=net2, eps=torch.tensor(0.0))
    c = fresh.evaluate()
    assert not torch.equal(b.samples, a.samples)
    assert torch.equal(c.samples, a.samples) and torch.equal(c.weights, a.weights) and torch.equal(c.xs, a.xs)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_gpu(gpu):
    model, _ = make(gpu, model_type="target_informed_zero_init")  # a ScoreCtrl
    with pytest.raises(E.UnsupportedByEngine, match="ScoreCtrl over an energy-based"):
        model.evaluate()
    model, _ = make(gpu, loss_type="kl")
    x = model.prior.sample((64,)).to(gpu)
    ts = model.train_timesteps(device=gpu)
    with pytest.raises(E.UnsupportedByEngine, match="second order in the energy net"):
        model.loss(ts, x, model.clipped_target_unnorm_log_prob, model.reference_distr.log_prob)
    model, _ = make(gpu)
    with pytest.raises(E.UnsupportedByEngine, match="compute_eubo over an energy-based"):
        model.loss.compute_eubo(ts, x, model.clipped_target_unnorm_log_prob, model.reference_distr.log_prob)
    model.loss.sde_ctrl_noise = 0.1
    with pytest.raises(E.UnsupportedByEngine, match="sde_ctrl_noise / sde_ctrl_dropout over an energy-based"):
        model.loss(ts, x, model.clipped_target_unnorm_log_prob, model.reference_distr.log_prob)
