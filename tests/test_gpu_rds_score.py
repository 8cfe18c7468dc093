"""Reference samplers (RDS / LRDS) with a target-informed control on the HIP engine: ScoreCtrl / RemoveReferenceCtrl(CancelDriftCtrl) over
Gaussian, diagonal-mixture and full-covariance mixture references -- sampling (loss.simulate), the noising direction (loss.compute_eubo),
log-variance and KL training, against the real reference's outputs (tests/golden/gen_golden_rds_score.py).  GPU box only.

Bound of every simulate / EUBO case: max(1e-5, 10 x s), s = how far the REFERENCE's own fp32 result moves under a one-ulp relative
change of x0 (stored in the fixture) -- measured on the reference, never on the kernel.  Metrics as tests/test_gpu_parity.py: rel_err on
the states, log-weights relative to their largest summand."""
import pytest
import torch

from oracle import sde_oracle as orc
from sde_sampler_lrds_amd import engine as E
from tests import golden_cases as gc
from tests import rds_score_cases as rc

TOL = 1e-5


def _noise(c, gpu):
    m = c.meta
    return torch.stack([orc.philox_normal(m["seed"], k, 0, m["B"], m["d"]) for k in range(m["N"])]).to(gpu)


def _bound(c):
    scale = rc.rnd_scale(c)
    s = rc.ulp_sensitivity(c, scale)
    return scale, s, max(TOL, 10 * s)


def _errors(x, rnd, c, scale):
    ex = gc.rel_err(x.cpu(), c["out_x"])
    er = float(((rnd.cpu().double().view(-1, 1) - c["rnd"].double().view(-1, 1)).abs() / scale.double().view(-1, 1)).max())
    return ex, er


@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.SIM_CASES)
def test_simulate_matches_reference_fixture(gpu, name):
    """Injected noise (the normals the reference consumed, bit for bit), then the engine's own Philox stream.  The three shapes run a
    partial particle tile and idle waves of the shared-table kernels: B = 37 on 3 tiles, B = 20 on the 6-tile instance (d = 72), B = 48
    on the 8-tile instance (d = 100, phi^4).  (The phi^4 case is the one that amplifies: the reference's own x_N moves 5.1e-6 under one ulp
    of x0, so its bound is 5.1e-5 -- on states of size ~3 and log-weights whose largest summand is ~7e3; the other two stay near 1e-5.)"""
    c = rc.load(name)
    b = rc.build(c, gpu)
    scale, s, tol = _bound(c)
    for mode, noise in (("injected", _noise(c, gpu)), ("philox", None)):
        x, rnd, _ = b["loss"].simulate(b["ts"], b["x0"], *b["args"], noise=noise)
        torch.cuda.synchronize()
        ex, er = _errors(x, rnd, c, scale)
        print(f"{name} [{mode}]: max rel err x_N {ex:.2e}, rnd {er:.2e}   (bound {tol:.1e}; the reference moves {s:.1e} under one ulp of x0)")
        assert ex < tol and er < tol, (mode, ex, er, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.EUBO_CASES)
def test_compute_eubo_matches_reference_fixture(gpu, name):
    c = rc.load(name)
    b = rc.build(c, gpu)
    scale, s, tol = _bound(c)
    for mode, noise in (("injected", _noise(c, gpu)), ("philox", None)):
        x = b["x0"].clone()
        rnd = b["loss"].compute_eubo(b["ts"], x, *b["args"], noise=noise)  # noises x in place, like the reference
        torch.cuda.synchronize()
        ex, er = _errors(x, rnd, c, scale)
        print(f"{name} [{mode}]: max rel err noised x {ex:.2e}, rnd {er:.2e}   (bound {tol:.1e}; the reference moves {s:.1e} under one ulp of x0)")
        assert ex < tol and er < tol, (mode, ex, er, tol)


def _train(c, b, gpu):
    loss = b["loss"]
    loss.train_calls = 0
    ctrl = E.unwrap_ctrl(loss.generative_ctrl)[0]
    for p in ctrl.parameters():
        p.grad = None
    value, metrics = loss(b["ts"], b["x0"], *b["args"])
    value.backward()
    loss_err = abs(float(value.detach()) - c.meta["loss"]) / max(1.0, abs(c.meta["loss"]))
    worst, n = 0.0, 0
    for k, p in ctrl.named_parameters():
        if "grad." + k not in c.a:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        ref = c["grad." + k]
        worst, n = max(worst, float((p.grad.cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)), n + 1
    tol = max(TOL, 10 * c.meta["grad_sensitivity"])
    print(f"{c.name}: loss {float(value.detach()):.6f} vs {c.meta['loss']:.6f} (rel {loss_err:.1e}); worst relative gradient error {worst:.2e} over "
          f"{n} parameters (bound {tol:.1e}; the reference's gradient moves {c.meta['grad_sensitivity']:.1e} under a 1.2e-6 move of its normals)")
    assert n == sum(1 for k in c.a if k.startswith("grad.")) and n >= 8
    assert loss_err < 1e-5 and worst < tol, (loss_err, worst, tol)
    assert "train/n_filtered_cumulative" in metrics
    return loss


@pytest.mark.gpu
def test_lv_training_matches_reference(gpu):
    """Log-variance training over a full-covariance reference: the rollout is the new PAR = 1 instance, the gradient the fused pass."""
    c = rc.load(rc.TRAIN_LV)
    _train(c, rc.build(c, gpu), gpu)


@pytest.mark.gpu
def test_kl_training_matches_reference_on_the_stepwise_adjoint(gpu):
    """KL training with a full-covariance reference: forward on the new instances, gradient by the per-step adjoint (the one-launch
    adjoint serves diagonal references)."""
    c = rc.load(rc.TRAIN_KL)
    b = rc.build(c, gpu)
    b["loss"].max_rnd = None
    loss = _train(c, b, gpu)
    assert loss.last_adjoint_path == "stepwise"


@pytest.mark.gpu
def test_perturbed_lv_training_matches_reference(gpu):
    """sde_ctrl_noise and sde_ctrl_dropout both set: the PAR = 2 instance over a full-covariance reference."""
    c = rc.load(rc.CTRL_PERTURB)
    b = rc.build(c, gpu)
    b["loss"].sde_ctrl_noise, b["loss"].sde_ctrl_dropout = c.meta["sde_ctrl_noise"], c.meta["sde_ctrl_dropout"]
    _train(c, b, gpu)


@pytest.mark.gpu
def test_large_batch_is_reproducible_shardable_and_pad_features_stay_out(gpu):
    """d = 100 (7 live tiles on the 8-tile instance), phi^4, K = 2 full covariance, B = 20 000, N = 16, the engine's own noise.  x_in has row
    stride d: the pad columns of the state cannot be reached from outside, so the first 48 particles -- the fixture's, same seed, same
    global indices -- are held row by row to the reference's result instead: a pad feature's noise leaking through the lattice term into
    feature 99 would show there."""
    c = rc.load("rds_em_score_phi4_fullcov_d100_k2")
    b = rc.build(c, gpu)
    m, loss = c.meta, b["loss"]
    B = 20000
    x0 = orc.philox_normal(m["seed"], 0, 0, B, m["d"], stream=1).to(gpu)
    assert torch.equal(x0[:m["B"]].cpu(), c["x0"])
    x, rnd, _ = loss.simulate(b["ts"], x0, *b["args"])
    x2, rnd2, _ = loss.simulate(b["ts"], x0, *b["args"])
    assert torch.equal(x, x2) and torch.equal(rnd, rnd2)
    assert torch.isfinite(rnd).all() and torch.isfinite(x).all()
    for p0, sl in ((0, slice(0, B // 2)), (B // 2, slice(B // 2, None))):
        loss.particle0 = p0
        xs_, rs_, _ = loss.simulate(b["ts"], x0[sl].contiguous(), *b["args"])
        assert torch.equal(xs_, x[sl]) and torch.equal(rs_, rnd[sl]), p0
    loss.particle0 = 0
    scale, s, tol = _bound(c)
    ex, er = _errors(x[:m["B"]], rnd[:m["B"]], c, scale)
    worst_col = int(((x[:m["B"]].cpu() - c["out_x"]).abs() / c["out_x"].abs().clamp(min=1.0)).max(dim=0).values.argmax())
    print(f"B = {B}: first {m['B']} rows vs the reference x_N {ex:.2e} (worst feature {worst_col}), rnd {er:.2e}   (bound {tol:.1e})")
    assert ex < tol and er < tol


def _phi4_model(integrator, model_type, full, gpu, d=100):
    from sde_sampler_lrds_amd.experiments.benchmark_utils import make_model, make_target_details
    g = torch.Generator().manual_seed(5)
    means = torch.stack([torch.ones(d), -torch.ones(d)]) * 0.9 + 0.05 * torch.randn(2, d, generator=g)
    if full:  # as experiments/sample_phi_four_gmm_mcmc.py passes a full-covariance fit: torch.linalg.eigh(covariances)
        a = torch.randn(2, d, d, generator=g) / d ** 0.5
        variances = torch.linalg.eigh(0.05 * a @ a.transpose(-1, -2) + 0.05 * torch.eye(d))
    else:
        variances = 0.05 * (1.0 + torch.rand(2, d, generator=g))
    details = dict(means_ref=means, variances_ref=variances, weights_ref=torch.tensor([0.5, 0.5]))
    train = dict(train_batch_size=256, eval_batch_size=512, train_steps=3)
    model = make_model("vp-ref", "gmm", "lv", integrator, model_type, "uniform", details, make_target_details("phi_four", dim=d), train,
                       n_steps=16, compute_samples_based_metrics=False, device=gpu)

    # PhiFour has no sampler (upstream neither, so its TrainableWrapper skips the EUBO metrics on this target): hand the wrapper samples
    # around the two wells of the lattice, as the experiment has its MCMC data set at hand
    def sample(shape):
        n = shape[0]
        return torch.stack([torch.ones(d), -torch.ones(d)])[torch.arange(n) % 2] * 0.9 + 0.1 * torch.randn(n, d, generator=g)
    model.target.sample = sample
    return model


@pytest.mark.gpu
@pytest.mark.parametrize("integrator,model_type,full", [("ei", "target_informed_zero_init", True), ("ei", "target_informed_zero_init", False),
                                                        ("em", "target_informed_langevin_init", True)])
def test_phi_four_lrds_end_to_end(gpu, integrator, model_type, full):
    """make_model -> TrainableWrapper.run(): three log-variance training steps, sampling and the EUBO-side metrics, every pass a HIP launch."""
    from sde_sampler_lrds_amd.additions.hacking import TrainableWrapper
    model = _phi4_model(integrator, model_type, full, gpu)
    res = TrainableWrapper(model, verbose=False).run()
    got = {k: res.metrics[k] for k in ("eval/elbo", "eval/eubo", "eval/norm_effective_sample_size_f")}
    print(f"phi_four d=100 {integrator} {model_type} {'full-covariance' if full else 'diagonal'} reference: {got}")
    assert all(torch.isfinite(torch.tensor(v)) for v in got.values()), got
    assert torch.isfinite(res.samples).all() and torch.isfinite(res.weights).all()
