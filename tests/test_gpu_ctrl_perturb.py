"""Log-variance training with a perturbed simulated control: ``sde_ctrl_noise`` / ``sde_ctrl_dropout`` (BaseOCLoss.generative_and_sde_ctrl,
losses/oc.py:97-102), the control-perturbation stage of the step-loop kernels (SDENG_FLAG_CTRL_NOISE / _DROPOUT, include/sdeng.h).  Fixtures:
the real reference's ``loss(...)`` + ``backward()`` under the replayed engine noise, tests/golden/gen_golden_ctrl_perturb.py."""
import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from tests import build_cases as bc
from tests import golden_cases as gc

KINDS = {"train_lv": "rds_gmm", "train_lv_dis": "dis_ei", "train_lv_dis_orig": "dis_orig", "train_lv_dds": "dds", "train_lv_pis": "pis_phi4"}
NAMES = ["ctrl_perturb_em_gmm_d16_noise", "ctrl_perturb_ei_gmm_d16_noise_dropout", "ctrl_perturb_ddpm_gmm_d16_dropout",
         "ctrl_perturb_pis_phi4_d100_noise_dropout", "ctrl_perturb_dis_ei_d8_noise_dropout", "ctrl_perturb_dis_orig_d8_noise",
         "ctrl_perturb_dds_d2_noise", "ctrl_perturb_ei_gmm_d128_noise_dropout"]
BIG = "ctrl_perturb_ei_gmm_d128_noise_dropout"  # B = 512, d = 128: the split-tile kernel's ground when split_tiles is on


def _build(name, gpu, split=False, noise="fixture", dropout="fixture"):
    c = gc.load(name)
    c.meta["kind"] = KINDS[c.meta["kind"]]
    b = bc.build(c, gpu)
    loss = b["loss"]
    loss.method, loss.split_tiles = "lv", split
    loss.sde_ctrl_noise = c.meta["sde_ctrl_noise"] if noise == "fixture" else noise
    loss.sde_ctrl_dropout = c.meta["sde_ctrl_dropout"] if dropout == "fixture" else dropout
    return c, b


def _train(b, ts=None, x0=None):
    """One training call from the loss's first training seed -> (loss value, {parameter: gradient}, (x_N, rnd, xs) of its step loop)."""
    loss = b["loss"]
    loss.train_calls = 0
    ctrl = loss.generative_ctrl
    for p in ctrl.parameters():
        p.grad = None
    rec, orig = {}, loss.simulate

    def spy(*a, **k):  # the trajectory the training call integrates
        rec["out"] = orig(*a, **k)
        return rec["out"]
    loss.simulate = spy
    try:
        kw = {k: v for k, v in b["kwargs"].items() if k == "initial_log_prob"}
        value, _ = loss(b["ts"] if ts is None else ts, b["x0"] if x0 is None else x0, *b["args"], **kw)
    finally:
        del loss.simulate
    value.backward()
    return value.detach(), {k: p.grad.clone() for k, p in ctrl.named_parameters() if p.grad is not None}, rec["out"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,split", [(n, False) for n in NAMES] + [(BIG, True)])
def test_perturbed_lv_training_matches_reference(gpu, name, split):
    """Loss value to 1e-5 relative and every gradient to max(5e-5, 10 x the fixture's own sensitivity to a 1.2e-6 move of the normals) --
    the rule of tests/test_gpu_training.py -- against the reference run with the same perturbation draws."""
    c, b = _build(name, gpu, split=split)
    value, grads, _ = _train(b)
    loss_err = abs(float(value) - c.meta["loss"]) / max(1.0, abs(c.meta["loss"]))
    tol = max(5e-5, 10 * c.meta["grad_sensitivity"])
    worst, n = 0.0, 0
    for k, g in grads.items():
        ref = c["grad." + k]
        worst, n = max(worst, float((g.cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)), n + 1
    print(f"{name} split={split}: loss {float(value):.6f} vs {c.meta['loss']:.6f} (rel {loss_err:.1e}); worst relative gradient error {worst:.2e} "
          f"over {n} parameters (tolerance {tol:.1e})")
    assert n == sum(1 for k in c.a if k.startswith("grad.")) and n >= 8
    assert loss_err < 1e-5 and worst < tol


@pytest.mark.gpu
@pytest.mark.parametrize("name,split", [("ctrl_perturb_ei_gmm_d16_noise_dropout", False), ("ctrl_perturb_pis_phi4_d100_noise_dropout", False),
                                        (BIG, False), (BIG, True)])
def test_degenerate_settings_equal_the_unperturbed_path_bit_for_bit(gpu, name, split):
    """sde_ctrl_noise = 0 (u + 0 eps) and sde_ctrl_dropout = 1 (U > 1 never holds: nothing is replaced) run the perturbed kernels and must give
    the unperturbed path's loss, x_N, log-weights and gradients bit for bit -- on the standard and on the split-tile kernel."""
    _, b = _build(name, gpu, split=split, noise=None, dropout=None)
    base = _train(b)
    for noise, dropout in ((0.0, None), (None, 1.0), (0.0, 1.0)):
        b["loss"].sde_ctrl_noise, b["loss"].sde_ctrl_dropout = noise, dropout
        got = _train(b)
        assert torch.equal(got[0], base[0]), (noise, dropout)
        for i in range(3):
            assert torch.equal(got[2][i], base[2][i]), (noise, dropout, i)
        assert got[1].keys() == base[1].keys() and all(torch.equal(got[1][k], base[1][k]) for k in base[1]), (noise, dropout)


@pytest.mark.gpu
@pytest.mark.parametrize("name,split", [("ctrl_perturb_dis_ei_d8_noise_dropout", False), (BIG, False), (BIG, True)])
def test_full_dropout_replaces_every_element(gpu, name, split):
    """sde_ctrl_dropout = 0: U > 0 always, so the control of every step is -(a_k x) / g_k of the loss's SDE -- the trajectory is a host
    recursion of the table's own coefficients (LIN form: x' = c1 x + c2 u + c3 z), to fp32 round-off.  The d = 128 RDS case runs without its
    reference drift here (reference_ctrl = None), so that nothing but the replaced control enters the update."""
    _, b = _build(name, gpu, split=split, noise=None, dropout=0.0)
    loss = b["loss"]
    loss.reference_ctrl = None
    _, _, (x_n, _, xs) = _train(b)
    N, B, d = xs.shape[0] - 1, xs.shape[1], xs.shape[2]
    coef = E.coef_table(loss.kind, b["ts"].cpu(), E._cpu_sde(loss.sde), ctrl_dropout=0.0).to(gpu)
    z = E.philox_noise(loss.seed, N, B, d, loss.particle0, gpu)
    worst = 0.0
    for k in range(N):
        c = coef[k]
        u = -((c[14] * xs[k]) / c[15])
        x = c[1] * xs[k] + c[2] * u + c[3] * z[k]
        worst = max(worst, gc.rel_err(xs[k + 1].cpu(), x.cpu()))
    print(f"{name} split={split}: every control replaced; worst relative state error of the {N} steps against the host recursion {worst:.2e}")
    assert torch.equal(xs[-1], x_n) and worst < 1e-5


def _philox_steps(seed, N, B, d, particle0, stream, device):
    out = torch.empty(N, B, d, dtype=torch.float32, device=device)
    L.check(L.lib().sdeng_philox_normal_steps(int(seed), 0, N, int(particle0), B, d, stream, out.data_ptr(), E._stream_ptr(device)))
    return out


@pytest.mark.gpu
def test_control_noise_counter_layout(gpu):
    """One Euler-Maruyama step from x0 = 0 (PIS, ScaledBM: no drift): x_1 = c2 c4 u~ + c2 c5 z, so (x_1(sigma) - x_1(0)) / (c2 c4 sigma) recovers
    the control noise -- it must be sigma * the Philox normals of stream 4 with the step noise's counter layout (sdeng_philox_normal_steps,
    d = 100: the last feature tile holds 12 pad features), and not those of any other stream."""
    sigma = 0.5
    _, b = _build("ctrl_perturb_pis_phi4_d100_noise_dropout", gpu, noise=0.0, dropout=None)
    ts = b["ts"][:2].contiguous()
    x1 = {}
    for s in (0.0, sigma):
        b["loss"].sde_ctrl_noise = s
        x1[s] = _train(b, ts=ts)[2][0]
    loss = b["loss"]
    c = E.coef_table(loss.kind, ts.cpu(), E._cpu_sde(loss.sde))[0]
    eps = (x1[sigma] - x1[0.0]) / (c[2] * c[4] * sigma)
    B, d = eps.shape
    want = _philox_steps(loss.seed, 1, B, d, loss.particle0, 4, gpu)[0]
    err = float((eps - want).abs().max())
    print(f"control noise recovered from one step: max |eps - philox(stream 4)| = {err:.2e}")
    assert err < 1e-3
    for other in (0, 1, 5):
        assert float((eps - _philox_steps(loss.seed, 1, B, d, loss.particle0, other, gpu)[0]).abs().max()) > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True])
def test_sharded_training_runs_equal_the_unsharded_run(gpu, split):
    """Two shards (particle0 = 0 and B/2) of the d = 128 case: every particle's log-weight and end state bit-equal to the unsharded run's
    -- the perturbation draws are keyed by the global particle index like the step noise."""
    _, b = _build(BIG, gpu, split=split)
    loss = b["loss"]
    _, _, (x_full, rnd_full, _) = _train(b)
    x0, half = b["x0"], b["x0"].shape[0] // 2
    for p0, sl in ((0, slice(0, half)), (half, slice(half, None))):
        loss.particle0 = p0
        _, _, (x_n, rnd, _) = _train(b, x0=x0[sl].contiguous())
        assert torch.equal(x_n, x_full[sl]) and torch.equal(rnd, rnd_full[sl]), p0
    loss.particle0 = 0


@pytest.mark.gpu
def test_kl_methods_still_refuse_the_perturbation(gpu):
    """The options perturb the LV trajectories only; KL training (through the trajectory) keeps refusing them, as does CMCD
    (tests/test_gpu_training.py)."""
    for noise, dropout in ((0.1, None), (None, 0.5)):
        _, b = _build("ctrl_perturb_ei_gmm_d16_noise_dropout", gpu, noise=noise, dropout=dropout)
        for method in ("kl", "kl_ito"):
            b["loss"].method = method
            with pytest.raises(E.UnsupportedByEngine):
                b["loss"](b["ts"], b["x0"], *b["args"])
