"""Training an energy-based reference on the GPU: sdeng_tilted_vjp and the autograd.Function behind net.energy against the reference's
own float64 parameter gradients, with the reference's own float32 run as the yardstick (tests/golden/tilted_train_*.npz); bit-exact
properties of the per-row arrays; the MaximumLikelihoodEBM trainer.

Per parameter tensor err_p(g) = |g - g64|_inf / |g64|_inf; required: err_p(HIP) <= 10 x max(err_p(reference float32), 2^-23) -- the
margin split-f16 chains get over the reference's own round-off everywhere in this project (MARGIN of tests/test_gpu_tilted.py), with the
output format's rounding as the floor."""
import copy

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.additions import ebm_mle
from tests import tilted_cases as tc
from tests import tilted_train_ref as tr

pytestmark = pytest.mark.gpu
MARGIN = 10.0
FLOOR = 2.0 ** -23
_CACHE = {}


def on_gpu(case, gpu):
    """(training fixture, trainable mirror on the GPU with param_grads on, t, x), built once per case; tests leave it unchanged."""
    if case not in _CACHE:
        fx, net = tc.mirror(case)
        net = net.to(gpu)
        net.param_grads = True
        _CACHE[case] = (tr.TrainFixture(case), net, fx["t"].to(gpu), fx["x"].to(gpu))
    return _CACHE[case]


def bound(err32):
    return MARGIN * max(err32, FLOOR)


@pytest.mark.parametrize("case", tr.CASES)
def test_parameter_gradients_match_the_reference(case, gpu):
    fx, net, t, x = on_gpu(case, gpu)
    net.zero_grad()
    en = net.energy(t, x)
    assert en.shape == (x.shape[0],) and en.requires_grad
    tr.loss_of(en, fx.w.to(gpu)).backward()
    with torch.no_grad():
        lp = E.tilted_eval(net, t, x, want_grad=False)[0]
    e_en, ref_lp = tc.err(-en.detach().cpu(), fx.base["out.lp64"]), tc.err(fx.base["out.lp32"], fx.base["out.lp64"])
    print(f"\ntilted_vjp parity case {case}: d={fx.base.spec['d']} M={x.shape[0]}  energy err {e_en:.3e} (bound {MARGIN * ref_lp:.3e}); "
          f"bit-equal to -tilted_eval: {torch.equal(en.detach(), -lp)}")
    assert e_en <= MARGIN * ref_lp
    failures = []
    for name, p in net.named_parameters():
        want = fx.grads[name]
        assert p.grad is not None and p.grad.shape == want.shape and torch.isfinite(p.grad).all(), name
        got, lim = tr.tensor_err(p.grad, want), bound(fx.err32[name])
        print(f"  {name:50s} err {got:.3e}  bound {lim:.3e}  (reference float32 {fx.err32[name]:.3e})")
        if float(want.abs().max()) == 0.0:  # case f below the zero last layer: exactly nothing
            assert float(p.grad.abs().max()) == 0.0, name
        if got > lim:
            failures.append((name, got, lim))
    net.zero_grad()
    assert not failures, failures


@pytest.mark.parametrize("case", tr.CASES)
def test_reruns_and_layouts_agree_bit_for_bit(case, gpu):
    fx, net, t, x = on_gpu(case, gpu)

    def flat(out):
        lp, grad, arrays, _ = out
        return [lp, grad, arrays["xs"], arrays["dv"], *arrays["a"], *arrays["d"]]
    first = flat(E.tilted_vjp(net, t, x, want_grad=True))
    for other in (E.tilted_vjp(net, t, x, want_grad=True), E.tilted_vjp(net, t, x, want_grad=True, per_row_times=True)):
        assert all(torch.equal(u, v) for u, v in zip(first, flat(other)))
    assert all(torch.isfinite(u).all() for u in first)
    no_score = E.tilted_vjp(net, t, x)  # the score is optional: the arrays do not depend on it
    assert no_score[1] is None and all(torch.equal(u, v) for u, v in zip(first[2:], flat(no_score)[2:])) and torch.equal(no_score[0], first[0])
    with torch.no_grad():
        lp, grad = E.tilted_eval(net, t, x)
    assert torch.equal(first[1], grad)
    print(f"\ntilted_vjp case {case}: log_prob bit-equal to tilted_eval: {torch.equal(first[0], lp)}")
    # the parameter gradients go through library GEMMs: report, do not require bits
    grads = []
    for _ in range(2):
        net.zero_grad()
        net.energy(t, x).sum().backward()
        grads.append([p.grad.clone() for p in net.parameters()])
    net.zero_grad()
    print(f"  parameter gradients, rerun: max |difference| = {max(float((u - v).abs().max()) for u, v in zip(*grads)):.3e}")


def test_more_than_one_wave_per_workgroup(gpu):
    """Two times x 4 100 rows = 513 tiles: two waves per workgroup (sd_tilted_waves), tiles straddling the time boundary.  The per-row
    arrays equal, bit for bit, those of the same rows evaluated in two one-time calls (257 tiles each: one wave per workgroup)."""
    _, net, _, _ = on_gpu("a", gpu)
    rows, g = 4100, torch.Generator().manual_seed(977)
    times = torch.tensor([0.25, 0.75])
    t = times.repeat_interleave(rows).reshape(-1, 1)
    s, sig = net.sde.s(t.to(gpu)).cpu(), net.sde.sigma_sq(t.to(gpu)).cpu()
    x = (s * net.mean_gauss.cpu() + s * torch.sqrt(net.var_gauss.cpu() + sig) * torch.randn(2 * rows, 2, generator=g)).to(gpu)
    t = t.to(gpu)
    lp, grad, arrays, (N, B, tu) = E.tilted_vjp(net, t, x, want_grad=True)
    assert (N, B) == (2, rows) and torch.equal(tu.cpu(), times)
    for i in range(2):
        sl = slice(i * rows, (i + 1) * rows)
        lp_i, grad_i, arr_i, (n_i, b_i, _) = E.tilted_vjp(net, t[sl], x[sl].contiguous(), want_grad=True)
        assert (n_i, b_i) == (1, rows)
        assert torch.equal(lp[sl], lp_i) and torch.equal(grad[sl], grad_i)
        assert torch.equal(arrays["xs"][sl], arr_i["xs"]) and torch.equal(arrays["dv"][sl], arr_i["dv"])
        for l in range(5):
            assert torch.equal(arrays["a"][l][sl], arr_i["a"][l]) and torch.equal(arrays["d"][l][sl], arr_i["d"][l]), l
    assert all(torch.isfinite(v).all() for v in (lp, grad, *arrays["a"], *arrays["d"]))


def test_gradient_with_respect_to_x_is_the_score_of_the_same_launch(gpu):
    _, net, t, x = on_gpu("b", gpu)
    xg = x.clone().requires_grad_(True)
    en = net.energy(t, xg)
    (gx,) = torch.autograd.grad(en.sum(), xg)
    with torch.no_grad():
        lp, score = E.tilted_eval(net, t, x)
    assert torch.equal(gx, -score) and torch.equal(en.detach(), -lp)
    lp_graph = net.unnorm_log_prob(t, xg)
    (gl,) = torch.autograd.grad(lp_graph.sum(), xg)
    assert torch.equal(gl, score) and torch.equal(lp_graph.detach(), lp)


def test_retain_graph_and_stale_parameters(gpu):
    _, net, t, x = on_gpu("a", gpu)
    net.zero_grad()
    loss = torch.square(net.energy(t, x)).sum()
    loss.backward(retain_graph=True)
    once = [p.grad.clone() for p in net.parameters()]
    loss.backward(retain_graph=True)
    worst = max(float((p.grad - 2.0 * g).abs().max() / g.abs().max()) for p, g in zip(net.parameters(), once))
    print(f"\nsecond backward over a retained graph: max |grad - 2 x first| / |first|_inf = {worst:.3e}")
    assert worst <= 4.0 * FLOOR  # the same products twice, up to the reduction order of the library GEMMs
    net.zero_grad()
    en = net.energy(t, x)
    bias = net.base_model.out_layer.bias
    with torch.no_grad():
        bias.add_(0.0)  # same values, newer version
    with pytest.raises(RuntimeError, match="modified in place"):
        en.sum().backward()
    assert all(p.grad is None for p in net.parameters())


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
def torch_energy(net, t, x):
    """Test-side float32 torch composition of net.energy over the same weights, differentiable with respect to the parameters: what a
    user had before the kernel (the arithmetic of ``autograd_closure`` in tests/test_gpu_tilted.py).  Diagonal mixtures (case a's net)."""
    t = t.reshape(-1, 1).expand(x.shape[0], 1).to(x.dtype)
    s, sig = net.sde.s(t), net.sde.sigma_sq(t)
    xs = (x - s * net.mean_gauss) / (s * torch.sqrt(net.var_gauss + sig))
    base = -(net.base_model(t, xs) * xs).sum(-1)
    tl = torch.maximum(t, net.t_limit * torch.ones_like(t))
    sl, sigl = net.sde.s(tl), net.sde.sigma_sq(tl)
    var = (sl ** 2 * sigl).unsqueeze(1) + (sl ** 2).unsqueeze(1) * net.variances.unsqueeze(0)
    z = x.unsqueeze(1) - sl.unsqueeze(1) * net.means.unsqueeze(0)
    lps = torch.log(net.weights / net.weights.sum()) - 0.5 * (x.shape[1] * 1.8378770664093453 + torch.log(var).sum(-1) + (z * z / var).sum(-1))
    return -(torch.logsumexp(lps, dim=-1) + (s.flatten() if net.use_s_t_scaling else 1.0) * base)


def make_trainer(gpu, sampler_type, **kw):
    from sde_sampler_lrds_amd.distr.gauss import Gauss
    _, net = tc.mirror("a")
    mle = ebm_mle.MaximumLikelihoodEBM(net.sde, Gauss(dim=2, loc=0.0, scale=1.0), net, sampler_type, step_sizes_per_noise=0.01,
                                       start_eps=0.05, end_eps=0.1, n_steps=2, **kw).to(gpu)
    return mle, mle.net


class Spy:
    """Records the arguments of every net.energy call and counts the sdeng_tilted_vjp launches."""

    def __init__(self, monkeypatch, net):
        self.calls, self.launches = [], 0
        energy, launch = net.energy, L.lib().sdeng_tilted_vjp

        def spy_energy(t, x, **kw):
            self.calls.append((t.detach().clone(), x.detach().clone()))
            return energy(t, x, **kw)

        def spy_launch(*a):
            self.launches += 1
            return launch(*a)
        monkeypatch.setattr(net, "energy", spy_energy)
        monkeypatch.setattr(L.lib(), "sdeng_tilted_vjp", spy_launch)


REG = 0.05


def test_trainer_first_step(gpu, monkeypatch):
    """One batch (3 levels x 8 rows, negatives from sample_prior: no MCMC has run): the gradients the optimizer sees and losses[0]
    against the float64 restatement on the very rows the trainer drew, with a float32 torch-autograd run on the GPU as the yardstick."""
    mle, net = make_trainer(gpu, "annealed_mcmc", use_ula=True)
    before = copy.deepcopy(net)
    spy, seen = Spy(monkeypatch, net), []
    step = torch.optim.Adam.step

    def spy_step(self, *a, **kw):
        seen.append({id(p): p.grad.clone() for group in self.param_groups for p in group["params"]})
        return step(self, *a, **kw)
    monkeypatch.setattr(torch.optim.Adam, "step", spy_step)
    data = 0.5 * torch.randn(8, 2, generator=torch.Generator().manual_seed(31)).to(gpu)
    torch.manual_seed(5)
    losses, diagnostics = mle.train(data, 8, 1, clip_val=0.0, reg_val=REG, verbose=False, lr=1e-4)
    assert losses.shape == (1,) and diagnostics == [] and len(seen) == 1 and len(spy.calls) == 2 and spy.launches == 2
    (ts, xs_pos), (ts_neg, xs_neg) = spy.calls
    assert ts.shape == (24, 1) and xs_pos.shape == xs_neg.shape == (24, 2) and torch.equal(ts, ts_neg)
    M = 24
    # truth: the float64 restatement on those rows; L = mean(E+ - E-) + reg (mean(E+^2) + mean(E-^2))
    e_pos, g_pos = tr.restated_param_grads("a", ts.cpu(), xs_pos.cpu(), lambda en: 1.0 / M + 2.0 * REG * en / M)
    e_neg, g_neg = tr.restated_param_grads("a", ts.cpu(), xs_neg.cpu(), lambda en: -1.0 / M + 2.0 * REG * en / M)
    loss64 = float((e_pos - e_neg).mean() + REG * (torch.square(e_pos).mean() + torch.square(e_neg).mean()))
    # yardstick: float32 autograd over the same weights on the GPU
    en_p, en_n = torch_energy(before, ts, xs_pos), torch_energy(before, ts, xs_neg)
    loss32 = (en_p - en_n).mean() + REG * (torch.square(en_p).mean() + torch.square(en_n).mean())
    names = [n for n, _ in before.named_parameters()]
    g32 = dict(zip(names, torch.autograd.grad(loss32, list(before.parameters()))))
    err_l, err_l32 = abs(float(losses[0]) - loss64) / abs(loss64), abs(float(loss32.detach()) - loss64) / abs(loss64)
    print(f"\ntrainer first step: loss {float(losses[0]):.7f} (float64 {loss64:.7f}) err {err_l:.3e}  bound {bound(err_l32):.3e}")
    failures = [] if err_l <= bound(err_l32) else [("loss", err_l, bound(err_l32))]
    for name, p in net.named_parameters():
        want = g_pos[name] + g_neg[name]
        got, lim = tr.tensor_err(seen[0][id(p)], want), bound(tr.tensor_err(g32[name], want))
        print(f"  {name:50s} err {got:.3e}  bound {lim:.3e}")
        if got > lim:
            failures.append((name, got, lim))
    assert not failures, failures
    assert net.param_grads is False


@pytest.mark.parametrize("sampler_type,kw,acc", [("annealed_mcmc", dict(use_ula=True), 2), ("replica_exchange", dict(swap_frequency=2), 2),
                                                 ("cd", {}, 1)])
def test_trainer_runs(sampler_type, kw, acc, gpu, monkeypatch):
    mle, net = make_trainer(gpu, sampler_type, **kw)
    before = [p.detach().clone() for p in net.parameters()]
    spy = Spy(monkeypatch, net)
    data = 0.5 * torch.randn(32, 2, generator=torch.Generator().manual_seed(32)).to(gpu)
    torch.manual_seed(6)
    losses, norms, diagnostics = mle.train(data, 8, 2, initial_n_warmup_mcmc_steps=3, n_mcmc_steps=3, n_accumulation_steps=acc, reg_val=REG,
                                           use_ema=True, ema_steps=1, verbose=False, lr=1e-3)
    n_batches, fresh = 8, 8 // acc
    assert losses.shape == norms.shape == (n_batches,) and torch.isfinite(losses).all() and torch.isfinite(norms).all()
    assert len(diagnostics) == fresh - 1  # the very first negatives are sample_prior's
    assert len(spy.calls) == n_batches + fresh and spy.launches == len(spy.calls)  # one launch per energy call
    assert all(not torch.equal(p, q) and torch.isfinite(p).all() for p, q in zip(net.parameters(), before))
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in net.parameters())
    steps = mle.step_sizes_per_noise
    assert steps.numel() == 3 * 8 and torch.isfinite(steps).all() and bool((steps > 0).all())
    if sampler_type == "annealed_mcmc":
        assert steps.shape == (3, 8, 1)
    assert net.param_grads is False and hasattr(mle, "ema_net") and mle.ema_net.module.param_grads is False
    assert all(p.requires_grad for p in net.parameters())
