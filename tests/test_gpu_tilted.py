"""Energy-based (tilted-potential) references on the GPU: sdeng_tilted_eval against the reference's own float64 run, with the
reference's own float32 run as the yardstick (tests/golden/tilted_*.npz); bit-exact properties; the annealed samplers over an EBM.

err(a) = max over rows of |a - f64|_inf / (1 + |f64|_inf), for log_prob and for grad; required: err(HIP) <= 10 x err(reference float32)
-- the margin split-f16 chains get over the reference's own round-off everywhere in this project (tests/test_gpu_parity.py)."""
import pytest
import torch

from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.additions import ebm_mle
from tests import tilted_cases as tc

pytestmark = pytest.mark.gpu
MARGIN = 10.0
_CACHE = {}


def on_gpu(case, gpu):
    """(fixture, mirror on the GPU, t, x), built once per case."""
    if case not in _CACHE:
        fx, net = tc.mirror(case)
        net = net.to(gpu).requires_grad_(False)
        _CACHE[case] = (fx, net, fx["t"].to(gpu), fx["x"].to(gpu))
    return _CACHE[case]


@pytest.mark.parametrize("case", list(tc.CASES))
def test_parity_with_the_reference(case, gpu):
    fx, net, t, x = on_gpu(case, gpu)
    lp, grad = E.tilted_eval(net, t, x)                    # the C ABI, through the descriptor compiler
    lp_c, grad_c = net.unnorm_log_prob_and_grad(t, x)      # the classes
    ref_lp, ref_grad = tc.err(fx["out.lp32"], fx["out.lp64"]), tc.err(fx["out.grad32"], fx["out.grad64"])
    e_lp, e_grad = tc.err(lp.cpu(), fx["out.lp64"]), tc.err(grad.cpu(), fx["out.grad64"])
    print(f"\ntilted_eval parity case {case}: d={fx.spec['d']} M={x.shape[0]}  log_prob err {e_lp:.3e} (reference float32 {ref_lp:.3e}, ratio "
          f"{e_lp / ref_lp:.2f})  grad err {e_grad:.3e} (reference float32 {ref_grad:.3e}, ratio {e_grad / ref_grad:.2f})")
    assert lp.shape == (x.shape[0],) and grad.shape == x.shape
    assert torch.isfinite(lp).all() and torch.isfinite(grad).all()
    assert e_lp <= MARGIN * ref_lp and e_grad <= MARGIN * ref_grad
    # the classes are the same launch: same bits from every entry point
    assert torch.equal(lp_c, lp) and torch.equal(grad_c, grad)
    assert torch.equal(net(t, x), grad) and torch.equal(net.unnorm_log_prob(t, x), lp) and torch.equal(net.energy(t, x), -lp)


@pytest.mark.parametrize("case", list(tc.CASES))
def test_reruns_layouts_and_outputs_agree_bit_for_bit(case, gpu):
    fx, net, t, x = on_gpu(case, gpu)
    lp, grad = E.tilted_eval(net, t, x)
    again = E.tilted_eval(net, t, x)
    assert torch.equal(again[0], lp) and torch.equal(again[1], grad)
    rows = E.tilted_eval(net, t, x, per_row_times=True)    # the same rows as N = M times of one row
    assert torch.equal(rows[0], lp) and torch.equal(rows[1], grad)
    only_lp = E.tilted_eval(net, t, x, want_grad=False)    # no backward pass
    assert only_lp[1] is None and torch.equal(only_lp[0], lp)
    only_grad = E.tilted_eval(net, t, x, want_logp=False)
    assert only_grad[0] is None and torch.equal(only_grad[1], grad)
    if len(fx.spec["times"]) == 1:                         # a scalar time and a (1, 1) time are the (M, 1) column
        for tt in (float(fx.spec["times"][0]), t[:1]):
            got = E.tilted_eval(net, tt, x)
            assert torch.equal(got[0], lp) and torch.equal(got[1], grad)


def test_zero_last_layer_contributes_exactly_nothing(gpu):
    """Case f, the recipe's initialisation: the output is the prior's, bit for bit -- whatever the hidden layers hold, with and
    without the backward pass."""
    fx, net, t, x = on_gpu("f", gpu)
    lp, grad = E.tilted_eval(net, t, x)
    assert torch.equal(E.tilted_eval(net, t, x, want_grad=False)[0], lp)
    other = tc.build(dict(fx.spec, seed=977), *_mods(), fx.ctor_args()).to(gpu).requires_grad_(False)  # other hidden weights, same prior
    with torch.no_grad():
        other.mean_gauss.copy_(net.mean_gauss)
        other.var_gauss.copy_(net.var_gauss)
        assert float(other.base_model.out_layer.weight.abs().max()) == 0.0
        assert not torch.equal(other.base_model.input_embed.weight, net.base_model.input_embed.weight)
    lp_o, grad_o = E.tilted_eval(other, t, x)
    assert torch.equal(lp_o, lp) and torch.equal(grad_o, grad)
    assert tc.err(lp.cpu(), fx["out.lp64"]) <= MARGIN * tc.err(fx["out.lp32"], fx["out.lp64"])


def _mods():
    from sde_sampler_lrds_amd.eq import sdes
    from sde_sampler_lrds_amd.models import mlp, reparam
    return mlp, reparam, sdes


def test_packed_images_follow_the_parameters(gpu):
    """The images are cached per parameter version: an in-place edit of a weight is seen by the next call."""
    fx, net = tc.mirror("a")
    net = net.to(gpu).requires_grad_(False)
    t, x = fx["t"].to(gpu), fx["x"].to(gpu)
    lp0, _ = E.tilted_eval(net, t, x)
    with torch.no_grad():
        net.base_model.out_layer.weight.mul_(2.0)
    lp1, _ = E.tilted_eval(net, t, x)
    assert not torch.equal(lp0, lp1)
    with torch.no_grad():
        net.base_model.out_layer.weight.mul_(0.5)
    assert torch.equal(E.tilted_eval(net, t, x)[0], lp0)


# ---- the annealed samplers over an EBM ----------------------------------------------------------------------------------------------
def autograd_closure(net):
    """Test-side torch composition of the same arithmetic over the same weights (float32 on the GPU, autograd for the gradient): what a
    user had before the kernel.  Diagonal mixtures only (case a's net)."""
    def fn(t, x):
        with torch.enable_grad():
            x = x.detach().requires_grad_(True)
            t = t.reshape(-1, 1).expand(x.shape[0], 1).to(x.dtype)
            s, sig = net.sde.s(t), net.sde.sigma_sq(t)
            xs = (x - s * net.mean_gauss) / (s * torch.sqrt(net.var_gauss + sig))
            base = -(net.base_model(t, xs) * xs).sum(-1)
            tl = torch.maximum(t, net.t_limit * torch.ones_like(t))
            sl, sigl = net.sde.s(tl), net.sde.sigma_sq(tl)
            var = (sl ** 2 * sigl).unsqueeze(1) + (sl ** 2).unsqueeze(1) * net.variances.unsqueeze(0)
            z = x.unsqueeze(1) - sl.unsqueeze(1) * net.means.unsqueeze(0)
            lps = torch.log(net.weights / net.weights.sum()) - 0.5 * (x.shape[1] * 1.8378770664093453 + torch.log(var).sum(-1) + (z * z / var).sum(-1))
            lp = torch.logsumexp(lps, dim=-1) + (s.flatten() if net.use_s_t_scaling else 1.0) * base
            grad = torch.autograd.grad(lp.sum(), x)[0]
        return lp.detach(), grad
    return fn


class Margins:
    """|min(1, acceptance ratio) - u| of every accept / reject and swap decision of a sampler run, by replaying torch's generator around
    the moves (the closure draws nothing)."""

    def __init__(self, monkeypatch, device):
        self.values, self.device = [], device
        mala, swap = ebm_mle.mala_step, ebm_mle.re_step

        def mala_step(y, lp, g, f, step):
            before = torch.cuda.get_rng_state(device)
            out = mala(y, lp, g, f, step)
            after = torch.cuda.get_rng_state(device)
            torch.cuda.set_rng_state(before, device)
            torch.randn(y.shape, device=device)
            self.note(out[-1], torch.rand_like(out[-1]))
            torch.cuda.set_rng_state(after, device)
            return out

        def re_step(x, lp_x, g_x, f, times, i, j, *rest):
            log_acc = (f(times[i], x[j])[0] + f(times[j], x[i])[0]) - (lp_x[i] + lp_x[j])
            before = torch.cuda.get_rng_state(device)
            self.note(log_acc, torch.rand_like(log_acc))
            torch.cuda.set_rng_state(before, device)
            return swap(x, lp_x, g_x, f, times, i, j, *rest)
        monkeypatch.setattr(ebm_mle, "mala_step", mala_step)
        monkeypatch.setattr(ebm_mle, "re_step", re_step)

    def note(self, log_acc, u):
        self.values.append(float((torch.exp(log_acc).clamp(max=1.0) - u).abs().min()))


SAMPLER_SEED = {"re": 7, "smc": 3}  # closest decisions of these runs: 2.5e-2 from a tie (seeds 0 .. 7 measured, profiles/tilted_eval_parity.log; re 4 and 6 and smc 5 come within 1e-3)
LEVELS, CHAINS, WARM, KEEP = 3, 8, 2, 4


def run_sampler(kind, fn, net, gpu, seed):
    g = torch.Generator().manual_seed(611)
    times = torch.tensor([0.2, 0.5, 0.8], device=gpu).view(-1, 1, 1).repeat(1, CHAINS, 1)
    x_init = (net.mean_gauss.cpu() + net.var_gauss.cpu().sqrt() * torch.randn(CHAINS, net.dim, generator=g)).to(gpu)
    steps = 0.02 * torch.ones(LEVELS, CHAINS, 1, device=gpu)
    torch.manual_seed(seed)
    if kind == "re":
        return ebm_mle.re_sampler(x_init, times, fn, 3, WARM, KEEP, steps)[0]
    return ebm_mle.smc_sampler(x_init, times, fn, WARM, KEEP, steps, reweight_threshold=1.0)[0]


@pytest.mark.parametrize("kind", ["re", "smc"])
def test_samplers_over_an_ebm_match_the_autograd_closure(kind, gpu, monkeypatch):
    """re_sampler / smc_sampler with ebm_log_prob_and_grads(net) (3 levels x 8 chains, d = 2, six moves) against the same samplers
    driven by the autograd closure, under the same seed of torch's generator.

    Seed: torch's CUDA generator cannot be replayed on the CPU, so the seed is held to its condition HERE, on the autograd run: no
    decision of the run has min(1, ratio) within 1e-3 of its uniform draw (``Margins``).  Both closures then take the same decisions,
    which the tolerance below enforces: a flipped decision moves a chain by O(sqrt(2 step)) = 0.2.
    Tolerance: per call both closures are within e = 10 x the reference's float32 error of the float64 value (the parity test's bound;
    measured ratios are about 1): e_grad = 10 x 1.7e-7 relative to 1 + |grad|.  A move maps an error dg of the gradient to step dg =
    0.02 dg of the state and passes a state error on times at most 1 + step L.  Generous figures for these chains: |grad| <= 30
    (measured: about 3) and L <= 40 (the sharpest noised component has variance above 0.1), i.e. 1.8 per move and 1.8^6 = 34 over the
    six moves.  Bound: 6 moves x 34 x 0.02 x 2 e_grad x 31 = 4.3e-4; the test asserts 5e-4 and prints what it measured (2e-7 to 5e-7)."""
    fx, net = tc.mirror("a")
    net = net.to(gpu).requires_grad_(False)
    margins = Margins(monkeypatch, gpu)
    want = run_sampler(kind, autograd_closure(net), net, gpu, SAMPLER_SEED[kind])
    n_decisions, closest = len(margins.values), min(margins.values)
    got = run_sampler(kind, ebm_mle.ebm_log_prob_and_grads(net), net, gpu, SAMPLER_SEED[kind])
    diff = float((got - want).abs().max())
    print(f"\n{kind}_sampler over an EBM: {n_decisions} decision batches, closest |min(1, ratio) - u| = {closest:.2e}; max |chain difference| = {diff:.2e}")
    assert got.shape == (LEVELS, KEEP, CHAINS, 2) and torch.isfinite(got).all()
    assert closest > 1e-3, "choose another SAMPLER_SEED: a decision of this run is a near tie"
    assert diff < 5e-4
