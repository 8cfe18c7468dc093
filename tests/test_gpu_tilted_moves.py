"""All Langevin moves of a sampler level over an energy-based reference in one launch (sdeng_tilted_moves, k_tilted_moves) on the GPU:
against the host composition it replaces (mala_step / ula_step / heuristics_step_size over E.tilted_eval), the self-consistency of the
state it carries, bit-exact properties, the launch geometries, the Philox streams, and the samplers and the trainer that run through it."""
import ctypes
import math

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.additions import ebm_mle
from sde_sampler_lrds_amd.additions.mcmc import heuristics_step_size, mala_step, ula_step
from tests import tilted_cases as tc
from tests.test_gpu_tilted import KEEP, LEVELS, CHAINS, MARGIN, SAMPLER_SEED, _mods, on_gpu, run_sampler

pytestmark = pytest.mark.gpu
STEP, TARGET = 0.02, 0.75
EPS = 2.0 ** -24  # unit round-off of float32
_START = {}


def start(case, gpu):
    """(fixture, net, t, x, lp, grad) of a case, the last two from E.tilted_eval: computed once, never written to (the tests clone)."""
    if case not in _START:
        fx, net, t, x = on_gpu(case, gpu)
        _START[case] = (fx, net, t, x) + tuple(E.tilted_eval(net, t, x))
    return _START[case]


def moves(net, t, x, lp, grad, n_moves, step=None, **kw):
    """E.tilted_moves on clones -> dict of everything it returns or updates."""
    s = dict(x=x.clone(), lp=lp.clone(), grad=grad.clone(), step=torch.full((x.shape[0],), STEP, device=x.device) if step is None else step.clone())
    s["samples"], s["acc_sum"], s["acc_last"] = E.tilted_moves(net, t, s["x"], s["lp"], s["grad"], s["step"], n_moves, **kw)
    return s


def same(a, b, keys=("x", "lp", "grad", "step", "samples", "acc_sum", "acc_last")):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in keys)


def host_moves(net, t, x, lp, grad, n_moves, unadjusted=False):
    """Today's path: n_moves times mala_step (ula_step) and heuristics_step_size over E.tilted_eval, drawing from torch's generator.
    Returns the state, the steps, and per move the proposals' ingredients (z, u, log_acc) replayed from the generator."""
    f = lambda y: E.tilted_eval(net, t, y)  # noqa: E731
    x, lp, grad = x.clone(), lp.clone(), grad.clone()
    step = torch.full((x.shape[0], 1), STEP, device=x.device)
    trace = []
    for _ in range(n_moves):
        before = torch.cuda.get_rng_state(x.device)
        x0, g0, s0 = x.clone(), grad.clone(), step.clone()
        if unadjusted:
            x, lp, grad = ula_step(x, lp, grad, f, step)
            log_acc = None
        else:
            x, lp, grad, log_acc = mala_step(x, lp, grad, f, step)
            step = heuristics_step_size(step, log_acc, target_acceptance=TARGET)
        after = torch.cuda.get_rng_state(x.device)
        torch.cuda.set_rng_state(before, x.device)
        z = torch.randn(x.shape, device=x.device)
        u = None if unadjusted else torch.rand((x.shape[0],), device=x.device)
        torch.cuda.set_rng_state(after, x.device)
        trace.append(dict(x0=x0, g0=g0, s0=s0, z=z, u=u, log_acc=log_acc))
    return dict(x=x, lp=lp, grad=grad, step=step.flatten()), trace


def proposal_bound(tr):
    """|difference| allowed between two float32 evaluations of prop = sd z + (x + h g), sd = sqrt(2 h), that differ in which of the two
    multiply-adds are fused (see test_one_move_against_the_host_composition), elementwise, computed in float64."""
    x, g, z, h = tr["x0"].double(), tr["g0"].double(), tr["z"].double(), tr["s0"].double()
    sd = torch.sqrt(2.0 * tr["s0"]).double()  # the float32 square root both sides take
    return 2.0 * EPS * ((sd * z).abs() + (h * g).abs() + (x + h * g).abs() + (sd * z + x + h * g).abs())


MOVE_SEED = 0  # closest decision of the yardstick run over the five cases: 3.7e-3 from its uniform (case d; a 2.8e-2, b 2.8e-2, c 1.8e-2, e 1.8e-2)


@pytest.mark.parametrize("unadjusted", [False, True], ids=["mala", "ula"])
@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_one_move_against_the_host_composition(case, unadjusted, gpu):
    """One move, noise from torch's generator under MOVE_SEED, against mala_step (ula_step) + heuristics_step_size over E.tilted_eval run
    here under the same seed.  The seed is held to the condition of tests/test_gpu_tilted.py's ``Margins`` on the yardstick run: no
    decision has min(1, ratio) within 1e-3 of its uniform.  Required: the same accept decisions, steps equal up to one float32 rounding,
    and proposals within the bound below (the unadjusted move shows every proposal, the adjusted one those it accepted).

    Proposal bound.  prop = sd z + (x + h g) is two products and two sums; each side may fuse either product into the sum that follows.
    Unfused, with a = h g, b = sd z and |d_i| <= eps = 2^-24:  prop_u = (b (1 + d1) + (x + a (1 + d2)) (1 + d3)) (1 + d4), so
    |prop_u - exact| <= eps (|b| + |a| + |x + a| + |exact|) to first order; fully fused drops the first two terms.  Any two variants
    therefore differ by at most 2 eps (|b| + |a| + |x + a| + |prop|): a few ulp of the largest term.  (Measured: 0 -- this build
    compiles the kernel without contraction, so both sides round alike.)"""
    fx, net, t, x, lp, grad = start(case, gpu)
    torch.manual_seed(MOVE_SEED)
    want, (tr,) = host_moves(net, t, x, lp, grad, 1, unadjusted)
    torch.manual_seed(MOVE_SEED)
    got = moves(net, t, x, lp, grad, 1, unadjusted=unadjusted, target_acceptance=TARGET)
    moved_w, moved_g = (want["x"] != x).any(1), (got["x"] != x).any(1)
    excess = float(((got["x"] - want["x"]).abs().double() - proposal_bound(tr))[moved_w].max()) if bool(moved_w.any()) else 0.0
    d_step = float(((got["step"] - want["step"]).abs() / want["step"]).max())
    if unadjusted:
        closest = float("nan")
        assert got["acc_sum"] is None and got["acc_last"] is None and bool(moved_g.all())
    else:
        closest = float((torch.exp(tr["log_acc"]).clamp(max=1.0) - tr["u"]).abs().min())
        assert closest > 1e-3, "choose another MOVE_SEED: a decision of the yardstick run is a near tie"
        assert torch.allclose(got["acc_last"], torch.exp(tr["log_acc"].clamp(max=0.0)), rtol=1e-4, atol=1e-6)
    print(f"\ntilted_moves one move, case {case} {'ula' if unadjusted else 'mala'}: M={x.shape[0]} d={x.shape[1]} accepted {int(moved_g.sum())}, closest "
          f"|min(1, ratio) - u| = {closest:.2e}; proposals: max |diff| - bound = {excess:.2e}; max rel. step diff {d_step:.2e}; "
          f"acc_last mean {float(got['acc_last'].mean()) if not unadjusted else float('nan'):.4f}")
    assert torch.equal(moved_g, moved_w)                      # identical accept decisions
    assert excess <= 0.0                                      # proposals
    assert d_step <= 2.0 * EPS                                # one rounding of the step
    assert torch.equal(got["samples"][0], got["x"])
    # the carried log-density and score are the evaluation's at the (same, up to the bound above) proposal: each side within MARGIN x the
    # case's reference-float32 error of float64
    assert tc.err(got["lp"].cpu(), want["lp"].cpu().double()) <= 2 * MARGIN * fx.meta["err32_lp"]
    assert tc.err(got["grad"].cpu(), want["grad"].cpu().double()) <= 2 * MARGIN * fx.meta["err32_grad"]


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_carried_state_is_the_evaluation_at_the_final_state(case, gpu):
    """After K = 4 moves the lp / grad that come out against E.tilted_eval at the very same x_out, in tilted_cases.err; bound: 2 x MARGIN x
    the case's stored reference-float32 error (each side is held to MARGIN x that error against float64 by the parity test).  The two
    kernels call the same walk (csrc/tilted_kernel.hpp), so they also agree bit for bit."""
    fx, net, t, x, lp, grad = start(case, gpu)
    torch.manual_seed(11)
    got = moves(net, t, x, lp, grad, 4, target_acceptance=TARGET)
    lp_e, grad_e = E.tilted_eval(net, t, got["x"])
    e_lp, e_grad = tc.err(got["lp"].cpu(), lp_e.cpu().double()), tc.err(got["grad"].cpu(), grad_e.cpu().double())
    b_lp, b_grad = 2 * MARGIN * fx.meta["err32_lp"], 2 * MARGIN * fx.meta["err32_grad"]
    print(f"\ntilted_moves carried state, case {case}: log_prob err {e_lp:.3e} (bound {b_lp:.3e}, ratio {e_lp / b_lp:.3f})  grad err {e_grad:.3e} "
          f"(bound {b_grad:.3e}, ratio {e_grad / b_grad:.3f})  bit-equal: {torch.equal(got['lp'], lp_e) and torch.equal(got['grad'], grad_e)}")
    assert torch.isfinite(got["x"]).all() and not torch.equal(got["x"], x)
    assert e_lp <= b_lp and e_grad <= b_grad
    assert torch.equal(got["lp"], lp_e) and torch.equal(got["grad"], grad_e)


@pytest.mark.parametrize("prior", tc.WALK_PRIORS)
@pytest.mark.parametrize("nt", range(1, 9))
def test_every_instance_carries_the_evaluation_bit_for_bit(nt, prior, gpu):
    """tilted_cases.walk_spec: every k_tilted_moves<NT> and k_tilted_eval<NT> instance over a diagonal and an eigen-form prior, at a d whose
    last quad is partly pad, on three tiles that straddle the times (15 pad rows).  Four MALA moves with injected (z, u): the state stays
    finite and moves, and the lp / grad carried out are E.tilted_eval at the final x bit for bit -- the move kernel and the evaluation
    call one walk -- as is the log-density-only evaluation (no backward pass)."""
    spec = tc.walk_spec(nt, prior)
    net = tc.build(spec, *_mods())
    t, x = tc.draw_inputs(spec, net)
    net, t, x = net.to(gpu).requires_grad_(False), t.to(gpu), x.to(gpu)
    assert x.shape == (33, 16 * nt - 3)
    lp, grad = E.tilted_eval(net, t, x)
    g = torch.Generator().manual_seed(700 + nt)
    z, u = torch.randn(4, *x.shape, generator=g).to(gpu), torch.rand(4, x.shape[0], generator=g).to(gpu)
    got = moves(net, t, x, lp, grad, 4, target_acceptance=TARGET, noise=(z, u))
    lp_e, grad_e = E.tilted_eval(net, t, got["x"])
    print(f"\ntilted_moves walk NT={nt} {prior}: d={x.shape[1]} rows moved {int((got['x'] != x).any(1).sum())} of {x.shape[0]}; carried state "
          f"bit-equal to the evaluation: lp {torch.equal(got['lp'], lp_e)} grad {torch.equal(got['grad'], grad_e)}")
    assert all(torch.isfinite(got[k]).all() for k in ("x", "lp", "grad")) and not torch.equal(got["x"], x)
    assert torch.equal(got["lp"], lp_e) and torch.equal(got["grad"], grad_e)
    assert torch.equal(E.tilted_eval(net, t, got["x"], want_grad=False)[0], lp_e)


@pytest.mark.parametrize("case", ["a", "c"])
def test_bit_exact_properties_with_injected_noise(case, gpu):
    fx, net, t, x, lp, grad = start(case, gpu)
    K, K1 = 5, 2
    run = lambda n, **kw: moves(net, t, x, lp, grad, n, target_acceptance=TARGET, **kw)  # noqa: E731
    torch.manual_seed(21)
    one = run(K)
    torch.manual_seed(21)
    assert same(one, run(K))                                  # two launches on the same inputs, every output
    torch.manual_seed(21)                                     # K moves = K1 + K2 moves over the matching slices of the noise
    first = run(K1)
    second = moves(net, t, first["x"], first["lp"], first["grad"], K - K1, step=first["step"], target_acceptance=TARGET)
    assert same(one, second, ("x", "lp", "grad", "step", "acc_last"))
    assert torch.equal(one["samples"], torch.cat([first["samples"], second["samples"]]))
    torch.manual_seed(21)                                     # keep_from only changes what is stored
    late = run(K, keep_from=3)
    assert same(one, late, ("x", "lp", "grad", "step", "acc_last")) and torch.equal(late["samples"], one["samples"][3:])
    torch.manual_seed(21)
    last_only = run(K, keep_from=K - 1)                       # one kept move: its acceptance is the sum
    assert torch.equal(last_only["acc_sum"], one["acc_last"]) and bool((late["acc_sum"] <= one["acc_sum"]).all())
    torch.manual_seed(21)                                     # no samples: nothing else changes
    bare = run(K, want_samples=False)
    assert bare["samples"] is None and same(one, bare, ("x", "lp", "grad", "step", "acc_sum", "acc_last"))
    torch.manual_seed(21)                                     # the unadjusted move has no acceptance outputs; fixed steps stay fixed
    fixed = moves(net, t, x, lp, grad, K, target_acceptance=0.0)
    assert torch.equal(fixed["step"], torch.full_like(fixed["step"], STEP))


@pytest.mark.parametrize("case,split", [("b", 16), ("b", 32), ("c", 64)])
def test_rows_split_at_a_tile_boundary_equal_the_one_launch(case, split, gpu):
    """The rows of a batch in two launches, split at a multiple of 16, equal the one launch -- with the noise injected (the two launches
    get the matching rows of the same normals and uniforms) and with Philox (chain0 = the first row of each part).  An unaligned split
    regroups the rows into other tiles; that is printed, not asserted."""
    fx, net, t, x, lp, grad = start(case, gpu)
    M, d, K = x.shape[0], x.shape[1], 3
    g = torch.Generator().manual_seed(31)
    z, u = torch.randn(K, M, d, generator=g).to(gpu), torch.rand(K, M, generator=g).to(gpu)

    def parts(cut, philox):
        out = []
        for lo, hi in ((0, cut), (cut, M)):
            noise = "philox" if philox else (z[:, lo:hi].contiguous(), u[:, lo:hi].contiguous())
            out.append(moves(net, t[lo:hi].contiguous(), x[lo:hi], lp[lo:hi], grad[lo:hi], K, target_acceptance=TARGET, noise=noise, seed=77, chain0=lo))
        return {k: torch.cat([out[0][k], out[1][k]], dim=1 if k == "samples" else 0) for k in out[0]}
    for philox in (False, True):
        whole = moves(net, t, x, lp, grad, K, target_acceptance=TARGET, noise="philox" if philox else (z, u), seed=77)
        assert same(whole, parts(split, philox))
        odd = parts(split + 4, philox)
        print(f"\ntilted_moves case {case} rows split at {split + 4} ({'philox' if philox else 'injected'}): equal to the one launch: {same(whole, odd)}")
    assert not torch.equal(whole["x"], x)


def sd_tilted_waves(ntiles):  # csrc/tilted_kernel.hpp
    w = 1
    while w < 8 and ntiles // (2 * w) >= 256:
        w *= 2
    return w


def sd_tilted_grid(ntiles, waves):
    return min(512, max(1, -(-ntiles // waves)))


GEOMETRIES = {
    # the first M above 8 192 that is no multiple of 16: two waves per workgroup, the last workgroup's second wave idle, 15 pad rows
    "idle_wave": dict(M=8193, ntiles=513, waves=2, grid=257, rounds=1, idle=1),
    # just above 65 536: eight waves, more tiles than 512 workgroups hold: a second round, in which all but one wave of the grid idle
    "second_round": dict(M=65537, ntiles=4097, waves=8, grid=512, rounds=2, idle=4095),
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_launch_geometry(name, gpu):
    """Case a's net (d = 2) with K = 2 moves under torch's generator against the host composition of the one-move test, at the two
    geometries above (derived here from sd_tilted_waves / sd_tilted_grid).  With 10^4 .. 10^5 chains some decisions of any seed are
    near ties, so the seed condition of the one-move test becomes a per-chain one: chains of which a decision of the yardstick run lies
    within 1e-3 of its uniform (or a step-size test within 1e-4 of its threshold: a flipped update changes the next step by 1 %) are left
    out of the comparison (expected: 2 moves x 2e-3 of the chains; asserted: under 1 %); every other
    chain must take the same two decisions and end within 2e-5 of the yardstick's state.  That bound is the one of
    test_samplers_over_an_ebm_match_the_autograd_closure for two moves: 2 moves x 1.8^2 x step 0.02 x 2 e_grad x (1 + |grad| <= 31), with
    e_grad = 10 x 1.7e-7, is 1.4e-5."""
    geo = GEOMETRIES[name]
    M = geo["M"]
    ntiles = -(-M // 16)
    waves = sd_tilted_waves(ntiles)
    grid = sd_tilted_grid(ntiles, waves)
    rounds = -(-ntiles // (grid * waves))
    assert M % 16 != 0 and dict(M=M, ntiles=ntiles, waves=waves, grid=grid, rounds=rounds, idle=rounds * grid * waves - ntiles) == geo
    _, net, _, _ = on_gpu("a", gpu)
    times = torch.tensor(tc.CASES["a"]["times"])
    # three runs; of equal length at M = 8193 (tiles straddle the boundaries), else one time per row
    t = times[(torch.arange(M) * 3) // M].reshape(-1, 1).to(gpu)
    s, sig = net.sde.s(t), net.sde.sigma_sq(t)
    z0 = torch.randn(M, 2, generator=torch.Generator().manual_seed(41)).to(gpu)
    x = (s * net.mean_gauss + s * torch.sqrt(net.var_gauss + sig) * z0).contiguous()
    lp, grad = E.tilted_eval(net, t, x)
    torch.manual_seed(42)
    want, trace = host_moves(net, t, x, lp, grad, 2)
    torch.manual_seed(42)
    got = moves(net, t, x, lp, grad, 2, target_acceptance=TARGET)
    clear = torch.ones(M, dtype=torch.bool, device=gpu)
    for tr in trace:
        clear &= (torch.exp(tr["log_acc"]).clamp(max=1.0) - tr["u"]).abs() > 1e-3
        for edge in (math.log(TARGET) + math.log1p(0.05), math.log(TARGET) + math.log1p(-0.05)):  # ... or a step-size test: 1e-4 of its threshold
            clear &= (tr["log_acc"] - edge).abs() > 1e-4
    diff = (got["x"] - want["x"]).abs().amax(1)
    print(f"\ntilted_moves geometry {name}: {geo}; near-tie chains left out {int((~clear).sum())} of {M}; max |x - host| over the others "
          f"{float(diff[clear].max()):.2e}; acc_last mean {float(got['acc_last'].mean()):.4f}; bit-equal chains {int((diff == 0).sum())}")
    assert int((~clear).sum()) < M // 100
    assert torch.isfinite(got["x"]).all() and torch.isfinite(got["lp"]).all()
    assert float(diff[clear].max()) < 2e-5
    assert float(((got["step"] - want["step"]).abs() / want["step"])[clear].max()) <= 4.0 * EPS  # the same two heuristic updates


def test_philox_normals_are_replayed_by_stream_8(gpu):
    """The unadjusted move, one move, Philox: x_out = x + step grad + sqrt(2 step) z with z from sdeng_philox_normal_steps(stream_id = 8,
    step0 = the move, particle0 = chain0); bound of the one-move test."""
    fx, net, t, x, lp, grad = start("d", gpu)  # d = 61: the last quad of a row is partly pad
    M, d = x.shape
    seed, chain0 = 0xC0FFEE12345, 1000
    got = moves(net, t, x, lp, grad, 1, unadjusted=True, noise="philox", seed=seed, chain0=chain0)
    z = torch.empty(1, M, d, device=gpu)
    L.check(L.lib().sdeng_philox_normal_steps(seed, 0, 1, chain0, M, d, 8, z.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)))
    step = torch.full((M, 1), STEP, device=gpu)
    want = torch.sqrt(2.0 * step) * z[0] + (x + step * grad)
    excess = float(((got["x"] - want).abs().double() - proposal_bound(dict(x0=x, g0=grad, z=z[0], s0=step))).max())
    print(f"\ntilted_moves philox replay: max |diff| - bound = {excess:.2e}, bit-equal {torch.equal(got['x'], want)}; |z| mean {float(z.abs().mean()):.3f}")
    assert excess <= 0.0 and 0.7 < float(z.abs().mean()) < 0.9
    other = moves(net, t, x, lp, grad, 1, unadjusted=True, noise="philox", seed=seed + 1, chain0=chain0)
    assert not torch.equal(other["x"], got["x"])


def test_philox_chains_keep_the_mixture(gpu):
    """MALA on case f, whose zero last layer makes the density exactly the mixture noised to t: 4 096 chains start from exact draws of
    it (net.sample_prior), run 32 moves on Philox noise, and are then still exact draws (MALA leaves its target invariant; the chains are
    independent).  Every coordinate's mean and variance must lie within 5 standard errors of the mixture's own moments: coordinate i is a
    1-D Gaussian mixture with means m_k = s mu_ki and variances v_k = s^2 sum_a P_kia^2 (D_ka + sigma^2), so mean = sum w m, variance
    = sum w (v + (m - mean)^2), fourth central moment mu4 = sum w ((m - mean)^4 + 6 (m - mean)^2 v + 3 v^2), se(mean) = sqrt(var / M),
    se(variance) = sqrt((mu4 - var^2) / M).  Seeded, run once."""
    fx, net, _, _ = on_gpu("f", gpu)
    M, n_moves, tt = 4096, 32, 0.3
    t = torch.full((M, 1), tt, device=gpu)
    torch.manual_seed(51)
    x = net.sample_prior(t).contiguous()
    lp, grad = E.tilted_eval(net, t, x)
    got = moves(net, t, x, lp, grad, n_moves, target_acceptance=TARGET, noise="philox", seed=52, want_samples=False)
    _, _, tinfo = E.tilted_times(net, torch.tensor(tt), M)
    s, sig = float(tinfo[0, 1]), float(tinfo[0, 2])
    w = (net.weights / net.weights.sum()).double().cpu().reshape(-1, 1)
    m = s * net.means.double().cpu()
    D, P = net.cov_D.double().cpu().reshape(m.shape), net.cov_P.double().cpu().reshape(m.shape[0], m.shape[1], m.shape[1])
    v = s * s * torch.einsum("kia,ka->ki", P * P, D + sig)
    mean = (w * m).sum(0)
    var = (w * (v + (m - mean) ** 2)).sum(0)
    mu4 = (w * ((m - mean) ** 4 + 6.0 * (m - mean) ** 2 * v + 3.0 * v * v)).sum(0)
    xs = got["x"].double().cpu()
    z_mean = (xs.mean(0) - mean) / torch.sqrt(var / M)
    z_var = (xs.var(0, unbiased=True) - var) / torch.sqrt((mu4 - var * var) / M)
    acc = float((got["acc_sum"] / n_moves).mean())
    moved = float((got["x"] != x).any(1).float().mean())
    print(f"\ntilted_moves philox statistics: max |z| of the means {float(z_mean.abs().max()):.2f}, of the variances {float(z_var.abs().max()):.2f} "
          f"(16 coordinates each, bound 5); mean acceptance {acc:.4f}; chains that moved {moved:.3f}; step mean {float(got['step'].mean()):.4f}")
    assert torch.isfinite(got["x"]).all()
    assert float(z_mean.abs().max()) < 5.0 and float(z_var.abs().max()) < 5.0
    assert 0.0 < acc < 1.0 and moved > 0.99


class EvalSpy:
    """Counts the E.tilted_eval calls (what the closure, the classes and the host loops evaluate through)."""

    def __init__(self, monkeypatch):
        self.n = 0
        real = E.tilted_eval

        def spy(*a, **kw):
            self.n += 1
            return real(*a, **kw)
        monkeypatch.setattr(E, "tilted_eval", spy)


@pytest.mark.parametrize("kind", ["re", "smc"])
def test_samplers_run_their_local_moves_through_the_kernel(kind, gpu, monkeypatch):
    """The schedule of tests/test_gpu_tilted.py (3 levels x 8 chains, 2 + 4 moves, swap_frequency = 3).  Replica exchange: steps 0 and 3
    are swap steps, so two runs of two moves; five evaluations (the initial one, two per swap step).  SMC: one run and one evaluation
    per level.  With NATIVE_MOVES off the same seed gives the same chains, within the 5e-4 derived in the existing sampler test (the two
    routes are the two sides of the one-move test)."""
    _, net, _, _ = on_gpu("a", gpu)
    fn = ebm_mle.ebm_log_prob_and_grads(net)
    spy, calls = EvalSpy(monkeypatch), ebm_mle._native_calls[0]
    native = run_sampler(kind, fn, net, gpu, SAMPLER_SEED[kind])
    runs, evals = ebm_mle._native_calls[0] - calls, spy.n
    assert (runs, evals) == ((2, 5) if kind == "re" else (LEVELS, LEVELS))
    monkeypatch.setattr(ebm_mle, "NATIVE_MOVES", False)
    calls, spy.n = ebm_mle._native_calls[0], 0
    host = run_sampler(kind, fn, net, gpu, SAMPLER_SEED[kind])
    assert ebm_mle._native_calls[0] == calls and spy.n == evals + (4 if kind == "re" else 6 * LEVELS)  # one evaluation per local move
    diff = float((native - host).abs().max())
    print(f"\n{kind}_sampler over an EBM, one-launch moves against the host loop: max |chain difference| = {diff:.2e}")
    assert native.shape == (LEVELS, KEEP, CHAINS, 2) and torch.isfinite(native).all() and diff < 5e-4
    monkeypatch.setattr(ebm_mle, "NATIVE_MOVES", True)  # Philox noise: other chains, same shapes, still finite
    monkeypatch.setattr(ebm_mle, "NATIVE_NOISE", True)
    other = run_sampler(kind, fn, net, gpu, SAMPLER_SEED[kind])
    assert other.shape == native.shape and torch.isfinite(other).all() and not torch.equal(other, native)


@pytest.mark.parametrize("sampler_type,kw,rows,runs", [("replica_exchange", dict(swap_frequency=2), 32, 4), ("cd", {}, 16, 1)])
def test_trainer_samples_through_the_kernel(sampler_type, kw, rows, runs, gpu):
    """MaximumLikelihoodEBM.train at the sizes of tests/test_gpu_tilted_train.py: one epoch of replica exchange (four batches; the first
    batch's negatives are sample_prior's, the second samples with 3 + 1 steps at swap_frequency 2 -- swap, move, swap, move: two runs of
    one move --, the last two with 2 + 1 steps: one run each), and contrastive divergence for two batches (the first is sample_prior's
    again, so the second is the one batch that runs cd_sampling: one run of 3 + 1 moves).  The parameters move and stay finite."""
    from tests.test_gpu_tilted_train import REG, make_trainer
    mle, net = make_trainer(gpu, sampler_type, **kw)
    before = [p.detach().clone() for p in net.parameters()]
    data = 0.5 * torch.randn(rows, 2, generator=torch.Generator().manual_seed(32)).to(gpu)
    torch.manual_seed(6)
    calls = ebm_mle._native_calls[0]
    losses, norms, diagnostics = mle.train(data, 8, 1, initial_n_warmup_mcmc_steps=3, n_mcmc_steps=3, reg_val=REG, verbose=False, lr=1e-3)
    samplings = rows // 8 - 1
    assert ebm_mle._native_calls[0] - calls == runs
    assert len(diagnostics) == samplings and all(0.0 <= float(torch.as_tensor(dg["local_acc"]).mean()) <= 1.0 for dg in diagnostics)
    assert torch.isfinite(losses).all() and torch.isfinite(norms).all()
    assert all(not torch.equal(p, q) and torch.isfinite(p).all() for p, q in zip(net.parameters(), before))
    steps = mle.step_sizes_per_noise
    assert steps.numel() == 3 * 8 and torch.isfinite(steps).all() and bool((steps > 0).all())
