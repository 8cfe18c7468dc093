"""The Checkerboard target on the host (fixtures: tests/golden/gen_golden_toy.py, from the reference): the mirror's log-density and
score, the descriptor the engine builds from it (and from an object of the reference's own class), and ``make_model`` on the toy suite.
CPU only: nothing here launches a kernel."""
import math

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.distr.checkerboard import Checkerboard
from sde_sampler_lrds_amd.experiments import benchmark_utils as bu
from sde_sampler_lrds_amd.models import reparam
from tests import golden_cases as gc


def test_mirror_log_density_is_bit_identical_to_the_reference():
    c = gc.load("toy_checkerboard_logp")
    lp = Checkerboard().unnorm_log_prob(c["x"])
    assert lp.shape == c["logp"].shape
    assert torch.equal(torch.isinf(lp), torch.isinf(c["logp"])) and not torch.isnan(lp).any()
    assert torch.equal(lp, c["logp"])  # (-inf == -inf): finite values and the places of -inf alike
    assert c.meta["n_inf"] > 100 and int(torch.isfinite(lp).sum()) > 100


def test_squares_are_half_open_and_nan_is_outside():
    cb = Checkerboard()
    lo, hi = cb.low, cb.high
    inside = cb.unnorm_log_prob(lo)  # low corner: inside
    assert torch.isfinite(inside).all()
    assert torch.isinf(cb.unnorm_log_prob(torch.tensor([[-2.0, 4.0]]))).all()  # high edge of square 0 in y, no square above
    assert torch.isinf(cb.unnorm_log_prob(torch.tensor([[float("nan"), 3.0], [-1.0, float("nan")]]))).all()
    w = cb.distr.mixture_distribution.probs
    assert torch.allclose(w, torch.tensor([3.0, 1.0] * 4) / 16.0)
    assert torch.allclose(inside.view(-1), torch.log(w) - 2.0 * math.log(2.0))


def test_mirror_tables_score_and_domain():
    c = gc.load("toy_checkerboard_logp")
    cb = Checkerboard(dim=2, width=4)
    assert cb.n_mixtures == 8
    assert torch.equal(cb.low, c["low"]) and torch.equal(cb.high, c["high"]) and torch.equal(cb.loc, c["loc"])
    assert torch.equal(cb.distr.mixture_distribution.probs, c["probs"])
    assert torch.equal(cb.low[:, 0], torch.tensor([-2.0, 2.0, -4.0, 0.0, -2.0, 2.0, -4.0, 0.0]))
    assert torch.equal(cb.high[:, 1], torch.tensor([4.0, 4.0, 2.0, 2.0, 0.0, 0.0, -2.0, -2.0]))
    assert torch.equal(cb.domain, torch.tensor([[-4.0, 4.0], [-4.0, 4.0]]))
    assert torch.equal(cb.score(c["x"]), torch.zeros_like(c["x"])) and torch.equal(c["score"], torch.zeros_like(c["x"]))
    s = cb.sample((4096,))
    assert s.shape == (4096, 2) and torch.isfinite(cb.unnorm_log_prob(s)).all()
    with pytest.raises(ValueError):
        Checkerboard(dim=3)


class _Stand:
    """A stand-in for the reference's object: same class name and the attributes the engine reads (``distr``, ``unnorm_log_prob``),
    derived from none of this package's types."""


def _reference_like():
    mirror = Checkerboard()
    obj = type("Checkerboard", (_Stand,), {})()
    obj.distr = mirror.distr
    obj.unnorm_log_prob = lambda x: obj.distr.log_prob(x).unsqueeze(-1)
    return obj


@pytest.mark.parametrize("make", [Checkerboard, _reference_like])
def test_descriptor_tables(make):
    c = gc.load("toy_checkerboard_logp")
    keep = []
    ds = E.dist_desc(make(), "cpu", keep)
    assert ds.kind == L.DIST_CHECKERBOARD == 9 and ds.k == 8
    by_ptr = {t.data_ptr(): t for t in keep}
    low, high, const = by_ptr[ds.loc], by_ptr[ds.scale], by_ptr[ds.w]
    assert torch.equal(low, c["low"]) and torch.equal(high, c["high"])
    # the per-square constant is the reference's own log-density anywhere inside the square (here: at every probe point inside)
    inside = torch.isfinite(c["logp"].view(-1))
    x = c["x"][inside]
    sq = ((x[:, None, :] >= low[None]) & (x[:, None, :] < high[None])).all(-1).float().argmax(-1)
    assert torch.equal(const[sq], c["logp"].view(-1)[inside])


def test_make_target_details_checkerboard():
    assert bu.make_target_details("checkerboard") == {"name": "checkerboard"}
    assert isinstance(bu._make_target(bu.make_target_details("checkerboard")), Checkerboard)


TRAIN = dict(train_steps=10, train_batch_size=8, eval_batch_size=16)


@pytest.mark.parametrize("solver,ref,time_type", [("pis_orig", "default", "uniform"), ("dds_orig", "default", "uniform"),
                                                 ("dis_orig", "default", "uniform"), ("cmcd", "gaussian", "uniform"),
                                                 ("vp-ref", "default", "uniform"), ("pbm-ref", "default", "snr")])
def test_make_model_builds_the_toy_suite_on_the_checkerboard(solver, ref, time_type):
    """experiments/sample_toy_competing.py on the checkerboard: base_zero_init with force_base_zero_init=True (a ClippedCtrl)."""
    details = dict(mean=torch.zeros(2), var=torch.tensor([[5.0, 0.4], [0.4, 4.5]])) if solver == "cmcd" else dict(sigma=1.7)
    model = bu.make_model(solver_type=solver, ref_type=ref, loss_type="lv", integrator_type="em", model_type="base_zero_init",
                          time_type=time_type, solver_details=details, target_details=bu.make_target_details("checkerboard"),
                          training_details=TRAIN, n_steps=4, force_base_zero_init=True, device="cpu")
    assert isinstance(model.target, Checkerboard)
    assert isinstance(E.unwrap_ctrl(model.generative_ctrl)[0], reparam.ClippedCtrl)
    assert E.dist_desc(model.target, "cpu", []).kind == L.DIST_CHECKERBOARD
