"""The committed CPU oracle against the fixtures of tests/golden/gen_golden_rds_score.py (the real reference's outputs): reference
samplers with a target-informed control -- ScoreCtrl, or RemoveReferenceCtrl(CancelDriftCtrl) -- over Gaussian, diagonal-mixture and
full-covariance mixture references, forward (simulate) and noising (compute_eubo) direction, under the fixture's noise.  CPU only."""
import pytest

from tests import golden_cases as gc
from tests import rds_score_cases as rc


@pytest.mark.parametrize("name", rc.SIM_CASES)
def test_simulate_matches_reference(name):
    c = rc.load(name)
    x, rnd = rc.run_oracle(c)
    tol = rc.oracle_tol(name)
    ex, er = gc.rel_err(x, c["out_x"]), gc.rel_err(rnd, c["rnd"])
    print(f"{name}: oracle vs reference x_N {ex:.2e}, rnd {er:.2e} (tolerance {tol:.0e})")
    assert ex < tol and er < tol


@pytest.mark.parametrize("name", rc.EUBO_CASES)
def test_compute_eubo_matches_reference(name):
    c = rc.load(name)
    x, rnd = rc.run_oracle(c)
    tol = rc.oracle_tol(name)
    ex = gc.rel_err(x, c["out_x"])
    er = float((rnd - c["rnd"]).abs().max()) / max(1.0, float(c["rnd"].abs().max()))
    print(f"{name}: oracle vs reference noised x {ex:.2e}, rnd {er:.2e} (tolerance {tol:.0e})")
    assert ex < tol and er < tol


@pytest.mark.parametrize("name", rc.SIM_CASES + rc.EUBO_CASES)
def test_one_ulp_outputs_are_the_references_own(name):
    """The stored response to x0 * (1 + 1.2e-7) is reproduced by the oracle from that input, to the same tolerance."""
    c = rc.load(name)
    x, rnd = rc.run_oracle(c, x0=c["x0"] * (1 + 1.2e-7))
    tol = rc.oracle_tol(name)
    assert gc.rel_err(x, c["out_x_ulp"]) < tol
    assert float((rnd - c["rnd_ulp"]).abs().max()) / max(1.0, float(c["rnd_ulp"].abs().max())) < tol
