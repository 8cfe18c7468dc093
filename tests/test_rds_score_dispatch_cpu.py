"""Kernel selection for the reference samplers with a target-informed control, without a GPU (the method of tests/test_dispatch_cpu.py:
sdeng_simulate validates and selects before any HIP call, so a NULL workspace returns E_WORKSPACE exactly when a registered instance was
found).  Accepted here: a full-covariance mixture reference together with a Score / Lerp / CancelDrift control on a mixture or phi^4
target (forward forms and compute_eubo), compute_eubo of every reference kind with such a control, and RemoveReferenceCtrl over a
full-covariance reference on the forward forms."""
import ctypes
import itertools

import pytest

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from tests import rds_score_cases as cases
from tests.test_dispatch_cpu import D_OF_TILES, P, _desc, _dist

SCORE_CTRLS = [L.CTRL_SCORE, L.CTRL_LERP, L.CTRL_CANCEL_DRIFT]
SCORE_TARGETS = [L.DIST_GMM_DIAG, L.DIST_PHI4]
# (ref.kind, k, shared_var): Gaussian, small mixture (responsibilities in registers), large mixture -- also with one shared variance vector,
# which a ClippedCtrl would send to the matrix pipe --, full covariance
REFS = [(L.REF_GAUSS_DIAG, 1, 0), (L.REF_GMM_DIAG, 2, 0), (L.REF_GMM_DIAG, 16, 0), (L.REF_GMM_DIAG, 16, 1), (L.REF_GMM_FULL, 2, 0)]


def _probe(nt, ref, ctrl, tk, form, flags=0, io=False, B=20000):
    lib = L.lib()
    rk, k, sv = ref
    desc = _desc(D_OF_TILES[nt], B=B)
    desc.form, desc.flags = form, flags
    desc.xs_out = desc.noise_in = P if io else None
    desc.net.ctrl_kind = ctrl
    desc.ref.kind, desc.ref.k, desc.ref.shared_var = rk, k, sv
    desc.ref.means_init = desc.ref.vars_init = desc.ref.weights = desc.ref.eigvecs = P if rk else None
    if tk != L.DIST_NONE:
        _dist(desc.target, tk)
    rc = lib.sdeng_simulate(ctypes.byref(desc), None)
    return rc, lib.sdeng_last_error().decode()


@pytest.mark.parametrize("nt", sorted(D_OF_TILES))
def test_score_control_over_a_full_covariance_reference_selects_a_kernel(nt):
    """Every tile count (5 and 7 run on the 6- and 8-tile instances), LIN / EM with PAR 0 / 1 / 2 and EUBO with PAR 0 / 1."""
    ref = (L.REF_GMM_FULL, 2, 0)
    for ctrl, tk in itertools.product(SCORE_CTRLS, SCORE_TARGETS):
        for form, (flags, io) in itertools.product((L.FORM_LIN, L.FORM_EM), ((0, False), (0, True), (L.FLAG_CTRL_NOISE, False),
                                                                             (L.FLAG_CTRL_NOISE | L.FLAG_CTRL_DROPOUT, True))):
            rc, msg = _probe(nt, ref, ctrl, tk, form, flags, io)
            assert rc == L.E_WORKSPACE and "no kernel instance" not in msg, (nt, ctrl, tk, form, flags, io, rc, msg)
        for io in (False, True):
            rc, msg = _probe(nt, ref, ctrl, tk, L.FORM_EUBO, 0, io)
            assert rc == L.E_WORKSPACE and "no kernel instance" not in msg, (nt, ctrl, tk, io, rc, msg)


@pytest.mark.parametrize("nt", sorted(D_OF_TILES))
def test_compute_eubo_with_a_score_control_selects_a_kernel_for_every_reference(nt):
    for ref, ctrl, tk, io in itertools.product(REFS, SCORE_CTRLS, SCORE_TARGETS, (False, True)):
        rc, msg = _probe(nt, ref, ctrl, tk, L.FORM_EUBO, 0, io)
        assert rc == L.E_WORKSPACE and "no kernel instance" not in msg, (nt, ref, ctrl, tk, io, rc, msg)


def test_remove_reference_over_a_full_covariance_reference():
    ref = (L.REF_GMM_FULL, 2, 0)
    for nt, tk, form in itertools.product(sorted(D_OF_TILES), SCORE_TARGETS, (L.FORM_LIN, L.FORM_EM)):
        rc, msg = _probe(nt, ref, L.CTRL_CANCEL_DRIFT, tk, form, L.FLAG_REMOVE_REF)
        assert rc == L.E_WORKSPACE, (nt, tk, form, rc, msg)
    for ref in REFS:  # the noising direction has no RemoveReferenceCtrl
        rc, msg = _probe(3, ref, L.CTRL_CANCEL_DRIFT, L.DIST_GMM_DIAG, L.FORM_EUBO, L.FLAG_REMOVE_REF)
        assert rc == L.E_UNSUPPORTED and "FLAG_REMOVE_REF" in msg, (ref, rc, msg)
    rc, msg = _probe(3, (L.REF_GMM_FULL, 2, 0), L.CTRL_CLIPPED, L.DIST_GMM_DIAG, L.FORM_EM, L.FLAG_REMOVE_REF)  # nothing to remove it from
    assert rc == L.E_UNSUPPORTED and "FLAG_REMOVE_REF" in msg, (rc, msg)


def test_what_stays_refused_says_why():
    full = (L.REF_GMM_FULL, 2, 0)
    # an in-loop logistic-regression score together with a reference drift
    for ref, form in itertools.product(REFS, (L.FORM_LIN, L.FORM_EM, L.FORM_EUBO)):
        rc, msg = _probe(4, ref, L.CTRL_SCORE, L.DIST_LOGREG, form)
        assert rc == L.E_UNSUPPORTED and "logistic-regression" in msg, (ref, form, rc, msg)
    # a full-covariance mixture TARGET of a score control together with a reference drift, or in the noising direction
    for ref in REFS:
        rc, msg = _probe(3, ref, L.CTRL_SCORE, L.DIST_GMM_FULL, L.FORM_EM)
        assert rc == L.E_UNSUPPORTED and "full-covariance mixture target" in msg, (ref, rc, msg)
    rc, msg = _probe(3, (L.REF_NONE, 0, 0), L.CTRL_SCORE, L.DIST_GMM_FULL, L.FORM_EUBO)
    assert rc == L.E_UNSUPPORTED and "forward forms only" in msg, (rc, msg)
    # compute_eubo with neither a reference nor a score control
    rc, msg = _probe(3, (L.REF_NONE, 0, 0), L.CTRL_CLIPPED, L.DIST_GMM_DIAG, L.FORM_EUBO)
    assert rc == L.E_UNSUPPORTED and "compute_eubo kernels" in msg, (rc, msg)
    # the control perturbation belongs to the forward forms
    rc, msg = _probe(3, full, L.CTRL_SCORE, L.DIST_GMM_DIAG, L.FORM_EUBO, L.FLAG_CTRL_NOISE)
    assert rc == L.E_UNSUPPORTED and "FLAG_CTRL_NOISE" in msg, (rc, msg)
    # the split-tile kernels have no full-covariance reference and no score control: the flag is not honoured, the standard kernel runs
    for ctrl, tk in ((L.CTRL_CLIPPED, L.DIST_GMM_DIAG), (L.CTRL_SCORE, L.DIST_PHI4)):
        rc, msg = _probe(7, full, ctrl, tk, L.FORM_EM, L.FLAG_SPLIT_TILES, B=256)
        assert rc == L.E_WORKSPACE and "no kernel instance" not in msg, (ctrl, rc, msg)
    # a shared-variance mixture with a score control stays on the vector path (the matrix-pipe kernels are ClippedCtrl, forward forms)
    for form in (L.FORM_LIN, L.FORM_EM, L.FORM_EUBO):
        rc, msg = _probe(8, (L.REF_GMM_DIAG, 16, 1), L.CTRL_SCORE, L.DIST_GMM_DIAG, form)
        assert rc == L.E_WORKSPACE and "no kernel instance" not in msg, (form, rc, msg)


def test_python_raises_unsupported_by_engine_for_a_refused_descriptor(monkeypatch):
    """E_UNSUPPORTED from sdeng_simulate reaches the caller as the documented UnsupportedByEngine (a NotImplementedError), with the
    library's reason; other error codes stay EngineError."""
    import torch
    _no_workspace(monkeypatch)
    x = torch.zeros(32, 40)

    def desc(form, flags):
        d = _desc(40, B=32)
        d.form, d.flags, d.net.ctrl_kind = form, flags, L.CTRL_CANCEL_DRIFT
        d.ref.kind, d.ref.k = L.REF_GMM_FULL, 2
        d.ref.means_init = d.ref.vars_init = d.ref.weights = d.ref.eigvecs = P
        _dist(d.target, L.DIST_GMM_DIAG)
        return d
    with pytest.raises(E.UnsupportedByEngine, match="FLAG_REMOVE_REF"):
        E.run(desc(L.FORM_EUBO, L.FLAG_REMOVE_REF), x, [])
    with pytest.raises(L.EngineError) as err:  # accepted: stops at the NULL workspace
        E.run(desc(L.FORM_EUBO, 0), x, [])
    assert err.value.code == L.E_WORKSPACE


def _no_workspace(monkeypatch):
    import torch

    class NoWorkspace:
        def get(self, nbytes, device):
            return torch.empty(0, dtype=torch.uint8)

    monkeypatch.setattr(E, "require_gpu", lambda x: None)
    monkeypatch.setattr(E, "_stream_ptr", lambda device: None)
    monkeypatch.setattr(E, "_WS", NoWorkspace())


@pytest.mark.parametrize("name", cases.SIM_CASES + cases.EUBO_CASES)
def test_fixture_descriptors_select_a_kernel(name, monkeypatch):
    """The descriptor each fixture's loss compiles on the host passes validation and selection (then stops at the NULL workspace)."""
    _no_workspace(monkeypatch)
    c = cases.load(name)
    b = cases.build(c, "cpu")
    with pytest.raises(L.EngineError) as err:
        if c.meta["kind"] == "eubo_score":
            b["loss"].compute_eubo(b["ts"], b["x0"].clone(), *b["args"])
        else:
            b["loss"].simulate(b["ts"], b["x0"], *b["args"])
    assert err.value.code == L.E_WORKSPACE, str(err.value)
    assert "no kernel instance" not in L.lib().sdeng_last_error().decode()
