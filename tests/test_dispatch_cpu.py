"""Kernel selection without a GPU.  sdeng_simulate and sdeng_ctrl_forward validate the descriptor and select the kernel instance
before any HIP call, so a call with workspace = NULL returns E_WORKSPACE when the descriptor passes both phases, and E_UNSUPPORTED /
E_INVALID when it is rejected.  Nothing is launched: the data pointers below only have to be non-null, they are never read."""
import ctypes
import itertools

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from tests import build_cases as bc
from tests import golden_cases as gc

_HOST = ctypes.create_string_buffer(64)
P = ctypes.addressof(_HOST)  # a non-null address for every array argument (never dereferenced: nothing is launched)
D_OF_TILES = {1: 2, 2: 29, 3: 45, 4: 61, 5: 77, 6: 93, 7: 100, 8: 128}
REFS = [(L.REF_NONE, 0, 0), (L.REF_GAUSS_DIAG, 1, 0)] + [(L.REF_GMM_DIAG, k, sv) for k in (2, 4, 16, 100) for sv in (0, 1)] + \
       [(L.REF_GMM_FULL, 3, 0)]
CTRLS = [L.CTRL_CLIPPED, L.CTRL_SCORE, L.CTRL_LERP, L.CTRL_CANCEL_DRIFT, L.CTRL_NONE]
TARGETS = [L.DIST_NONE, L.DIST_GMM_DIAG, L.DIST_GAUSS_DIAG, L.DIST_ISO_GAUSS, L.DIST_PHI4, L.DIST_LOGREG, L.DIST_GAUSS_FULL, L.DIST_RINGS,
           L.DIST_GMM_FULL, L.DIST_CHECKERBOARD]
FORMS = [L.FORM_LIN, L.FORM_EM, L.FORM_CMCD, L.FORM_EUBO, L.FORM_CMCD_EUBO]
VARIANTS = [(0, False), (L.FLAG_SPLIT_TILES, False), (L.FLAG_CTRL_NOISE, False), (L.FLAG_CTRL_DROPOUT, False), (L.FLAG_REMOVE_REF, False),
            (0, True), (L.FLAG_SPLIT_TILES | L.FLAG_CTRL_NOISE, False)]  # (flags, xs_out and noise_in set)


def _dist(ds, kind, k=4):
    ds.kind, ds.k = kind, k
    ds.loc = ds.scale = ds.w = ds.aux = P
    ds.p0 = ds.p1 = ds.p2 = ds.p3 = 1.0


def _desc(d, B=256):
    desc = L.Desc()
    desc.abi_version, desc.B, desc.d, desc.N = L.ABI_VERSION, B, d, 8
    desc.coef = desc.x_in = desc.x_out = desc.rnd_out = P
    n = desc.net
    n.w_in = n.b_in = n.w_h1 = n.b_h1 = n.w_h2 = n.b_h2 = n.w_out = n.b_out = P
    te = n.t_embed
    te.coeff = te.phase = te.w_out = te.b_out = te.w[0] = te.b[0] = P
    te.n_hidden, te.dim_out = 1, 64
    _dist(desc.prior, L.DIST_ISO_GAUSS)
    return desc


def _check(lib, rc, what):
    msg = lib.sdeng_last_error().decode()
    assert rc in (L.E_WORKSPACE, L.E_UNSUPPORTED, L.E_INVALID), (what, rc, msg)
    assert "no kernel instance" not in msg, (what, msg)
    return rc == L.E_WORKSPACE


def test_simulate_selection_sweep():
    lib = L.lib()
    accepted = set()
    for nt, (rk, k, sv), ctrl, tk, form, (flags, io) in itertools.product(D_OF_TILES, REFS, CTRLS, TARGETS, FORMS, VARIANTS):
        desc = _desc(D_OF_TILES[nt], B=256 if flags & L.FLAG_SPLIT_TILES else 20000)
        desc.form = form
        desc.flags = flags | (L.FLAG_INIT_LOGP | L.FLAG_TERM_TARGET if form in (L.FORM_CMCD, L.FORM_CMCD_EUBO) else 0)
        desc.xs_out = desc.noise_in = P if io else None
        desc.net.ctrl_kind = ctrl
        desc.ref.kind, desc.ref.k, desc.ref.shared_var = rk, k, sv
        desc.ref.means_init = desc.ref.vars_init = desc.ref.weights = desc.ref.eigvecs = P if rk else None
        if tk != L.DIST_NONE:
            _dist(desc.target, tk)
        if _check(lib, lib.sdeng_simulate(ctypes.byref(desc), None), (nt, rk, k, sv, ctrl, tk, form, flags, io)):
            accepted.add((nt, rk, ctrl, tk, form))
    # every tile count, reference kind, control kind, target kind and form reaches a kernel
    for i, values in enumerate((D_OF_TILES, [r[0] for r in REFS], CTRLS, TARGETS, FORMS)):
        assert {a[i] for a in accepted} == set(values), i


def test_ctrl_forward_selection_sweep():
    lib = L.lib()
    accepted = set()
    for nt, ctrl, tk in itertools.product(D_OF_TILES, CTRLS, TARGETS):
        desc = _desc(D_OF_TILES[nt])
        desc.net.ctrl_kind = ctrl
        if tk != L.DIST_NONE:
            _dist(desc.target, tk)
        rc = lib.sdeng_ctrl_forward(ctypes.byref(desc), 0.5, 1.0, 0.0, P, P, None)
        if _check(lib, rc, (nt, ctrl, tk)):
            accepted.add((nt, ctrl, tk))
        if ctrl != L.CTRL_CLIPPED and tk == L.DIST_LOGREG:  # no ctrl_forward kernel has a logistic-regression score
            assert rc == L.E_UNSUPPORTED
    assert {a[0] for a in accepted} == set(D_OF_TILES)
    assert (8, L.CTRL_SCORE, L.DIST_GMM_DIAG) in accepted and (4, L.CTRL_LERP, L.DIST_PHI4) in accepted


@pytest.mark.parametrize("name", [n for n in gc.SIM_CASES if n != "cmcd_logreg_d61"])
def test_golden_case_descriptors_select_a_kernel(name, monkeypatch):
    """The descriptor each case's loss compiles on the host passes validation and selection (then stops at the NULL workspace)."""
    lib = L.lib()

    class NoWorkspace:
        def get(self, nbytes, device):
            return torch.empty(0, dtype=torch.uint8)

    monkeypatch.setattr(E, "require_gpu", lambda x: None)
    monkeypatch.setattr(E, "_stream_ptr", lambda device: None)
    monkeypatch.setattr(E, "_WS", NoWorkspace())
    c = gc.load(name)
    b = bc.build(c, "cpu")
    with pytest.raises(L.EngineError) as err:
        b["loss"].simulate(b["ts"], b["x0"], *b["args"], **b["kwargs"])
    assert err.value.code == L.E_WORKSPACE, str(err.value)
    assert "no kernel instance" not in lib.sdeng_last_error().decode()
