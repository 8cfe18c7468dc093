"""Langevin moves in one launch (sdeng_langevin_moves), without a GPU: the C entry point shares its host path with sdeng_rwmh_moves, so it
refuses what that one refuses (tests/test_rwmh_cpu.py) -- validation comes before any HIP call, so nothing is launched -- and
engine.langevin_moves checks everything the kernel indexes."""
import ctypes

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from tests import langevin_cases as lc
from tests.test_dispatch_cpu import P, _dist


def _call(kind=L.DIST_GMM_DIAG, target=True, prior=None, B=8, d=2, n_moves=4, keep_from=0, ula=0, t=None, x=P, lp=P, grad=P, step=P, z=None,
          u=None, ws=None, ws_bytes=0):
    lib = L.lib()
    ds, dp = L.Dist(), L.Dist()
    _dist(ds, kind)
    if prior is not None:
        _dist(dp, prior)
    rc_ = lib.sdeng_langevin_moves(ctypes.byref(dp) if prior is not None else None, ctypes.byref(ds) if target else None, B, d, n_moves, keep_from,
                                   ula, 0.75, t, x, lp, grad, step, z, u, 1, 0, None, None, None, ws, ws_bytes, None)
    return rc_, lib.sdeng_last_error().decode()


@pytest.mark.parametrize("kw", [dict(target=False), dict(x=None), dict(lp=None), dict(grad=None), dict(step=None), dict(B=-1), dict(d=0),
                                dict(n_moves=-1), dict(keep_from=-1), dict(keep_from=5), dict(z=P), dict(u=P), dict(kind=L.DIST_NONE)])
def test_invalid_arguments_are_refused_before_any_launch(kw):
    """(z without u, or u without z, is MALA here: ula = 0)"""
    code, msg = _call(**kw)
    assert code == L.E_INVALID and "langevin_moves" in msg, (kw, code, msg)


def test_refusals_and_the_workspace_stop():
    code, msg = _call(d=256)
    assert code == L.E_UNSUPPORTED and "langevin_moves" in msg and "d <= 255" in msg and "256" in msg
    for kw in (dict(kind=L.DIST_RINGS, d=3), dict(prior=L.DIST_RINGS, d=3)):  # both ends of the path are validated before anything runs
        code, msg = _call(**kw)
        assert code == L.E_INVALID and "two-dimensional" in msg, (kw, code, msg)
    for kw in (dict(kind=L.DIST_CHECKERBOARD), dict(prior=L.DIST_CHECKERBOARD)):
        code, msg = _call(**kw)
        assert code == L.E_UNSUPPORTED and "checkerboard" in msg, (kw, code, msg)
    assert _call(B=0)[0] == 0 and _call(n_moves=0)[0] == 0  # nothing to do: no workspace needed
    # a valid call stops at the workspace: NULL, or shorter than sdeng_langevin_moves_workspace_bytes
    for kind, d in ((L.DIST_RINGS, 2), (L.DIST_GMM_DIAG, 24), (L.DIST_ISO_GAUSS, 255), (L.DIST_GAUSS_DIAG, 5)):
        for prior in (None, L.DIST_NONE, L.DIST_GAUSS_DIAG):
            ds, dp = L.Dist(), L.Dist()
            _dist(ds, kind)
            _dist(dp, prior or L.DIST_NONE)
            need = L.lib().sdeng_langevin_moves_workspace_bytes(ctypes.byref(dp) if prior is not None else None, ctypes.byref(ds), d)
            assert need >= 256 and need >= L.lib().sdeng_rwmh_moves_workspace_bytes(ctypes.byref(ds), d)
            # (MALA with both or neither; ULA may inject the normals alone, or the uniforms it never reads)
            for ula, z, u in ((0, None, None), (0, P, P), (1, None, None), (1, P, P), (1, P, None), (1, None, P)):
                code, msg = _call(kind=kind, prior=prior, d=d, ula=ula, z=z, u=u, t=P, keep_from=4)
                assert code == L.E_WORKSPACE and str(need) in msg, (kind, prior, d, ula, code, msg)
            code, msg = _call(kind=kind, prior=prior, d=d, ws=P, ws_bytes=need - 1)
            assert code == L.E_WORKSPACE and str(need - 1) in msg and str(need) in msg and "langevin_moves" in msg
    assert L.lib().sdeng_langevin_moves_workspace_bytes(None, None, 2) == 0


def test_engine_langevin_moves_checks_what_the_kernel_indexes(monkeypatch):
    from sde_sampler_lrds_amd.distr.gauss import IsotropicGauss
    monkeypatch.setattr(E, "require_gpu", lambda x: None)
    monkeypatch.setattr(E, "_stream_ptr", lambda device: None)
    target, prior = IsotropicGauss(dim=3, scale=1.0), IsotropicGauss(dim=3, scale=2.0)
    B, d = 6, 3
    x, lp, grad, step = torch.zeros(B, d), torch.zeros(B), torch.zeros(B, d), torch.ones(B)
    with pytest.raises(ValueError, match=r"langevin_moves: x must be \[B, d\]"):
        E.langevin_moves(target, prior, torch.zeros(B, d, 1), lp, grad, step, 4)
    with pytest.raises(ValueError, match=r"x must be \[B, d\]"):
        E.langevin_moves(target, prior, torch.zeros(B), lp, grad, step, 4)
    with pytest.raises(ValueError, match="langevin_moves: lp and step must hold one value per chain"):
        E.langevin_moves(target, prior, x, torch.zeros(B - 1), grad, step, 4)
    with pytest.raises(ValueError, match="one value per chain"):
        E.langevin_moves(target, prior, x, lp, grad, torch.ones(B + 1), 4)
    for bad in (torch.zeros(B, d + 1), torch.zeros(B - 1, d), torch.zeros(B * d)):
        with pytest.raises(ValueError, match="grad must have the shape of x"):
            E.langevin_moves(target, prior, x, lp, bad, step, 4)
    for n in (2, B - 1, B + 1, 2 * B):
        with pytest.raises(ValueError, match="t must hold one tempering weight, or one per chain"):
            E.langevin_moves(target, prior, x, lp, grad, step, 4, t=torch.ones(n))
    for keep_from in (-1, 5):
        for unadjusted in (False, True):
            with pytest.raises(ValueError, match="keep_from"):
                E.langevin_moves(target, prior, x, lp, grad, step, 4, keep_from=keep_from, unadjusted=unadjusted)
    with pytest.raises(ValueError, match="noise"):
        E.langevin_moves(target, prior, x, lp, grad, step, 4, noise="numpy")
    with pytest.raises(ValueError, match="grad must be a contiguous float32"):
        E.langevin_moves(target, prior, x, lp, grad.double(), step, 4)
    with pytest.raises(ValueError, match="step must be a contiguous float32"):
        E.langevin_moves(target, prior, x, lp, grad, torch.ones(2 * B)[::2], 4)
    for t in (None, torch.ones(1), torch.ones(B), torch.ones(B, 1)):  # well-formed host tensors: still no launch
        with pytest.raises(ValueError, match="x must be a contiguous float32 CUDA"):
            E.langevin_moves(target, prior, x, lp, grad, step, 4, t=t)
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="MI355X"):
        E.langevin_moves(target, prior, x, lp, grad, step, 4)


@pytest.mark.parametrize("B", lc.EDGE_B)
@pytest.mark.parametrize("d", lc.EDGE_D)
def test_edge_shape_seeds_keep_every_decision_from_its_threshold(d, B):
    """The condition under which tests/test_gpu_langevin_moves.py allows no flipped chain: the MALA chains of each edge shape, run here
    with the distributions' own torch log-density and score in float32, take every accept / reject decision more than lc.MARGIN from
    its threshold -- and take both decisions somewhere among the 65-chain shapes."""
    seed = lc.SEEDS[d, B]
    target, prior, x0, t, step0 = lc.edge_inputs(d, B, seed)
    margins = []
    torch.manual_seed(seed)
    xs, x, lp, grad, step = lc.host_chain(lc.torch_path(target, prior), t, x0, step0, lc.N_MOVES, False, margins=margins)
    assert len(margins) == lc.N_MOVES and float(torch.stack(margins).min()) > lc.MARGIN
    assert xs.shape == (lc.N_MOVES, B, d) and bool(torch.isfinite(xs).all()) and bool(torch.isfinite(lp).all())
    if B == 65:
        moved = (xs[1:] != xs[:-1]).any(dim=-1)
        assert bool(moved.any()) and not bool(moved.all())
