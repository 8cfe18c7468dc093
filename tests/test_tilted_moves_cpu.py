"""Host side of the one-launch Langevin moves over an energy-based reference (no GPU): the C ABI's declaration, exports and refusals --
every one reached before any launch --, the workspace arithmetic, and the samplers' route decision."""
import ctypes
import os
import re

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.additions import ebm_mle
from tests import tilted_cases as tc
from tests.test_tilted_cpu import P, _desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_binding():
    header = open(os.path.join(ROOT, "include", "sdeng.h")).read()
    assert re.search(r"\bint\s+sdeng_tilted_moves\(const sdeng_tilted\* desc, const sdeng_tilted_moves_state\* mv, void\* stream\);", header)
    assert re.search(r"\bsize_t\s+sdeng_tilted_moves_workspace_bytes\(const sdeng_tilted\* desc\);", header)
    assert "stream_id = 8" in header and "#define SDENG_ABI_VERSION 4" in header
    assert "sdeng_tilted_moves" in L.EXPORTS and "sdeng_tilted_moves_workspace_bytes" in L.EXPORTS
    assert [n for n, _ in L.TiltedMovesState._fields_] == ["n_moves", "keep_from", "unadjusted", "reserved", "target_acceptance", "x", "lp", "grad",
                                                           "step", "z", "u", "seed", "chain0", "samples", "acc_sum", "acc_last"]
    lib = L.lib()
    assert lib.sdeng_tilted_moves.argtypes[:2] == [ctypes.POINTER(L.Tilted), ctypes.POINTER(L.TiltedMovesState)]
    assert lib.sdeng_tilted_moves_workspace_bytes.restype is ctypes.c_size_t


def _state(**over):
    mv = L.TiltedMovesState()
    mv.n_moves, mv.keep_from, mv.target_acceptance = 4, 1, 0.75
    for n in ("x", "lp", "grad", "step", "z", "u"):
        setattr(mv, n, P)
    for k, v in over.items():
        setattr(mv, k, v)
    return mv


def _refused(d, mv):
    lib = L.lib()
    rc = lib.sdeng_tilted_moves(ctypes.byref(d), None if mv is None else ctypes.byref(mv), None)
    return rc, lib.sdeng_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(abi_version=3), "ABI version 3"), (dict(d=0), "d = 0"), (dict(d=129), "d = 129"), (dict(k=0), "k = 0"), (dict(k=17), "k = 17"),
    (dict(M=47), "M = 47"), (dict(n_times=0, M=0), "M = 0"), (dict(tinfo=None), "null pointer"), (dict(w_out=None), "null pointer"),
    (dict(mean_gauss=None), "null pointer"), (dict(full_cov=1), "eigvecs"),
])
def test_invalid_descriptors_are_refused_before_any_launch(over, word):
    d = _desc(**over)
    rc, msg = _refused(d, _state())
    assert rc == L.E_INVALID and word in msg, (rc, msg)
    assert L.lib().sdeng_tilted_moves_workspace_bytes(ctypes.byref(d)) == 0


def test_the_three_ignored_pointers_are_ignored():
    """x, log_prob and grad of the descriptor may be NULL: the chain state is the move state's."""
    d = _desc(x=None, log_prob=None, grad=None)
    assert L.lib().sdeng_tilted_moves_workspace_bytes(ctypes.byref(d)) > 0
    assert _refused(d, _state())[0] == L.E_WORKSPACE


@pytest.mark.parametrize("over,word", [
    (dict(x=None), "required"), (dict(lp=None), "required"), (dict(grad=None), "required"), (dict(step=None), "required"),
    (dict(n_moves=-1, keep_from=0), "n_moves = -1"), (dict(keep_from=-1), "keep_from = -1"), (dict(keep_from=5), "keep_from = 5"),
    (dict(z=None), "both"), (dict(u=None), "both"),
])
def test_invalid_move_states_are_refused_before_any_launch(over, word):
    rc, msg = _refused(_desc(), _state(**over))
    assert rc == L.E_INVALID and word in msg, (rc, msg)


def test_null_move_state_and_unadjusted_noise():
    rc, msg = _refused(_desc(), None)
    assert rc == L.E_INVALID and "null move state" in msg
    # the unadjusted move reads no uniforms: the normals alone pass the validation (and stop at the workspace)
    assert _refused(_desc(), _state(unadjusted=1, u=None))[0] == L.E_WORKSPACE
    assert _refused(_desc(), _state(z=None, u=None))[0] == L.E_WORKSPACE  # Philox


@pytest.mark.parametrize("over,word", [
    (dict(num_layers=4), "num_layers=4"), (dict(channels=64), "channels=64"), (dict(tilt_type=L.TILT_SQ_NORM), "'dot'"),
    (dict(tilt_type=L.TILT_SUM), "'dot'"), (dict(use_scaling_factor=1), "use_scaling_factor"),
])
def test_unsupported_descriptors_name_their_reason(over, word):
    rc, msg = _refused(_desc(**over), _state())
    assert rc == L.E_UNSUPPORTED and word in msg, (rc, msg)


def test_workspace_arithmetic_and_missing_workspace():
    """The layout of an evaluation with grad, the per-wave slots one layer (8 KiB) longer, then the proposal and proposal-score rows, each
    [M, d] floats rounded up to 64 floats."""
    lib = L.lib()
    d = _desc()  # M = 48, d = 16: three tiles, one wave each
    ev, need = lib.sdeng_tilted_eval_workspace_bytes(ctypes.byref(d)), lib.sdeng_tilted_moves_workspace_bytes(ctypes.byref(d))
    assert need - ev == 3 * 8192 + 2 * 4 * 48 * 16
    odd = _desc(M=50, n_times=50, rows_per_time=1, d=3)  # four tiles; 150 floats per array -> 192
    ev, mv = lib.sdeng_tilted_eval_workspace_bytes(ctypes.byref(odd)), lib.sdeng_tilted_moves_workspace_bytes(ctypes.byref(odd))
    assert mv - ev == 4 * 8192 + 2 * 4 * 192
    full = _desc(full_cov=1, eigvecs=P)
    assert lib.sdeng_tilted_moves_workspace_bytes(ctypes.byref(full)) - need == 2 * 3 * 65536
    rc, msg = _refused(d, _state())
    assert rc == L.E_WORKSPACE and "need" in msg
    d.workspace, d.workspace_bytes = P, need - 1  # one byte short: still refused, still before any launch
    assert _refused(d, _state())[0] == L.E_WORKSPACE


# ---- the route decision -------------------------------------------------------------------------------------------------------------
class _OnGpu:
    """A [B, d] float32 tensor that says it is on the GPU: the route decision reads properties, nothing else."""

    def __init__(self, x):
        self.x = x

    is_cuda, dtype = True, torch.float32

    def dim(self):
        return self.x.dim()

    @property
    def device(self):
        return self.x.device


def _frozen(case="a"):
    fx, net = tc.mirror(case)
    return fx, net.requires_grad_(False)


def test_route_recognises_the_closure_and_the_trainer_method():
    from sde_sampler_lrds_amd.distr.gauss import Gauss
    fx, net = _frozen()
    x = _OnGpu(fx["x"])
    fn = ebm_mle.ebm_log_prob_and_grads(net)
    assert fn.hip_net is net
    route = ebm_mle._native_route(fn, x, None)
    assert isinstance(route, ebm_mle._EbmRoute) and route.net is net
    mle = ebm_mle.MaximumLikelihoodEBM(net.sde, Gauss(dim=2, loc=0.0, scale=1.0), net, "replica_exchange")
    assert mle.hip_net is mle.net
    route = ebm_mle._native_route(mle.log_prob_and_grads, x, None)
    assert isinstance(route, ebm_mle._EbmRoute) and route.net is mle.net
    # the analytic pair is still the pair; an unmarked callable and another object's method are nothing
    pair = ebm_mle.hip_tempered_log_prob_and_grads(Gauss(dim=2, loc=0.0, scale=1.0), Gauss(dim=2, loc=1.0, scale=2.0))
    assert ebm_mle._native_route(pair, x, None) is pair.hip_pair
    assert ebm_mle._native_route(lambda t, y: None, x, None) is None
    assert ebm_mle._native_route(net.unnorm_log_prob_and_grad, x, None) is None
    mle.net.has_unnorm_log_prob_and_grad = False  # the trainer's autograd branch is not the kernel's density
    assert mle.hip_net is None and ebm_mle._native_route(mle.log_prob_and_grads, x, None) is None


def test_route_falls_back(monkeypatch):
    fx, net = _frozen()
    fn = ebm_mle.ebm_log_prob_and_grads(net)
    x = _OnGpu(fx["x"])
    assert ebm_mle._native_route(fn, x, None) is not None
    assert ebm_mle._native_route(fn, x, (torch.eye(2), torch.eye(2))) is None            # preconditioned moves: the host loop
    assert ebm_mle._native_route(fn, fx["x"], None) is None                              # CPU tensors
    assert ebm_mle._native_route(fn, _OnGpu(fx["x"].reshape(-1, 1, 2)), None) is None    # not [B, d]
    monkeypatch.setattr(ebm_mle, "NATIVE_MOVES", False)
    assert ebm_mle._native_route(fn, x, None) is None
    monkeypatch.setattr(ebm_mle, "NATIVE_MOVES", True)
    # what tilted_eval refuses stays on the host loop, whose first evaluation raises tilted_eval's own error
    net.requires_grad_(True)
    assert "grad mode" in E.tilted_refusal(net, torch.device("cpu")) and ebm_mle._native_route(fn, x, None) is None
    with torch.no_grad():
        assert ebm_mle._native_route(fn, x, None) is not None
    with pytest.raises(E.UnsupportedByEngine, match="parameters"):
        net.unnorm_log_prob_and_grad(fx["t"], fx["x"])
    net.requires_grad_(False)
    net.tilt_type = "sq_norm"
    assert "'dot'" in E.tilted_refusal(net, torch.device("cpu")) and ebm_mle._native_route(fn, x, None) is None
    net.tilt_type, net.use_scaling_factor = "dot", True
    assert "scaling_factor" in E.tilted_refusal(net, torch.device("cpu")) and ebm_mle._native_route(fn, x, None) is None


def test_cpu_tensors_do_not_reach_the_kernel():
    """A sampler over an EBM with CPU tensors takes the host loop, whose evaluation needs the GPU: _native_calls does not move."""
    fx, net = _frozen()
    calls = ebm_mle._native_calls[0]
    times = torch.tensor([0.2, 0.5, 0.8]).view(-1, 1, 1).repeat(1, 4, 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        ebm_mle.re_sampler(torch.zeros(4, 2), times, ebm_mle.ebm_log_prob_and_grads(net), 3, 2, 4, 0.02 * torch.ones(3, 4, 1))
    assert ebm_mle._native_calls[0] == calls
    x = fx["x"].clone()
    with pytest.raises(RuntimeError, match="MI355X"):  # the engine entry itself: checked before anything is built
        E.tilted_moves(net, fx["t"], x, torch.zeros(15), torch.zeros(15, 2), torch.full((15,), 0.02), 2)

