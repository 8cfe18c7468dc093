"""Host side of training an energy-based reference (no GPU): the formulas of sdeng_tilted_vjp and engine.tilted_param_grads pinned by a
float64 restatement without autograd against the reference's own float64 parameter gradients (tests/golden/tilted_train_*.npz,
gen_golden_tilted_train.py); the new C ABI entry points and their refusals; the param_grads opt-in; the trainer's argument checks."""
import ctypes
import os
import re

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.additions import ebm_mle
from tests import tilted_cases as tc
from tests import tilted_train_ref as tr
from tests.test_tilted_cpu import P, _desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDING = 2.0 ** -23  # the fixtures hold float64 gradients rounded to float32


@pytest.mark.parametrize("case", tr.CASES)
def test_float64_restatement_reproduces_the_reference_gradients(case):
    """Per-row arrays from the written-out forward and backward pass, multiplied out by engine.tilted_param_grads: every parameter
    gradient of L = sum w E + 0.1 mean(E^2) equals the reference's float64 autograd result to the fixture's own rounding."""
    fx = tr.TrainFixture(case)
    _, grads = tr.restated_param_grads(case)
    assert sorted(grads) == sorted(fx.grads) == sorted(fx.meta["names"])
    for name, want in fx.grads.items():
        got = grads[name]
        assert got.shape == want.shape and got.dtype == torch.float64
        assert tr.tensor_err(got, want) <= ROUNDING, (name, tr.tensor_err(got, want))
        if case == "f" and not name.startswith("base_model.out_layer."):  # zero last layer: nothing reaches the layers below it
            assert float(want.abs().max()) == 0.0 and float(got.abs().max()) == 0.0, name
    if case == "f":
        assert float(fx.grads["base_model.out_layer.weight"].abs().max()) > 0.0
    # the stored yardstick is a float32 run's error, per tensor
    assert set(fx.err32) == set(fx.grads) and all(0.0 <= v < 1e-4 for v in fx.err32.values()) and max(fx.err32.values()) > 1e-8


def test_cotangent_is_the_derivative_of_the_loss():
    E_ = torch.randn(9, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    w = tr.weights("a", 9)
    (g,) = torch.autograd.grad(tr.loss_of(E_, w), E_)
    assert torch.allclose(g, tr.cotangent(E_.detach(), w), rtol=1e-14, atol=0.0)


def test_exports_and_header():
    header = open(os.path.join(ROOT, "include", "sdeng.h")).read()
    assert re.search(r"\bsdeng_tilted_vjp\(const sdeng_tilted\* desc, const sdeng_tilted_rows\* rows, void\* stream\)", header)
    assert re.search(r"\bsdeng_tilted_vjp_workspace_bytes\(const sdeng_tilted\* desc\)", header)
    assert re.search(r"typedef struct sdeng_tilted_rows \{ float \*a\[5\], \*d\[5\]; float \*xs, \*dv; \} sdeng_tilted_rows;", header)
    assert "reparam.py:426-451" in header and "ebm_mle.py:735-771" in header


def _rows(over=None):
    r = L.TiltedRows()
    for l in range(5):
        r.a[l] = r.d[l] = P
    r.xs = r.dv = P
    for k, v in (over or {}).items():
        if isinstance(k, tuple):
            getattr(r, k[0])[k[1]] = v
        else:
            setattr(r, k, v)
    return r


def _refused(d, r):
    lib = L.lib()
    rc = lib.sdeng_tilted_vjp(ctypes.byref(d), ctypes.byref(r) if r is not None else None, None)
    return rc, lib.sdeng_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(abi_version=3), "ABI version 3"), (dict(d=0), "d = 0"), (dict(d=129), "d = 129"), (dict(k=0), "k = 0"), (dict(k=17), "k = 17"),
    (dict(M=47), "M = 47"), (dict(n_times=0, M=0), "M = 0"), (dict(x=None), "null pointer"), (dict(tinfo=None), "null pointer"),
    (dict(w_out=None), "null pointer"), (dict(mean_gauss=None), "null pointer"), (dict(full_cov=1), "eigvecs"),
])
def test_invalid_descriptors_are_refused_before_any_launch(over, word):
    d = _desc(**over)
    rc, msg = _refused(d, _rows())
    assert rc == L.E_INVALID and word in msg, (rc, msg)
    assert L.lib().sdeng_tilted_vjp_workspace_bytes(ctypes.byref(d)) == 0


@pytest.mark.parametrize("over,word", [
    (dict(num_layers=4), "num_layers=4"), (dict(channels=64), "channels=64"), (dict(tilt_type=L.TILT_SQ_NORM), "'dot'"),
    (dict(tilt_type=L.TILT_SUM), "'dot'"), (dict(use_scaling_factor=1), "use_scaling_factor"),
])
def test_unsupported_descriptors_name_their_reason(over, word):
    d = _desc(**over)
    rc, msg = _refused(d, _rows())
    assert rc == L.E_UNSUPPORTED and word in msg, (rc, msg)
    assert L.lib().sdeng_tilted_vjp_workspace_bytes(ctypes.byref(d)) == 0


@pytest.mark.parametrize("over,word", [(None, "null rows")] +
                         [({("a", l): None}, f"a[{l}]") for l in range(5)] + [({("d", l): None}, f"d[{l}]") for l in range(5)] +
                         [(dict(xs=None), "rows->xs"), (dict(dv=None), "rows->dv")])
def test_every_rows_pointer_is_checked_before_any_launch(over, word):
    rc, msg = _refused(_desc(), None if over is None else _rows(over))
    assert rc == L.E_INVALID and word in msg, (rc, msg)


def test_valid_descriptor_stops_at_the_workspace():
    """The workspace is that of an evaluation with grad, whether or not log_prob and grad are asked for; without one the call ends
    with SDENG_E_WORKSPACE, before any launch."""
    lib = L.lib()
    want = lib.sdeng_tilted_eval_workspace_bytes(ctypes.byref(_desc()))
    for d in (_desc(), _desc(grad=None), _desc(log_prob=None, grad=None)):
        assert lib.sdeng_tilted_vjp_workspace_bytes(ctypes.byref(d)) == want
        assert _refused(d, _rows())[0] == L.E_WORKSPACE
    full = _desc(full_cov=1, eigvecs=P, grad=None)
    assert lib.sdeng_tilted_vjp_workspace_bytes(ctypes.byref(full)) - want == 2 * 3 * 65536


def test_opt_in():
    fx, net = tc.mirror("a")
    t, x = fx["t"], fx["x"]
    assert type(net).param_grads is False and net.param_grads is False
    with pytest.raises(E.UnsupportedByEngine, match="parameters") as info:  # the default: as before, and the message names the switch
        net.energy(t, x)
    assert "param_grads" in str(info.value)
    net.param_grads = True
    for call in (lambda: net.energy(t, x), lambda: net.unnorm_log_prob(t, x)):
        with pytest.raises(RuntimeError, match="MI355X"):  # no CPU path
            call()
    for call in (lambda: net.unnorm_log_prob_and_grad(t, x), lambda: net(t, x)):  # the score's parameter gradients are second order
        with pytest.raises(E.UnsupportedByEngine, match="parameters"):
            call()
    with pytest.raises(E.UnsupportedByEngine, match="scaling_factor"):
        net.energy(t, x, scaling_factor=2.0)
    with pytest.raises(RuntimeError, match="MI355X"):  # frozen parameters, x wants a gradient: the graph goes to x alone
        net.requires_grad_(False).energy(t, x.clone().requires_grad_(True))


def _trainer(sampler_type, **kw):
    from sde_sampler_lrds_amd.distr.gauss import Gauss
    fx, net = tc.mirror("a")
    return ebm_mle.MaximumLikelihoodEBM(net.sde, Gauss(dim=2, loc=0.0, scale=1.0), net, sampler_type, n_steps=2, **kw), net


def test_trainer_argument_checks():
    data = torch.zeros(8, 2)
    with pytest.raises(ValueError, match="n_accumulation_steps"):
        _trainer("cd")[0].train(data, 8, 1, n_accumulation_steps=2, verbose=False)
    with pytest.raises(NotImplementedError, match="Loss scaling"):
        _trainer("cd")[0].train(data, 8, 1, reweight_loss=True, verbose=False)
    with pytest.raises(NotImplementedError, match="x_init"):
        _trainer("smc_pdds")[0].train(data, 8, 1, verbose=False)
    with pytest.raises(NotImplementedError, match="not found"):
        _trainer("hmc")[0].train(data, 8, 1, verbose=False)
    mle, net = _trainer("annealed_mcmc")
    assert mle.times.shape == (3, 1) and mle.net is net and mle.use_precond is False
    with pytest.raises(RuntimeError, match="MI355X"):  # past the checks: training needs the GPU
        mle.train(data, 8, 1, verbose=False)
    assert net.param_grads is False
