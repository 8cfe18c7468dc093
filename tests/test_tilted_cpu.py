"""Host side of the energy-based (tilted-potential) references (no GPU): the formulas the kernel implements, pinned by a float64
restatement against the reference's own float64 outputs (tests/golden/tilted_*.npz, gen_golden_tilted.py); the descriptor compiled from
the mirror classes and from the reference's objects; the state_dict contract; the C ABI's exports and its refusals."""
import ctypes
import os
import re

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from tests import tilted_cases as tc
from tests import tilted_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(tc.CASES)


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference(case):
    """Forward pass, analytic J^T xs and noised prior in float64 against the reference's float64 run (autograd, its own prior code): far
    below the float32 round-off the GPU test measures against, so the restatement -- and with it the kernel's formulas -- is pinned."""
    fx = tc.Fixture(case)
    lp, grad = tilted_ref.from_fixture(fx)(fx["t"], fx["x"])
    assert tc.err(lp, fx["out.lp64"]) < 1e-11 and tc.err(grad, fx["out.grad64"]) < 1e-10
    lp_only, none = tilted_ref.from_fixture(fx)(fx["t"], fx["x"], want_grad=False)
    assert none is None and torch.equal(lp_only, lp)
    # the stored float32 run is the yardstick of the GPU test: it must be a float32 run, not a copy of the float64 one
    assert fx["out.lp32"].dtype == torch.float32 and 1e-9 < fx.meta["err32_lp"] < 1e-5 and 1e-9 < fx.meta["err32_grad"] < 1e-4


def test_zero_last_layer_leaves_the_prior():
    fx = tc.Fixture("f")
    r = tilted_ref.from_fixture(fx)
    plp, pgrad = r.prior(fx["t"].double(), fx["x"].double())
    assert tc.err(plp, fx["out.lp64"]) < 1e-12 and tc.err(pgrad, fx["out.grad64"]) < 1e-12


@pytest.mark.parametrize("case", CASES)
def test_state_dict_contract(case):
    """Same buffer and parameter names as the reference: the stored key list, and the stored state_dict loads (strict)."""
    fx, net = tc.mirror(case)
    keys = tc.Fixture(fx.meta.get("base", case)).meta["keys"]
    assert list(net.state_dict().keys()) == keys
    fresh = tc.build(fx.spec, *_mods())
    fresh.load_state_dict(fx.state_dict(), strict=True)
    for k, v in fx.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v), k
    for name in ("energy", "unnorm_log_prob", "unnorm_log_prob_and_grad", "forward", "sample_prior", "get_gmm_params"):
        assert callable(getattr(net, name))
    assert net.has_unnorm_log_prob_and_grad is True and net.has_sample_prior is True


def _mods():
    from sde_sampler_lrds_amd.eq import sdes
    from sde_sampler_lrds_amd.models import mlp, reparam
    return mlp, reparam, sdes


def test_mirror_moments_and_prior_sampling():
    """mean_gauss / var_gauss computed by the mirror's constructor equal the reference's stored buffers; sample_prior and get_gmm_params
    run on the host."""
    for case in ("a", "b", "c", "d"):
        fx = tc.Fixture(case)
        net = tc.build(fx.spec, *_mods(), fx.ctor_args())
        sd = fx.state_dict()
        assert torch.allclose(net.mean_gauss, sd["mean_gauss"], rtol=1e-5, atol=1e-6)
        assert torch.allclose(net.var_gauss, sd["var_gauss"], rtol=1e-5, atol=1e-6)
        torch.manual_seed(0)
        xs = net.sample_prior(torch.full((7, 1), 0.4))
        assert xs.shape == (7, fx.spec["d"]) and torch.isfinite(xs).all()
        w, m, v = net.get_gmm_params(torch.tensor(0.4))
        assert m.shape == (fx.spec["K"], fx.spec["d"])


def _fields(d):
    return {n: getattr(d, n) for n, _ in L.Tilted._fields_ if n in ("abi_version", "d", "k", "full_cov", "num_layers", "channels", "tilt_type",
                                                                      "use_scaling_factor", "use_s_t_scaling")}


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_descriptor_from_mirror_and_from_reference_objects(case):
    """engine.tilted_desc recognises the reference's own objects by class name and attributes (stood in for by foreign classes of the
    same names, as tests/test_host_cpu.py does): same scalar fields, same arrays in the same order."""
    from tests.test_host_cpu import _foreign
    fx, net = tc.mirror(case)
    theirs = _foreign(net)
    theirs.base_model = _foreign(net.base_model)
    theirs.base_model.timestep_embed = _foreign(net.base_model.timestep_embed)
    theirs.sde = _foreign(net.sde)
    assert not isinstance(theirs, type(net)) and type(theirs).__name__ == type(net).__name__
    keep_a, keep_b = [], []
    da, db = E.tilted_desc(net, torch.device("cpu"), keep_a), E.tilted_desc(theirs, torch.device("cpu"), keep_b)
    spec = fx.spec
    assert _fields(da) == _fields(db) == dict(abi_version=L.ABI_VERSION, d=spec["d"], k=spec["K"], full_cov=int(spec["prior"] in ("eig", "cov")),
                                             num_layers=6, channels=128, tilt_type=L.TILT_DOT, use_scaling_factor=0,
                                             use_s_t_scaling=int(spec["st"]))
    assert len(keep_a) == len(keep_b) and all(torch.equal(u, v) for u, v in zip(keep_a, keep_b))
    assert bool(da.eigvecs) == (spec["prior"] in ("eig", "cov"))
    if spec["prior"] == "cov":  # covariance matrices are decomposed in float64: P diag(D) P^T gives them back
        D, P = keep_a[-2].double(), keep_a[-1].double()
        assert torch.allclose(torch.einsum("kia,ka,kja->kij", P, D, P), fx.ctor_args()[2].double(), atol=1e-6)
    n_times, B, tinfo = E.tilted_times(net, fx["t"], fx["t"].shape[0])
    assert (n_times, B) == (len(spec["times"]), spec["B"]) and tinfo.shape == (n_times, 5)
    s, sig = tilted_ref.sde_scalars(spec["sde"], tc.SDE_ARGS[spec["sde"]], torch.tensor(spec["times"]).reshape(-1, 1))
    assert torch.allclose(tinfo[:, 1:3].double(), torch.cat([s, sig], 1), rtol=1e-5)
    assert torch.equal(tinfo[:, 3:], tinfo[:, 1:3]) == (not any(t < spec["t_limit"] for t in spec["times"]))


def test_time_layouts():
    _, net = tc.mirror("a")
    assert E.tilted_times(net, torch.tensor(0.3), 40)[:2] == (1, 40)
    assert E.tilted_times(net, torch.tensor([[0.3]]), 40)[:2] == (1, 40)
    assert E.tilted_times(net, torch.tensor([0.1, 0.1, 0.2, 0.2, 0.1, 0.1]), 6)[:2] == (3, 2)
    assert E.tilted_times(net, torch.tensor([0.1, 0.1, 0.2, 0.3, 0.3, 0.3]), 6)[:2] == (6, 1)  # runs of unequal length: every row its own time
    assert E.tilted_times(net, torch.arange(5) / 10.0, 5)[:2] == (5, 1)
    with pytest.raises(ValueError):
        E.tilted_times(net, torch.zeros(3), 5)


def test_exports_and_header():
    header = open(os.path.join(ROOT, "include", "sdeng.h")).read()
    for sym in ("sdeng_tilted_eval", "sdeng_tilted_eval_workspace_bytes"):
        assert re.search(r"\b" + sym + r"\(const sdeng_tilted\* desc", header)
    assert "models/reparam.py:277-520" in header and "models/mlp.py:57-143" in header


_HOST = ctypes.create_string_buffer(64)
P = ctypes.addressof(_HOST)  # a non-null address, never dereferenced: a refused descriptor launches nothing


def _desc(**over):
    d = L.Tilted()
    d.abi_version, d.M, d.n_times, d.rows_per_time, d.d, d.k = L.ABI_VERSION, 48, 2, 24, 16, 3
    d.num_layers, d.channels, d.tilt_type = 6, 128, L.TILT_DOT
    for n in ("x", "tinfo", "w_in", "b_in", "w_out", "b_out", "te_coeff", "te_phase", "te_w1", "te_b1", "te_w2", "te_b2", "mean_gauss",
              "var_gauss", "weights", "means", "vars", "log_prob", "grad"):
        setattr(d, n, P)
    for i in range(4):
        d.w_h[i] = d.b_h[i] = P
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _refused(d):
    lib = L.lib()
    rc = lib.sdeng_tilted_eval(ctypes.byref(d), None)
    assert lib.sdeng_tilted_eval_workspace_bytes(ctypes.byref(d)) == 0
    return rc, lib.sdeng_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(abi_version=3), "ABI version 3"), (dict(d=0), "d = 0"), (dict(d=129), "d = 129"), (dict(k=0), "k = 0"), (dict(k=17), "k = 17"),
    (dict(M=47), "M = 47"), (dict(n_times=0, M=0), "M = 0"), (dict(x=None), "null pointer"), (dict(tinfo=None), "null pointer"),
    (dict(w_out=None), "null pointer"), (dict(mean_gauss=None), "null pointer"), (dict(full_cov=1), "eigvecs"),
    (dict(log_prob=None, grad=None), "nothing to compute"),
])
def test_invalid_descriptors_are_refused_before_any_launch(over, word):
    rc, msg = _refused(_desc(**over))
    assert rc == L.E_INVALID and word in msg, (rc, msg)


@pytest.mark.parametrize("over,word", [
    (dict(num_layers=4), "num_layers=4"), (dict(channels=64), "channels=64"), (dict(tilt_type=L.TILT_SQ_NORM), "'dot'"),
    (dict(tilt_type=L.TILT_SUM), "'dot'"), (dict(use_scaling_factor=1), "use_scaling_factor"),
])
def test_unsupported_descriptors_name_their_reason(over, word):
    rc, msg = _refused(_desc(**over))
    assert rc == L.E_UNSUPPORTED and word in msg, (rc, msg)


def test_valid_descriptor_stops_at_the_workspace():
    """Accepted descriptors: the size is reported (images, constants and -- with a gradient -- the pre-activations of every wave), and a
    call without a workspace ends with SDENG_E_WORKSPACE, still before any launch."""
    lib = L.lib()
    with_grad, without = _desc(), _desc(grad=None)
    a, b = lib.sdeng_tilted_eval_workspace_bytes(ctypes.byref(with_grad)), lib.sdeng_tilted_eval_workspace_bytes(ctypes.byref(without))
    assert a - b == 3 * 40960 and b > 15 * 65536  # three 16-row tiles, one wave each; 15 net images
    full = _desc(full_cov=1, eigvecs=P)
    assert lib.sdeng_tilted_eval_workspace_bytes(ctypes.byref(full)) - a == 2 * 3 * 65536
    assert lib.sdeng_tilted_eval(ctypes.byref(with_grad), None) == L.E_WORKSPACE


def test_trainable_parameters_in_grad_mode_raise():
    """No torch fallback: a call that would need gradients with respect to the net's parameters is refused, on any device."""
    fx, net = tc.mirror("a")
    assert any(p.requires_grad for p in net.parameters())
    for call in (lambda: net.unnorm_log_prob_and_grad(fx["t"], fx["x"]), lambda: net(fx["t"], fx["x"]), lambda: net.energy(fx["t"], fx["x"]),
                 lambda: net.unnorm_log_prob(fx["t"], fx["x"])):
        with pytest.raises(E.UnsupportedByEngine, match="parameters"):
            call()
    with pytest.raises(E.UnsupportedByEngine, match="scaling_factor"):
        net.unnorm_log_prob(fx["t"], fx["x"], scaling_factor=2.0)
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):  # past that check: the evaluation itself needs the GPU
        net.unnorm_log_prob(fx["t"], fx["x"])


def test_still_out_of_scope():
    """The step-loop 'nn' reference is the next step: resolve_reference keeps raising on it."""
    class Rds:
        reference_distr_utils = dict(net=object())

        def reference_ctrl(self, t, x):
            return x
    with pytest.raises(E.UnsupportedByEngine):
        E.resolve_reference(Rds().reference_ctrl)
