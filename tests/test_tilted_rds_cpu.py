"""Host side of RDS over an energy-based ('nn') reference (no GPU): the route decisions, make_model / change_reference_type / state_dict,
the refusals and their reasons, the C ABI's exports and its refusals before any launch -- and the recursion the kernel is specified by,
restated in float64 (tests/tilted_ref.Restated for the score, the torch control in double, the coefficient rows of engine.coef_table in
double) and held to the reference's own float64 runs in tests/golden/rds_nn_*.npz."""
import copy
import ctypes
import math
import os
import re

import pytest
import torch

from oracle import sde_oracle as orc
from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd import routes as R
from sde_sampler_lrds_amd.experiments import benchmark_utils as bu
from tests import rds_nn_cases as rc
from tests import tilted_cases as tc
from tests import tilted_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = dict(train_steps=10, train_batch_size=8, eval_batch_size=16)
F64 = torch.float64


def _model(integrator="ei", loss_type="lv", model_type="base_zero_init", case="a", **kw):
    net = tc.mirror(case)[1]
    target = bu.make_target_details("many_modes", dim=net.dim, n_modes=3)
    return bu.make_model("vp-ref", "nn", loss_type, integrator, model_type, "snr" if integrator == "ddpm_like" else "uniform",
                         dict(net=net, sigma=1.0, **kw), target, TRAIN, n_steps=4, device="cpu"), net


# ---- routes ------------------------------------------------------------------------------------------------------------------------------
def test_resolve_reference_recognises_a_tilted_potential():
    model, net = _model()
    kind, utils = E.resolve_reference(model.reference_ctrl)
    assert kind == "nn" and utils["net"] is net
    assert R.diagonal_reference("nn", utils) is False
    assert R.lv_route(model.loss)[0] == "fused"  # log-variance training of the ClippedCtrl: no new training code
    with pytest.raises(E.UnsupportedByEngine, match="second order in the energy net"):
        R.kl_route(model.loss, model.reference_ctrl)


def test_other_nets_stay_refused_with_the_reason():
    class Rds:
        reference_distr_utils = dict(net=torch.nn.Linear(2, 2))

        def reference_ctrl(self, t, x):
            return x
    with pytest.raises(E.UnsupportedByEngine, match="Linear needs autograd inside the step"):
        E.resolve_reference(Rds().reference_ctrl)


# ---- the public interface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["em", "ei", "ddpm_like"])
def test_make_model_builds_on_the_cpu(integrator):
    model, net = _model(integrator)
    assert model.ref_type == "nn" and model.reference_distr_utils == {"net": net}
    assert not any(p.requires_grad for p in net.parameters())  # solver/oc.py:579-580
    assert type(model.reference_distr).__name__ == "WrapperDistrNN" and model.reference_distr.net is net
    assert float(model.reference_distr.t) == pytest.approx(1e-4 if integrator == "ddpm_like" else 0.0)  # eps: the start of the grid
    assert model.loss.reference_ctrl == model.reference_ctrl
    assert type(model.loss).__name__ == {"em": "EMReferenceSDELoss", "ei": "EIReferenceSDELoss", "ddpm_like": "DDPMLikeReferenceSDELoss"}[integrator]


def test_make_model_says_what_it_expects():
    target = bu.make_target_details("many_modes", dim=2, n_modes=3)
    for details, word in ((dict(sigma=1.0), "no net"), (dict(sigma=1.0, net=torch.nn.Linear(2, 2)), "got Linear")):
        with pytest.raises(E.UnsupportedByEngine, match="GMMTitledPotential / GaussTiltedPotential.*" + word):
            bu.make_model("vp-ref", "nn", "lv", "ei", "base_zero_init", "uniform", details, target, TRAIN, n_steps=4, device="cpu")
    model, _ = _model()
    with pytest.raises(E.UnsupportedByEngine, match="GMMTitledPotential / GaussTiltedPotential"):
        model.change_reference_type("nn", net=torch.nn.Linear(2, 2), eps=torch.tensor(0.0))
    with pytest.raises(ValueError, match="eps"):
        model.change_reference_type("nn", net=tc.mirror("a")[1])


def test_state_dict_round_trips_the_reference():
    model, net = _model()
    sd = model.state_dict()
    assert sd["ref_type"] == "nn" and sd["ref_net"] is net
    other, _ = _model()
    other.change_reference_type("gmm", weights=torch.ones(2), means=torch.zeros(2, 2), variances=torch.ones(2, 2))
    assert other.ref_type == "gmm"
    other.load_state_dict(sd)
    assert other.ref_type == "nn" and other.reference_distr_utils["net"] is net
    assert E.resolve_reference(other.loss.reference_ctrl)[0] == "nn"
    assert float(other.reference_distr.t) == float(other.train_timesteps()[0])


def test_kl_and_eubo_raise_with_their_reasons():
    ts, x = torch.linspace(0.0, 1.0, 5), torch.zeros(8, 2)
    model, _ = _model(loss_type="kl")
    with pytest.raises(E.UnsupportedByEngine, match="KL training differentiates the reference score: second order in the energy net"):
        model.loss(ts, x, model.clipped_target_unnorm_log_prob, model.reference_distr.log_prob)
    model, _ = _model()
    with pytest.raises(E.UnsupportedByEngine, match="compute_eubo over an energy-based"):
        model.loss.compute_eubo(ts, x, model.clipped_target_unnorm_log_prob, model.reference_distr.log_prob)
    model.loss.sde_ctrl_noise = 0.1
    with pytest.raises(E.UnsupportedByEngine, match="sde_ctrl_noise / sde_ctrl_dropout over an energy-based"):
        model.loss(ts, x, model.clipped_target_unnorm_log_prob, model.reference_distr.log_prob)
    model, _ = _model(model_type="target_informed_zero_init")  # a ScoreCtrl
    with pytest.raises(E.UnsupportedByEngine, match="ScoreCtrl over an energy-based"):
        model.loss(ts, x, model.clipped_target_unnorm_log_prob, model.reference_distr.log_prob)
    with pytest.raises(E.UnsupportedByEngine, match="ScoreCtrl over an energy-based"):
        model.loss.compute_eubo(ts, x, model.clipped_target_unnorm_log_prob, model.reference_distr.log_prob)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports():
    header = open(os.path.join(ROOT, "include", "sdeng.h")).read()
    assert re.search(r"int sdeng_tilted_simulate\(const sdeng_tilted\* ref, const sdeng_tilted_rds\* run, void\* stream\);", header)
    assert re.search(r"size_t sdeng_tilted_simulate_workspace_bytes\(const sdeng_tilted\* ref, const sdeng_tilted_rds\* run\);", header)
    assert "typedef struct sdeng_tilted_rds {" in header and "solver/oc.py:577-592" in header and "losses/oc.py:444-510" in header
    body = re.search(r"typedef struct sdeng_tilted_rds \{(.*?)\} sdeng_tilted_rds;", re.sub(r"/\*.*?\*/", " ", header, flags=re.S), re.S)[1]
    declared = re.findall(r"[\s*](\w+)\s*[;,]", body)
    assert [n for n, _ in L.TiltedRds._fields_] == declared  # the binding's struct is the header's, field for field
    assert L.TiltedRds.net.size == ctypes.sizeof(L.Net) and L.ABI_VERSION == 4
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "sdeng_tilted_simulate") and hasattr(lib, "sdeng_tilted_simulate_workspace_bytes")
    assert {"sdeng_tilted_simulate", "sdeng_tilted_simulate_workspace_bytes"} <= set(L.EXPORTS)


_HOST = ctypes.create_string_buffer(64)
P = ctypes.addressof(_HOST)  # a non-null address, never dereferenced: a refused call launches nothing


def _ref(**over):
    d = L.Tilted()
    d.abi_version, d.M, d.n_times, d.rows_per_time, d.d, d.k = L.ABI_VERSION, 37, 8, 0, 16, 3
    d.num_layers, d.channels, d.tilt_type = 6, 128, L.TILT_DOT
    for n in ("tinfo", "w_in", "b_in", "w_out", "b_out", "te_coeff", "te_phase", "te_w1", "te_b1", "te_w2", "te_b2", "mean_gauss", "var_gauss",
              "weights", "means", "vars"):
        setattr(d, n, P)
    for i in range(4):
        d.w_h[i] = d.b_h[i] = P
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _run(**over):
    r = L.TiltedRds()
    r.form, r.flags, r.N = L.FORM_LIN, L.FLAG_ITO, 8
    for n in ("coef", "x_in", "x_out", "rnd_out"):
        setattr(r, n, P)
    net = r.net
    net.ctrl_kind = L.CTRL_CLIPPED
    for n in ("w_in", "b_in", "w_h1", "b_h1", "w_h2", "b_h2", "w_out", "b_out"):
        setattr(net, n, P)
    te = net.t_embed
    te.coeff = te.phase = te.w_out = te.b_out = P
    te.w[0] = te.b[0] = P
    te.n_hidden, te.dim_out = 1, 64
    for k, v in over.items():
        if k == "ctrl_kind":
            r.net.ctrl_kind = v
        else:
            setattr(r, k, v)
    return r


def _refused(ref, run):
    lib = L.lib()
    rc_ = lib.sdeng_tilted_simulate(ctypes.byref(ref), ctypes.byref(run) if run is not None else None, None)
    assert lib.sdeng_tilted_simulate_workspace_bytes(ctypes.byref(ref), ctypes.byref(run) if run is not None else None) == 0
    return rc_, lib.sdeng_last_error().decode()


@pytest.mark.parametrize("ref,run,word", [
    (dict(abi_version=3), {}, "ABI version 3"), (dict(d=129), {}, "d = 129"), (dict(k=17), {}, "k = 17"), (dict(M=0), {}, "M = 0"),
    (dict(tinfo=None), {}, "null pointer"), (dict(w_out=None), {}, "null pointer"), (dict(full_cov=1), {}, "eigvecs"),
    ({}, None, "null run"), ({}, dict(x_in=None), "required"), ({}, dict(rnd_out=None), "required"), ({}, dict(coef=None), "required"),
    ({}, dict(N=0), "N = 0"), ({}, dict(N=7), "N = 7"),
])
def test_invalid_calls_are_refused_before_any_launch(ref, run, word):
    code, msg = _refused(_ref(**ref), None if run is None else _run(**run))
    assert code == L.E_INVALID and word in msg, (code, msg)


@pytest.mark.parametrize("ref,run,word", [
    (dict(num_layers=4), {}, "num_layers=4"), (dict(tilt_type=L.TILT_SUM), {}, "'dot'"), (dict(use_scaling_factor=1), {}, "use_scaling_factor"),
    ({}, dict(ctrl_kind=L.CTRL_SCORE), "ClippedCtrl"), ({}, dict(ctrl_kind=L.CTRL_CANCEL_DRIFT), "ClippedCtrl"),
    ({}, dict(form=L.FORM_EUBO), "SDENG_FORM_LIN and SDENG_FORM_EM only"), ({}, dict(form=L.FORM_CMCD), "SDENG_FORM_LIN and SDENG_FORM_EM only"),
    ({}, dict(flags=L.FLAG_ITO | L.FLAG_REMOVE_REF), "REMOVE_REF"), ({}, dict(flags=L.FLAG_CTRL_NOISE), "CTRL_NOISE"),
    ({}, dict(flags=L.FLAG_CTRL_DROPOUT), "CTRL_DROPOUT"), ({}, dict(flags=L.FLAG_SPLIT_TILES), "SPLIT_TILES"),
])
def test_unsupported_calls_name_their_reason(ref, run, word):
    code, msg = _refused(_ref(**ref), _run(**run))
    assert code == L.E_UNSUPPORTED and word in msg, (code, msg)


def test_valid_call_stops_at_the_workspace():
    """The rows_per_time, x, log_prob and grad of the reference's descriptor are ignored; the size grows by the per-launch pieces; the
    packed images stay where sdeng_tilted_eval keeps them."""
    lib = L.lib()
    ref, run = _ref(), _run()
    need = lib.sdeng_tilted_simulate_workspace_bytes(ctypes.byref(ref), ctypes.byref(run))
    ev = _ref(rows_per_time=37, n_times=1, x=P, grad=P)
    base = lib.sdeng_tilted_eval_workspace_bytes(ctypes.byref(ev))
    rows = 4 * ((37 * 16 + 63) // 64 * 64)
    assert need > base and need - base >= 3 * rows + 8 * (64 + 128) * 4
    assert lib.sdeng_tilted_simulate(ctypes.byref(ref), ctypes.byref(run), None) == L.E_WORKSPACE
    assert lib.sdeng_tilted_simulate_workspace_bytes(ctypes.byref(_ref()), ctypes.byref(_run(form=L.FORM_EM, flags=0))) == need


# ---- the recursion, in float64 ---------------------------------------------------------------------------------------------------------------
def coef64(kind, ts, sde):
    """The rows [N, 7] of engine.coef_table(kind, ts, sde, with_ref=True) evaluated in float64: the same expressions (engine._transition_gains and
    the SDE's own methods) on the float32 numbers of the grid and of the SDE's buffers."""
    ts, sde = ts.to(F64), copy.deepcopy(sde).double()
    T, rows = ts[-1], []
    for s, t in zip(ts[:-1], ts[1:]):
        tau = T - s
        if kind in ("ei", "ddpm"):
            omega = sde.omega_ddpm(s, t) if kind == "ddpm" else sde.omega(s, t)
            g1, g2, g3 = E._transition_gains(sde, s, t, kind == "ddpm")
            rows.append([tau, g1, g2, g3, 0.5 * omega, torch.sqrt(omega), 0.0])
        else:
            g, dt = sde.diff(tau, None), t - s
            rows.append([tau, -sde.drift_coeff_t(tau), g, torch.square(g), dt, dt.sqrt(), 0.0])
    return torch.tensor([[float(torch.as_tensor(v).reshape(-1)[0]) for v in r] for r in rows], dtype=F64)


def restated_run(fx, coef=None, noise=None):
    """x_N, rnd, xs of the recursion include/sdeng.h states for sdeng_tilted_simulate, in float64, terminal costs included."""
    spec, kind = fx.spec, rc.KIND[fx.spec["integrator"]]
    net64, ctrl = tilted_ref.from_fixture(tc.Fixture(spec["tilted"])), fx.ctrl(F64)
    sde = tc.make_sde(__import__("sde_sampler_lrds_amd.eq.sdes", fromlist=["x"]), tc.Fixture(spec["tilted"]).spec["sde"])
    coef = coef64(kind, fx["ts"], sde) if coef is None else coef
    x, rnd, xs = fx["x0"].to(F64), torch.zeros(fx["x0"].shape[0], dtype=F64), [fx["x0"].to(F64)]
    with torch.no_grad():
        for k, (t, c1, c2, c3, c4, c5, c6) in enumerate(coef.tolist()):
            tt = torch.tensor(t, dtype=F64)
            ref = net64(tt, x)[1]
            u = ctrl(tt, x)
            z = (orc.philox_normal(spec["seed"], k, 0, x.shape[0], x.shape[1]) if noise is None else noise[k]).to(F64)
            if kind == "em":
                rnd = rnd + 0.5 * (u * u).sum(-1) * c4 + (u * (c5 * z)).sum(-1) + c6
                x = x + ((c1 * x + c3 * ref) + c2 * u) * c4 + c2 * (c5 * z)
            else:
                rnd = rnd + c4 * (u * u).sum(-1) + c5 * (u * z).sum(-1) + c6
                x = (c1 * x + c2 * (u + ref)) + c3 * z
            xs.append(x)
        ref_lp = net64(fx["ts"][0].to(F64), x, want_grad=False)[0]
        rnd = rnd + ref_lp - gmm_log_prob64(fx, x)
    return x, rnd, torch.stack(xs)


def gmm_log_prob64(fx, x):
    loc, scale, w = fx["tgt_loc"].to(F64), fx["tgt_scale"].to(F64), fx["tgt_w"].to(F64)
    z = (x.unsqueeze(1) - loc) / scale
    lp = torch.log(w / w.sum()) - 0.5 * (z * z).sum(-1) - torch.log(scale).sum(-1) - 0.5 * x.shape[1] * math.log(2.0 * math.pi)
    return torch.logsumexp(lp, dim=-1)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_float64_restatement_reproduces_the_reference(name):
    fx = rc.Fixture(name)
    assert (fx.meta["B"], fx.meta["N"]) == (rc.B, rc.N) and torch.equal(fx["ts"], rc.grid(fx.spec))
    x, rnd, xs = restated_run(fx)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    assert rel(x, fx["out.x64"]) < 1e-9 and rel(xs, fx["out.xs64"]) < 1e-9 and rel(rnd, fx["out.rnd64"]) < 1e-9
    # the stored float32 run is the yardstick of the GPU test: a float32 run, within the generator's condition, on a bounded trajectory
    assert fx["out.x32"].dtype == torch.float32 and fx["out.x64"].dtype == F64
    assert 1e-9 < fx.meta["err32_x"] <= 1e-3 and 1e-9 < fx.meta["err32_rnd"] <= 1e-3 and float(fx["out.xs64"].abs().max()) <= 100.0
    assert tc.err(fx["out.x32"], fx["out.x64"]) == pytest.approx(fx.meta["err32_x"])


@pytest.mark.parametrize("name", list(rc.CASES))
def test_float64_rows_are_the_engines_table(name):
    """The float64 rows above are engine.coef_table's: equal to fp32 round-off of the entries (the table is made of float32 scalars)."""
    fx = rc.Fixture(name)
    sde = fx.net().sde
    table = E.coef_table(rc.KIND[fx.spec["integrator"]], fx["ts"], sde, with_ref=True)
    rows = coef64(rc.KIND[fx.spec["integrator"]], fx["ts"], sde)
    assert torch.allclose(table[:, :7].double(), rows, rtol=2e-5, atol=1e-7)
    tinfo = E.tilted_times(fx.net(), table[:, 0], table.shape[0], per_row=True)
    assert tinfo[:2] == (rc.N, 1) and torch.equal(tinfo[2][:, 0], table[:, 0])
    if name == "c_ei":  # t_limit above the last step's time: that row's prior is noised to t_limit, not to t
        assert not torch.equal(tinfo[2][-1, 3:], tinfo[2][-1, 1:3]) and torch.equal(tinfo[2][0, 3:], tinfo[2][0, 1:3])
