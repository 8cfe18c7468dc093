"""The training routes, held to the record of what they were before ``routes.py`` said them once.  ``tests/golden/training_routes.json`` holds, for
every ``make_model`` combination the reference accepts on six targets (``tests/route_cases.py``), the log-variance route, the KL route and the
capturable flag the scattered predicates of the parent commit gave (``tests/golden/gen_training_routes.py``).  CPU only: models are built, route
functions asked, the C entries called up to the NULL workspace -- nothing is launched."""
import itertools
import json
import os

import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd import routes as R
from sde_sampler_lrds_amd.losses import oc
from sde_sampler_lrds_amd.losses import training as T
from tests import route_cases as rc

FIXTURE = json.load(open(os.path.join(rc.GOLDEN, "training_routes.json")))
LETTER = {"fused": "f", "graphed": "g", "eager": "e", "native": "n", "stepwise": "s"}


def kl_route(loss):
    """The KL route of a loss as its own ``__call__`` asks for it: the RDS losses hand ``_kl_loss`` their reference drift, the others none."""
    if isinstance(loss, oc.ControlledLangevinSDELoss):
        return R.cmcd_kl_route(loss)
    with_ref = isinstance(loss, oc.EMReferenceSDELoss) and E.resolve_reference(loss.reference_ctrl)[0] != "none"
    return R.kl_route(loss, loss.reference_ctrl if with_ref else None)


def capturable(loss):
    return R.graph_capturable(loss.generative_ctrl, *([loss.sde.target_score] if isinstance(loss, oc.ControlledLangevinSDELoss) else []))


def outcome(loss):
    lv = kl = ""
    flags = loss.fused_training, loss.graph_training, loss.native_adjoint
    for a, b in rc.SETTINGS:
        loss.fused_training, loss.graph_training = a, b
        lv += LETTER[R.lv_route(loss)[0]]
        loss.native_adjoint, loss.fused_training = a, b
        kl += LETTER[kl_route(loss)]
    loss.fused_training, loss.graph_training, loss.native_adjoint = flags
    return f"{lv}/{kl}/{int(capturable(loss))}"


@pytest.fixture(scope="module")
def models():
    """Every model of the fixture, built once: {key: solver}."""
    rc.register_sonar()
    built = {}
    for target in rc.TARGETS:
        for kw in rc.grid_ok():
            model = rc.build(target, kw)
            if model is not None:
                built[rc.key_of(target, kw)] = model
    return built


def test_every_route_is_the_recorded_one(models):
    axes = FIXTURE["axes"]
    assert list(axes) == list(rc.AXES)
    expected = {key: FIXTURE["outcomes"][ord(ch) - ord("a")] for key, ch in zip(itertools.product(*axes.values()), FIXTURE["index"]) if ch != "."}
    assert set(models) == set(expected)  # what make_model builds or refuses is what it built or refused then
    wrong = [(key, expected[key], outcome(m.loss)) for key, m in models.items() if outcome(m.loss) != expected[key]]
    assert not wrong, f"{len(wrong)} of {len(expected)} models take another route, first: {wrong[0]}"
    assert len(models) == len(expected) == len(FIXTURE["index"]) - FIXTURE["index"].count(".") > 1000


def test_wrapped_controls_take_the_recorded_routes():
    """The peel: a RemoveReferenceCtrl trains log-variance through its score (an EMA copy inside it included) and KL step by step as a whole;
    a bare EMA copy stays on the torch paths."""
    rc.register_sonar()
    got = {name: outcome(loss) for name, loss in rc.wrapped_cases()}
    assert got == FIXTURE["wrapped"] and len(got) == 22
    assert {v.split("/")[0][2] for k, v in got.items() if k.endswith("remove_ref")} == {"f", "e"}  # the peel reaches the fused pass where the inner control does


def _one_per(models, what):
    seen = {}
    for key, m in models.items():
        seen.setdefault(what(key, m), m)
    return seen


def test_routes_and_predicates_touch_no_data(models, monkeypatch):
    """No route decision builds a descriptor, copies a tensor or reads one back (the parent's ``fused_training_ok`` built a throw-away
    descriptor of the target on every log-variance step, ``adjoint_ctrl_ok`` one of PhiFour)."""
    def refuse(*a, **k):
        raise AssertionError("a route decision touched tensor data")
    for owner, name in ((E, "_dev_f32"), (E, "scalar_of"), (torch.Tensor, "cpu")):
        monkeypatch.setattr(owner, name, refuse)
    picked = _one_per(models, lambda key, m: (key[0], R.describe_ctrl(m.loss.generative_ctrl).kind))
    assert {t for t, _ in picked} == set(rc.TARGETS)
    for m in picked.values():
        loss, ctrl = m.loss, m.loss.generative_ctrl
        assert outcome(loss)
        assert isinstance(T.fused_training_ok(ctrl), bool) and isinstance(E.adjoint_ctrl_ok(ctrl), bool) and isinstance(E.cmcd_adjoint_ok(loss), bool)
        assert isinstance(E.diagonal_reference(*E.resolve_reference(getattr(loss, "reference_ctrl", None))), bool)
        assert R.dist_kind(m.target, score_only=True) is not None


def test_native_means_the_c_entry_accepts(models, monkeypatch):
    """Where Python says 'native', sdeng_kl_adjoint / sdeng_cmcd_kl_adjoint validate the descriptor and select a kernel: the call stops at the NULL
    workspace (E_WORKSPACE), before any HIP call.  One model per (loss class, control kind, target kind, reference kind).  Graph-less targets
    (logistic regression) need a launch for their scores before the entry is reached and are left out."""
    class NoWorkspace:
        def get(self, nbytes, device):
            return torch.empty(0, dtype=torch.uint8)

    monkeypatch.setattr(E, "require_gpu", lambda x: None)
    monkeypatch.setattr(E, "_stream_ptr", lambda device: None)
    monkeypatch.setattr(E, "_WS", NoWorkspace())

    def case(key, m):
        loss = m.loss
        rec = R.describe_ctrl(loss.generative_ctrl)
        ref = E.ref_desc(*E.resolve_reference(getattr(loss, "reference_ctrl", None)), "cpu", []).kind
        return (type(loss).__name__, rec.kind, R.dist_kind(m.target, score_only=True), ref) if kl_route(loss) == "native" and R.dist_kind(m.target) not in R.GRAPHLESS_TARGETS else None
    picked = _one_per(models, case)
    picked.pop(None)
    assert len(picked) >= 12 and {c[0] for c in picked} >= {"ControlledLangevinSDELoss", "EMReferenceSDELoss", "EIReferenceSDELoss", "TimeReversalLoss"}
    B, N = 8, 4
    for c, m in picked.items():
        loss, d = m.loss, m.target.dim
        ctrl = loss.generative_ctrl
        w, lam = torch.full((B, 1), 1.0 / B), torch.zeros(B, d)
        with pytest.raises(L.EngineError) as err:
            if isinstance(loss, oc.ControlledLangevinSDELoss):
                E.cmcd_kl_adjoint(ctrl, loss.sde, torch.zeros(N + 1, L.NCOEF), torch.zeros(N + 1, B, d), torch.zeros(N, B, d), w, lam)
            else:
                E.kl_adjoint(ctrl, torch.zeros(N, L.NCOEF), torch.zeros(N, B, d), torch.zeros(N, B, d), w, lam, lin=loss.kind not in ("em", "time_reversal"), ito=True,
                             ref=E.resolve_reference(getattr(loss, "reference_ctrl", None)))
        assert err.value.code == L.E_WORKSPACE, (c, str(err.value))
