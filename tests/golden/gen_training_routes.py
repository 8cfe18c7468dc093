"""Which training route every ``make_model`` combination takes -> ``training_routes.json``.

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.gen_training_routes      (from the root of a checkout of commit c4634d2, with this
                                                                               script and tests/route_cases.py copied in: neither exists at that commit)

Run against commit c4634d2, the last one whose route decisions were spread over ``engine.py``, ``losses/oc.py`` and
``losses/training.py``.  This is a record of how the fixture was made, not a tool for later trees: the predicates it composes
(``fused_training_ok``, ``adjoint_ctrl_ok``, ``diagonal_reference``, ``cmcd_adjoint_ok``, ``_capturable``) are composed below exactly
as that commit's ``BaseOCLoss._integral_pass``, ``BaseOCLoss._kl_loss`` and ``ControlledLangevinSDELoss._kl_loss_cmcd`` compose them.
(``ControlledLangevinSDELoss.__call__`` never reaches ``_integral_pass``: its log-variance pass is the eager ``ctrl_batched``.)

The models are those of ``tests/route_cases.py``.  For each one the fixture holds, as one string "lv/kl/cap":
  lv   the log-variance route under (fused_training, graph_training) = (F,F) (F,T) (T,F) (T,T):  f fused | g graphed | e eager
  kl   the KL route under (native_adjoint, fused_training) = (F,F) (F,T) (T,F) (T,T):           n native | f fused | s stepwise
       (ControlledLangevinSDELoss: the CMCD route, native | stepwise)
  cap  1 when the stepwise adjoint step may be captured as a graph, else 0.
The fixture is data: the axes, the distinct outcomes and one character per point of the axes' product ('.' where ``make_model``
rejects the combination, or has no kernel to offer: UNet drift nets and 'nn' references).

``wrapped`` holds the same string for the hand-wrapped controls of ``route_cases.wrapped_cases`` (a RemoveReferenceCtrl, an EMA copy), which no
``make_model`` combination hands a loss.

Before writing, the script builds the full product over ``loss_type`` and ``time_type`` too and checks that neither changes an outcome,
which is why the fixture holds one value of each.
"""
from __future__ import annotations

import itertools
import json
import os

from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.losses import oc
from sde_sampler_lrds_amd.losses import training as T
from tests import route_cases as rc


def lv_route(loss):  # BaseOCLoss._integral_pass
    if isinstance(loss, oc.ControlledLangevinSDELoss):
        return "e"
    ctrl = E.unwrap_ctrl(loss.generative_ctrl)[0] if type(loss.generative_ctrl).__name__ == "RemoveReferenceCtrl" else loss.generative_ctrl
    if loss.fused_training and T.fused_training_ok(ctrl):
        return "f"
    if loss.graph_training and type(ctrl).__name__ == "ClippedCtrl" and type(getattr(ctrl, "base_model", None)).__name__ == "FourierMLP":
        return "g"
    return "e"


def kl_route(loss):
    ctrl = loss.generative_ctrl
    if isinstance(loss, oc.ControlledLangevinSDELoss):  # _kl_loss_cmcd
        return "n" if loss.native_adjoint and E.cmcd_adjoint_ok(loss) else "s"
    reference_ctrl = None  # what the loss's __call__ hands _kl_loss: EMReferenceSDELoss.__call__ for the RDS losses, None elsewhere
    if isinstance(loss, oc.EMReferenceSDELoss) and E.resolve_reference(loss.reference_ctrl)[0] != "none":
        reference_ctrl = loss.reference_ctrl
    ref_kind = E.resolve_reference(reference_ctrl) if reference_ctrl is not None else ("none", {})
    if loss.native_adjoint and E.adjoint_ctrl_ok(ctrl) and E.diagonal_reference(*ref_kind):
        return "n"
    if loss.fused_training and type(ctrl).__name__ == "ClippedCtrl" and type(getattr(ctrl, "base_model", None)).__name__ == "FourierMLP":
        return "f"
    return "s"


def capturable(loss):
    if isinstance(loss, oc.ControlledLangevinSDELoss):
        return T._capturable(loss.generative_ctrl, loss.sde.target_score)
    return T._capturable(loss.generative_ctrl)


def outcome(loss):
    lv, kl = "", ""
    for a, b in rc.SETTINGS:
        loss.fused_training, loss.graph_training = a, b
        lv += lv_route(loss)
        loss.native_adjoint, loss.fused_training = a, b
        kl += kl_route(loss)
    return f"{lv}/{kl}/{int(capturable(loss))}"


def main():
    rc.register_sonar()
    found = {}
    for target in rc.TARGETS:
        for kw in rc.grid_ok(collapse=False):
            model = rc.build(target, kw)
            if model is None:
                continue
            got = outcome(model.loss)
            assert found.setdefault(rc.key_of(target, kw), got) == got, ("loss_type / time_type changes a route", target, kw)
    kept = [rc.key_of(t, kw) for t in rc.TARGETS for kw in rc.grid_ok()]
    assert set(found) <= set(kept)
    values = {a: [] for a in rc.AXES}
    for key in kept:
        for a, v in zip(rc.AXES, key):
            if v not in values[a]:
                values[a].append(v)
    outcomes, index = [], ""
    for key in itertools.product(*values.values()):
        if key not in found:
            index += "."
            continue
        if found[key] not in outcomes:
            outcomes.append(found[key])
        index += chr(ord("a") + outcomes.index(found[key]))
    out = dict(source="commit c4634d2: _integral_pass, _kl_loss, _kl_loss_cmcd over fused_training_ok, adjoint_ctrl_ok, diagonal_reference, "
                      "cmcd_adjoint_ok, _capturable", axes=values, outcomes=outcomes, index=index,
               wrapped={name: outcome(loss) for name, loss in rc.wrapped_cases()})
    with open(os.path.join(rc.GOLDEN, "training_routes.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(len(found), "models;", {o: index.count(chr(ord("a") + i)) for i, o in enumerate(outcomes)})


if __name__ == "__main__":
    main()
