"""Everything the loss classes hand libsdeng.so, call for call, against the record of commit 2bfc3b4 (tests/golden/launch_census.json, made by
tests/golden/gen_launch_census.py; recorder and scenarios: tests/launch_census.py).  No GPU: the library is a stub that logs its arguments."""
import json
import os

import pytest

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from tests import build_cases as bc
from tests import golden_cases as gc
from tests import launch_census as lc

with open(os.path.join(gc.GOLDEN_DIR, "launch_census.json")) as _f:
    RECORD = json.load(_f)["scenarios"]


def test_the_census_covers_what_it_should():
    labels = [label for label, _ in lc.scenarios()]
    assert labels == list(RECORD) and len(set(labels)) == len(labels)
    for name in gc.SIM_CASES:
        assert f"eval {name}" in RECORD
    for name in gc.EUBO_CASES:
        assert f"eubo {name}" in RECORD
    for name in gc.EULER_CASES:
        assert f"euler {name}" in RECORD
    for name in lc._fixtures("train_kl_"):
        for native in (0, 1):
            for fused in (0, 1):
                assert f"train kl {name} native={native} fused={fused}" in RECORD
    for name in lc._fixtures("train_lv_") + lc._fixtures("ctrl_perturb_"):
        assert f"train lv {name}" in RECORD
    entries = {line.split()[0] for calls in RECORD.values() for line in calls}
    assert {"simulate", "kl_adjoint", "cmcd_kl_adjoint", "ctrl_vjp", "tilted_simulate", "sample_x0", "philox_normal_steps", "logz"} <= entries


def test_every_call_hands_the_library_what_the_parent_commit_handed_it():
    got = lc.take()
    assert list(got) == list(RECORD)
    for label, calls in RECORD.items():
        assert got[label] == calls, label


def _training_case():
    c = gc.load("train_lv_ei_gmm_d16")
    c.meta["kind"] = lc.KINDS[c.meta["kind"]]
    return bc.build(c, "cpu")


@pytest.mark.parametrize("method", ["lv", "kl"])
def test_a_refused_launch_leaves_the_seed_alone(method):
    b = _training_case()
    loss = b["loss"]
    loss.method, loss.train_calls, seed = method, 3, loss.seed  # (the stream of training call 0 is the eval stream itself)
    with lc.recording(refuse=("sdeng_simulate",)) as stub:
        with pytest.raises(E.UnsupportedByEngine):
            loss(b["ts"], b["x0"], *b["args"])
    assert [r["entry"] for r in stub.calls][:2] == ["sdeng_workspace_bytes", "sdeng_simulate"]
    assert loss.seed == seed
    assert stub.calls[1]["args"][0]["seed"] != seed  # the launch was handed the training call's own stream as an argument


def test_the_perturbation_side_channel_is_gone():
    b = _training_case()
    loss = b["loss"]
    assert not hasattr(loss, "_perturb")
    loss.method, loss.sde_ctrl_noise = "lv", 0.25
    with lc.recording() as stub:
        loss(b["ts"], b["x0"], *b["args"])
    launch = next(r for r in stub.calls if r["entry"] == "sdeng_simulate")
    assert launch["args"][0]["flags"] & L.FLAG_CTRL_NOISE and not hasattr(loss, "_perturb")
