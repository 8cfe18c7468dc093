"""A census of everything the Python layer hands libsdeng.so, taken on the CPU: ``_lib.lib()`` is replaced by a stub that logs every
entry-point call -- its scalar arguments, every scalar field of every structure it is passed (recursively), which pointers are null, and
a SHA-256 of the coefficient table behind ``coef`` -- and returns success; ``engine.require_gpu`` and ``engine._stream_ptr`` are stubbed
too, and ``torch.empty`` gives zeros, so every call chain of the loss classes runs to completion on CPU tensors and is deterministic.

``scenarios()`` is the list of calls the census covers (public surface only: ``eval``, ``compute_eubo``, the training call followed by
``backward()``, ``engine.euler_states``); ``take()`` runs them and returns {scenario: [one line per library call]}.  The fixture
``tests/golden/launch_census.json`` was recorded by ``tests/golden/gen_launch_census.py``; ``tests/test_launch_census_cpu.py`` replays it."""
from __future__ import annotations

import contextlib
import ctypes as C
import glob
import hashlib
import json
import os

import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from tests import build_cases as bc
from tests import golden_cases as gc

KINDS = {"train_lv": "rds_gmm", "train_lv_dis": "dis_ei", "train_lv_dis_orig": "dis_orig", "train_lv_dds": "dds", "train_lv_pis": "pis_phi4",
         "train_lv_cmcd": "cmcd_gmm"}  # tests/test_gpu_training.py: objects as in the simulate cases
WORKSPACE_BYTES = 4096  # what every *_workspace_bytes entry point of the stub answers (0 would mean "descriptor rejected")


def _field(value, ctype):
    if isinstance(value, C.Structure):
        return _struct(value)
    if isinstance(value, C.Array):
        return [_field(v, ctype._type_) for v in value]
    if ctype is C.c_void_p:
        return "null" if not value else "ptr"
    return repr(value) if isinstance(value, float) else value


def _struct(s):
    return {name: _field(getattr(s, name), ctype) for name, ctype in s._fields_}


def _coef_rows(name, s, args):
    """How many rows of NCOEF floats stand behind ``s.coef`` in a call of ``name`` (include/sdeng.h)."""
    if "ctrl_vjp" in name:
        return int(args[1])  # (desc, n_times, ...): a table that holds the n_times times
    rows = int(s.N)
    if isinstance(s, L.Desc) and s.form in (L.FORM_CMCD, L.FORM_CMCD_EUBO):
        rows += 1
    return rows


class StubLibrary:
    """Stands in for the CDLL: every entry point of include/sdeng.h answers success and is logged."""

    def __init__(self, refuse=()):
        self.calls, self.refuse = [], set(refuse)

    def __getattr__(self, name):
        if name not in L._PROTOS:
            raise AttributeError(name)
        restype, argtypes = L._PROTOS[name]

        def entry(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            rec = {"entry": name, "args": []}
            for a, t in zip(args, argtypes):
                if hasattr(a, "_obj"):  # ctypes.byref(structure)
                    s = a._obj
                    d = _struct(s)
                    if getattr(s, "coef", None):
                        rows = _coef_rows(name, s, args)
                        d["coef"] = hashlib.sha256(C.string_at(s.coef, 4 * L.NCOEF * rows)).hexdigest() if rows > 0 else "ptr"
                    rec["args"].append(d)
                elif t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer)):
                    value = a.value if isinstance(a, C.c_void_p) else a
                    rec["args"].append("null" if not value else "ptr")
                else:
                    rec["args"].append(repr(float(a)) if t in (C.c_float, C.c_double) else int(a))
            self.calls.append(rec)
            if restype is C.c_char_p:
                return b"refused by the stub library"
            if restype is C.c_size_t:
                return WORKSPACE_BYTES
            return L.E_UNSUPPORTED if name in self.refuse else 0
        return entry


@contextlib.contextmanager
def recording(refuse=()):
    """Inside: the library is the stub, no GPU is asked for, fresh memory is zeros.  Yields the stub (``.calls``)."""
    stub = StubLibrary(refuse)
    saved = (L.lib, E.require_gpu, E._stream_ptr, torch.empty, torch.empty_like)
    L.lib, E.require_gpu, E._stream_ptr = (lambda: stub), (lambda x: None), (lambda device: None)
    torch.empty, torch.empty_like = torch.zeros, torch.zeros_like
    try:
        yield stub
    finally:
        L.lib, E.require_gpu, E._stream_ptr, torch.empty, torch.empty_like = saved


def line(rec):
    """One call as 'entry key=value ... #digest': the descriptor's headline fields, and a digest of the full record."""
    head = next((a for a in rec["args"] if isinstance(a, dict)), {})
    parts = [rec["entry"][6:]] + [f"{k}={head[k]}" for k in ("form", "flags", "N", "B", "d", "M", "n_times") if head.get(k)]
    return " ".join(parts) + " #" + hashlib.sha256(json.dumps(rec, sort_keys=True).encode()).hexdigest()[:12]


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------------
def _initial_kw(b):
    return {k: v for k, v in b.get("kwargs", {}).items() if k == "initial_log_prob"}


def _draw(b):
    from sde_sampler_lrds_amd.distr.gauss import IsotropicGauss
    B, d = b["x0"].shape
    return E.InitialDraw(IsotropicGauss(dim=d, scale=1.0), B, "cpu")


def _eval(name, draw=False, split=False):
    def run():
        b = bc.build(gc.load(name), "cpu")
        b["loss"].split_tiles = split
        b["loss"].eval(b["ts"], _draw(b) if draw else b["x0"], *b["args"], **_initial_kw(b))
    return run


def _eubo(name, draw=False):
    def run():
        b = bc.build(gc.load(name), "cpu")
        b["loss"].compute_eubo(b["ts"], _draw(b) if draw else b["x0"].clone(), *b["args"], **_initial_kw(b))
    return run


def _build_training(name):
    c = gc.load(name)
    if "_cmcd_" in name and name.startswith("train_kl") and name != "train_kl_cmcd_gmm_d16":
        from tests.test_gpu_cmcd_adjoint import build_fixture
        loss, ts, x0, target, prior = build_fixture(c, "cpu")
        return c, dict(loss=loss, ts=ts, x0=x0, args=(target.unnorm_log_prob,), kwargs=dict(initial_log_prob=prior.log_prob))
    if c.meta["kind"] not in KINDS:
        from tests import rds_score_cases as rsc
        return c, rsc.build(c, "cpu")
    c.meta["kind"] = KINDS[c.meta["kind"]]
    return c, bc.build(c, "cpu")


def _train(name, method, native=True, fused=True, draw=False, split=False, tps=1):
    """Two consecutive training calls, each followed by backward()."""
    def run():
        c, b = _build_training(name)
        loss = b["loss"]
        loss.method, loss.graph_adjoint, loss.native_adjoint, loss.fused_training, loss.split_tiles = method, False, native, fused, split
        loss.traj_per_sample = tps
        if method == "kl":
            loss.max_rnd = None
        if name.startswith("ctrl_perturb"):
            loss.sde_ctrl_noise, loss.sde_ctrl_dropout = c.meta["sde_ctrl_noise"], c.meta["sde_ctrl_dropout"]
        for _ in range(2):
            value, _metrics = loss(b["ts"], _draw(b) if draw else b["x0"], *b["args"], **_initial_kw(b))
            value.backward()
    return run


def _rds_nn(case, integrator, train):
    def run():
        from sde_sampler_lrds_amd.experiments import benchmark_utils as bu
        from tests import tilted_cases as tc
        net = tc.mirror(case)[1]
        target = bu.make_target_details("many_modes", dim=net.dim, n_modes=3)
        model = bu.make_model("vp-ref", "nn", "lv", integrator, "base_zero_init", "uniform", dict(net=net, sigma=1.0), target,
                              dict(train_steps=10, train_batch_size=64, eval_batch_size=96), n_steps=4, device="cpu")
        x = torch.randn(37, net.dim, generator=torch.Generator().manual_seed(3))
        ts = model.train_timesteps(device="cpu")
        args = (model.clipped_target_unnorm_log_prob, model.reference_distr.log_prob)
        if not train:
            model.loss.eval(ts, x, *args)
            return
        for _ in range(2):
            value, _metrics = model.loss(ts, x, *args)
            value.backward()
    return run


def _euler(name):
    def run():
        c = gc.load(name)
        E.euler_states(bc.build_euler(c, "cpu"), c["ts"], c["x0"], seed=c.meta["seed"])
    return run


def _fixtures(prefix):
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gc.GOLDEN_DIR, prefix + "*.npz")))
    return [n for n in names if "rds_nn" not in n]


def scenarios():
    """[(label, thunk)] in the order the census is taken (an order: the host caches of the engine are shared by the scenarios)."""
    out = [(f"eval {n}", _eval(n)) for n in gc.SIM_CASES]
    out += [(f"eval {n} draw", _eval(n, draw=True)) for n in ("rds_ei_gmm_d8_k4", "dds_two_modes_d2", "cmcd_gmm_iso_d16", "dis_orig_lerp_d8")]
    out += [(f"eval {n} split", _eval(n, split=True)) for n in ("rds_ei_gmm_d8_k4", "pis_em_phi4_d100", "cmcd_logreg_d61", "rds_em_remove_ref_d16")]
    out += [(f"eubo {n}", _eubo(n)) for n in gc.EUBO_CASES] + [("eubo eubo_cmcd_gmm_d16 draw", _eubo("eubo_cmcd_gmm_d16", draw=True))]
    out += [(f"train lv {n}", _train(n, "lv")) for n in _fixtures("train_lv_") + _fixtures("ctrl_perturb_")]
    out += [(f"train lv {n} unfused", _train(n, "lv", fused=False)) for n in ("train_lv_ei_gmm_d16", "train_lv_pis_phi4_d100")]
    out += [(f"train lv {n} split draw", _train(n, "lv", draw=True, split=True)) for n in ("train_lv_ei_gmm_d16", "train_lv_dis_orig_d8", "ctrl_perturb_dds_d2_noise")]
    out += [("train lv_traj train_lv_em_gmm_d16 tps=2", _train("train_lv_em_gmm_d16", "lv_traj", tps=2))]
    for native in (False, True):
        for fused in (False, True):
            out += [(f"train kl {n} native={int(native)} fused={int(fused)}", _train(n, "kl", native=native, fused=fused)) for n in _fixtures("train_kl_")]
    out += [(f"train kl {n} split draw", _train(n, "kl", draw=True, split=True)) for n in ("train_kl_ei_gmm_d16", "train_kl_dds_d2", "train_kl_cmcd_gmm_d16")]
    out += [("train kl train_kl_dis_ei_d8 tps=2", _train("train_kl_dis_ei_d8", "kl", tps=2))]
    out += [(f"rds_nn {c}_{i} {'train lv' if t else 'eval'}", _rds_nn(c, i, t)) for c, i in (("a", "ei"), ("b", "em")) for t in (False, True)]
    out += [(f"euler {n}", _euler(n)) for n in gc.EULER_CASES]
    return out


def take(only=None, full=False):
    """{label: [line per library call]} (``full``: the whole records) of every scenario, or of those whose label contains ``only``."""
    got = {}
    for label, run in scenarios():
        if only is not None and only not in label:
            continue
        torch.manual_seed(0)
        with recording() as stub:
            run()
        got[label] = stub.calls if full else [line(r) for r in stub.calls]
    return got
