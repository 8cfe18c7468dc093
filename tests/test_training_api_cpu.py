"""Host side of the three training entry points (no GPU): sdeng_ctrl_vjp, sdeng_kl_adjoint and sdeng_cmcd_kl_adjoint share one preparation
step (workspace check, weight images, time embeddings, the per-row outputs) -- their workspace layouts must stay where they were
(tests/golden/training_workspace_bytes.json, recorded from the library before the three were joined; regenerate with
tests/golden/gen_training_workspace_bytes.py only when a layout is meant to change) and a bad descriptor must still be refused with the
same code and message before any launch."""
import ctypes
import json
import os

import pytest

from sde_sampler_lrds_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "training_workspace_bytes.json")
DS, NS = (1, 2, 16, 17, 61, 64, 65, 100, 128), (1, 24, 100)
REFS = {"none": (L.REF_NONE, 0), "gauss": (L.REF_GAUSS_DIAG, 0), "gmm1": (L.REF_GMM_DIAG, 1), "gmm4": (L.REF_GMM_DIAG, 4), "gmm5": (L.REF_GMM_DIAG, 5)}
TARGETS = {"none": (L.DIST_NONE, 0), "gmm2": (L.DIST_GMM_DIAG, 2), "phi4": (L.DIST_PHI4, 0), "logreg": (L.DIST_LOGREG, 0)}
PRIORS = {"iso": L.DIST_ISO_GAUSS, "diag": L.DIST_GAUSS_DIAG}

_HOST = ctypes.create_string_buffer(64)
P = ctypes.addressof(_HOST)  # a non-null address (never dereferenced: a refused descriptor launches nothing, an accepted one stops at the NULL workspace)


def _desc(d, N=8, form=L.FORM_LIN, ctrl_kind=L.CTRL_CLIPPED, ref="none", target="none", prior="iso", flags=0):
    desc = L.Desc()
    desc.abi_version, desc.form, desc.flags, desc.B, desc.d, desc.N = L.ABI_VERSION, form, flags, 64, d, N
    desc.coef = P
    n = desc.net
    n.ctrl_kind = ctrl_kind
    n.w_in = n.b_in = n.w_h1 = n.b_h1 = n.w_h2 = n.b_h2 = n.w_out = n.b_out = P
    te = n.t_embed
    te.coeff = te.phase = te.w_out = te.b_out = te.w[0] = te.b[0] = P
    te.n_hidden, te.dim_out = 1, 64
    desc.ref.kind, desc.ref.k = REFS[ref] if isinstance(ref, str) else ref
    if desc.ref.kind != L.REF_NONE:
        desc.ref.means_init = desc.ref.vars_init = desc.ref.weights = P
    for ds, (kind, k) in ((desc.target, TARGETS[target]), (desc.prior, (PRIORS[prior], 0))):
        ds.kind, ds.k = kind, k
        ds.loc = ds.scale = ds.w = ds.aux = P
        ds.p0 = ds.p1 = ds.p2 = ds.p3 = 1.0
    desc.cmcd_g = 1.0
    return desc


def workspace_table():
    """{case: bytes} of the three ``*_workspace_bytes`` exports over the grid of the module's constants, wherever the entry point takes the
    combination (a logistic-regression design matrix lives in LDS: d <= 64; the CMCD adjoint always has a target)."""
    lib, out = L.lib(), {}
    for d in DS:
        for N in NS:
            out[f"ctrl_vjp d={d} N={N}"] = lib.sdeng_ctrl_vjp_workspace_bytes(d, N)
            for ref in REFS:
                for tgt in TARGETS:
                    if tgt == "logreg" and d > 64:
                        continue
                    desc = _desc(d, N, ref=ref, target=tgt, ctrl_kind=L.CTRL_CLIPPED if tgt == "none" else L.CTRL_SCORE)
                    out[f"kl_adjoint d={d} N={N} ref={ref} target={tgt}"] = lib.sdeng_kl_adjoint_workspace_bytes(ctypes.byref(desc))
            for tgt in ("gmm2", "phi4", "logreg"):
                for prior in PRIORS:
                    if tgt == "logreg" and d > 64:
                        continue
                    desc = _desc(d, N, form=L.FORM_CMCD, ctrl_kind=L.CTRL_SCORE, target=tgt, prior=prior)
                    out[f"cmcd_kl_adjoint d={d} N={N} target={tgt} prior={prior}"] = lib.sdeng_cmcd_kl_adjoint_workspace_bytes(ctypes.byref(desc))
    return out


def test_workspace_sizes_are_unchanged():
    want = json.load(open(GOLDEN))
    got = workspace_table()
    assert got.keys() == want.keys() and len(got) == len(NS) * (len(DS) * (1 + 5 * 4 + 3 * 2) - sum(d > 64 for d in DS) * (5 + 2))
    assert all(v > 0 for v in got.values())
    assert {k: v for k, v in got.items() if v != want[k]} == {}


def _ctrl_vjp(desc, cot=True, n_times=8, rows=64):
    lib = L.lib()
    outs = [P if cot else None] * 8  # a0 a1 a2 d0 d1 d2 dout gx
    rc = lib.sdeng_ctrl_vjp(ctypes.byref(desc) if desc is not None else None, n_times, rows, P, P if cot else None, *outs, None if cot else P, None)
    return rc, lib.sdeng_last_error().decode()


def _kl_adjoint(desc, noise=True, dst=True, ext_score=False, have_adj=True):
    adj = L.Adjoint()
    for name, _ in L.Adjoint._fields_:
        if name not in ("detach_score", "score"):
            setattr(adj, name, P)
    adj.noise, adj.dst, adj.score = (P if noise else None), (P if dst else None), (P if ext_score else None)
    lib = L.lib()
    rc = lib.sdeng_kl_adjoint(ctypes.byref(desc) if desc is not None else None, ctypes.byref(adj) if have_adj else None, None)
    return rc, lib.sdeng_last_error().decode()


def _wrong_abi(desc):
    desc.abi_version = L.ABI_VERSION + 1
    return desc


@pytest.mark.parametrize("what,call,code,word", [
    ("null descriptor", lambda: _ctrl_vjp(None), L.E_INVALID, "null argument"),
    ("wrong ABI", lambda: _ctrl_vjp(_wrong_abi(_desc(16))), L.E_INVALID, f"ABI version {L.ABI_VERSION + 1}, library has {L.ABI_VERSION}"),
    ("d = 129", lambda: _ctrl_vjp(_desc(129)), L.E_INVALID, "bad sizes (1 <= d <= 128"),
    ("no times", lambda: _ctrl_vjp(_desc(16), n_times=0), L.E_INVALID, "bad sizes (1 <= d <= 128"),
    ("backward pass without its outputs", lambda: _ctrl_vjp_missing_output(), L.E_INVALID, "every per-row output is required"),
    ("a score control", lambda: _ctrl_vjp(_desc(16, ctrl_kind=L.CTRL_SCORE, target="gmm2")), L.E_UNSUPPORTED, "ctrl_vjp: ClippedCtrl around the FourierMLP (ctrl_kind 1 given)"),
    ("null workspace, backward", lambda: _ctrl_vjp(_desc(16)), L.E_WORKSPACE, "workspace 0 bytes, need "),
    ("null workspace, forward only", lambda: _ctrl_vjp(_desc(100), cot=False), L.E_WORKSPACE, "workspace 0 bytes, need "),
    ("null workspace with the images kept", lambda: _ctrl_vjp(_desc(16, flags=L.FLAG_REUSE_PACK), n_times=1), L.E_WORKSPACE, "workspace 0 bytes, need ")])
def test_ctrl_vjp_refuses_before_any_launch(what, call, code, word):
    rc, msg = call()
    assert rc == code and word in msg, (what, rc, msg)


def _ctrl_vjp_missing_output():
    lib = L.lib()
    desc = _desc(16)
    rc = lib.sdeng_ctrl_vjp(ctypes.byref(desc), 8, 64, P, P, P, P, P, P, P, None, P, None, None, None)  # d2 missing
    return rc, lib.sdeng_last_error().decode()


@pytest.mark.parametrize("what,call,code,word", [
    ("null descriptor", lambda: _kl_adjoint(None), L.E_INVALID, "null descriptor"),
    ("wrong ABI", lambda: _kl_adjoint(_wrong_abi(_desc(16))), L.E_INVALID, f"ABI version {L.ABI_VERSION + 1}, library has {L.ABI_VERSION}"),
    ("d = 129", lambda: _kl_adjoint(_desc(129)), L.E_INVALID, "bad sizes (1 <= d <= 128"),
    ("CMCD form", lambda: _kl_adjoint(_desc(16, form=L.FORM_CMCD)), L.E_UNSUPPORTED, "kl_adjoint: forward forms LIN / EM (form 2)"),
    ("full-covariance reference", lambda: _kl_adjoint(_desc(16, ref=(L.REF_GMM_FULL, 3))), L.E_UNSUPPORTED, "a diagonal Gaussian / mixture reference (ref.kind 3)"),
    ("score control without a target", lambda: _kl_adjoint(_desc(16, ctrl_kind=L.CTRL_SCORE)), L.E_UNSUPPORTED, "on a diagonal mixture / phi^4 target (ctrl_kind 1"),
    ("null adjoint struct", lambda: _kl_adjoint(_desc(16), have_adj=False), L.E_INVALID, "null states / weights / lambda_N / per-row outputs"),
    ("FLAG_ITO without noise", lambda: _kl_adjoint(_desc(16, flags=L.FLAG_ITO), noise=False), L.E_INVALID, "FLAG_ITO needs the normals of the trajectory"),
    ("score control without dst", lambda: _kl_adjoint(_desc(16, ctrl_kind=L.CTRL_SCORE, target="gmm2"), dst=False), L.E_INVALID, "a score control needs the dst output"),
    ("null workspace", lambda: _kl_adjoint(_desc(16, flags=L.FLAG_ITO, ref="gmm4")), L.E_WORKSPACE, "workspace 0 bytes, need "),
    ("null workspace, score control", lambda: _kl_adjoint(_desc(100, form=L.FORM_EM, ctrl_kind=L.CTRL_SCORE, target="phi4")), L.E_WORKSPACE, "workspace 0 bytes, need "),
    ("null workspace, external score", lambda: _kl_adjoint(_desc(61, ctrl_kind=L.CTRL_SCORE, target="none"), ext_score=True), L.E_WORKSPACE, "workspace 0 bytes, need ")])
def test_kl_adjoint_refuses_before_any_launch(what, call, code, word):
    rc, msg = call()
    assert rc == code and word in msg, (what, rc, msg)


def test_the_refused_workspace_names_the_size_the_query_returns():
    """The size in the E_WORKSPACE message is the one ``*_workspace_bytes`` reports for the same descriptor: both come from the same layout."""
    lib = L.lib()
    desc = _desc(40, N=24, flags=L.FLAG_ITO, ref="gmm5")
    rc, msg = _kl_adjoint(desc)
    assert rc == L.E_WORKSPACE and msg.endswith(f"need {lib.sdeng_kl_adjoint_workspace_bytes(ctypes.byref(desc))}"), msg
    rc, msg = _ctrl_vjp(_desc(40), n_times=24)
    assert rc == L.E_WORKSPACE and msg.endswith(f"need {lib.sdeng_ctrl_vjp_workspace_bytes(40, 24)}"), msg
