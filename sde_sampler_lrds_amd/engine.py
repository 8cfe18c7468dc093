"""Descriptor compiler + launcher: turns the Python objects the reference's loss classes are handed
(drift-net module, SDE, reference, target / prior distributions, time grid) into one flat
``sdeng_desc`` (include/sdeng.h) and calls ``sdeng_simulate`` on the current HIP stream.

Objects are recognised by duck typing on class name + attributes, so both the reference's own classes
(``sde_sampler.eq.sdes.VP`` ...) and this package's mirrors are accepted.  Anything not recognised raises
``UnsupportedByEngine`` -- there is no PyTorch re-implementation of the step loop to fall back on.

Per-step scalars are computed on the host with the same 0-d fp32 torch expressions the
reference evaluates inside its loop, so the coefficients the kernel consumes are bit-identical to the
reference's; the table is cached per (loss, time grid).
"""
from __future__ import annotations

import copy
import ctypes as C
import dataclasses
import math
import weakref

import torch

from . import _lib as L
from . import routes as R
from .routes import UnsupportedByEngine, diagonal_reference, resolve_reference  # noqa: F401  (their names here)
from .routes import name_of as _name, self_of as _self_of

adjoint_ctrl_ok, cmcd_adjoint_ok = R.kl_native, R.cmcd_native  # the gates of the two one-launch adjoints, under the names they have here
_DIST_REFUSALS = {"PhiFour": "PhiFour: only the 1-D Dirichlet-0 untilted lattice", "Rings": "Rings: at most 8 radii"}  # where dist_kind has no kind


def _f32c(t: torch.Tensor) -> torch.Tensor:
    """``t`` as the kernels read it: no graph, float32, contiguous (``t`` itself when it already is)."""
    return t.detach().to(torch.float32).contiguous()


def _dev_f32(t: torch.Tensor, device, keep: list):
    t = t.detach().to(device=device, dtype=torch.float32).contiguous()
    keep.append(t)
    return t.data_ptr()


# ------------------------------------------------------------------------------------------------
# distributions
# ------------------------------------------------------------------------------------------------
def dist_desc(obj, device, keep, clip=None, score_only=False) -> L.Dist:
    """Distribution object -> sdeng_dist (distr/*.py parameters) of the kind ``routes.dist_kind`` names: classifier and builder cannot disagree."""
    ds = L.Dist()
    ds.clip = float(clip) if clip else 0.0
    kind = R.dist_kind(obj, score_only)
    if kind is None:
        raise UnsupportedByEngine(_DIST_REFUSALS.get(_name(obj), f"no HIP log-density/score for distribution {_name(obj)}"))
    ds.kind = kind
    if kind == L.DIST_ISO_GAUSS:
        # the four scalars are read back from the device once per parameter version (a read-back synchronises the stream)
        key = (obj.loc._version, obj.scale._version, obj.loc.data_ptr(), obj.scale.data_ptr())
        hit = getattr(obj, "_sdeng_scalars", None)
        if hit is None or hit[0] != key:
            loc, scale = obj.loc[0, 0].detach().float().cpu(), obj.scale[0, 0].detach().float().cpu()
            var = scale ** 2
            hit = (key, (float(loc), float(scale), float(-0.5 * obj.dim * (2.0 * math.pi * var).log()), float(var)))  # distr/gauss.py:759
            obj._sdeng_scalars = hit
        ds.p0, ds.p1, ds.p2, ds.p3 = hit[1]
    elif kind in (L.DIST_GAUSS_DIAG, L.DIST_GMM_DIAG):  # loc / scale [K,d]; a Gaussian is the one-component case without weights
        ds.k = int(obj.loc.shape[0])
        ds.loc = _dev_f32(obj.loc, device, keep)
        ds.scale = _dev_f32(obj.scale, device, keep)
        if kind == L.DIST_GMM_DIAG:
            ds.w = _dev_f32(obj.mixture_weights, device, keep)
    elif kind == L.DIST_PHI4:
        ds.p0, ds.p1, ds.p2 = scalar_of(obj.a), scalar_of(obj.b), scalar_of(obj.beta)
    elif kind == L.DIST_GAUSS_FULL:
        key = (obj.cov._version, obj.cov.data_ptr(), str(device))
        hit = getattr(obj, "_sdeng_chol", None)
        if hit is None or hit[0] != key:  # Cholesky factor, its inverse and log-determinant once per parameter version
            tril = torch.linalg.cholesky(obj.cov.detach().float().cpu())
            hit = (key, torch.linalg.inv(tril).to(device), float(tril.diagonal().log().sum()), tril.to(device))
            obj._sdeng_chol = hit
        ds.loc = _dev_f32(obj.loc, device, keep)
        ds.scale = _dev_f32(obj.prec, device, keep)
        ds.w = _dev_f32(hit[1], device, keep)
        ds.p0 = hit[2]
        ds.aux = _dev_f32(hit[3], device, keep)  # L itself: GaussFull.sample (x0_dist)
    elif kind == L.DIST_LOGREG:
        ds.k = int(obj.X_train.shape[0])
        ds.loc = _dev_f32(obj.X_train, device, keep)
        ds.scale = _dev_f32(obj.y_train, device, keep)
        ds.p0, ds.p1, ds.p2 = scalar_of(obj.weight_scale), scalar_of(obj.intercept_mean), scalar_of(obj.intercept_scale)
        ds.p3 = scalar_of(obj.threshold)
    elif kind == L.DIST_RINGS:  # distr/rings.py:38-109
        ds.k = int(obj.radiuses.shape[0])
        ds.loc = _dev_f32(obj.radiuses, device, keep)
        ds.w = _dev_f32(obj.radius_dist.mixture_distribution.probs, device, keep)
        ds.p0 = float(obj.radius_dist.component_distribution.scale.reshape(-1)[0])
    elif kind == L.DIST_CHECKERBOARD:  # distr/checkerboard.py: uniform squares; this package's mirror and the reference's object alike
        comp = obj.distr.component_distribution.base_dist
        ds.k = int(comp.low.shape[0])
        ds.loc = _dev_f32(comp.low, device, keep)
        ds.scale = _dev_f32(comp.high, device, keep)
        with torch.no_grad():  # each square's log-density: the object's own expression at the square's centre (it is constant inside)
            ds.w = _dev_f32(obj.unnorm_log_prob((comp.low + comp.high) / 2.0).reshape(-1), device, keep)
    elif kind == L.DIST_GMM_FULL:
        # score_mog_full inside the step loop (distr/gauss.py:110-121): the kernel takes each covariance in its eigen form, decomposed
        # once per parameter version in fp64 (the reference inverts the covariances once, in fp32, at construction)
        cov = getattr(obj, "cov", None)
        if cov is not None:
            eig = _EIGH.get(cov, lambda v: torch.linalg.eigh(v.detach().double()))
            evals, evecs = eig[0].float(), eig[1].float()
        else:
            eig = _EIGH.get(obj.prec, lambda v: torch.linalg.eigh(v.detach().double()))
            evals, evecs = (1.0 / eig[0]).float(), eig[1].float()
        ds.k = int(obj.loc.shape[0])
        ds.loc = _dev_f32(obj.loc, device, keep)
        ds.scale = _dev_f32(evals, device, keep)
        ds.w = _dev_f32(obj.mixture_weights, device, keep)
        ds.aux = _dev_f32(evecs, device, keep)
    return ds


class InitialDraw:
    """``prior.sample((B,))`` left to the engine: pass it wherever a loss takes ``x`` and the kernel draws
    x0 = loc + scale * z itself (z = Philox stream 1 at step 0, keyed by the loss's seed and the global particle index), in
    registers for IsotropicGauss / Gauss / Delta priors -- x0 never exists in HBM.  ``tensor(seed, particle0)`` gives the same
    x0 as a device tensor (``sdeng_sample_x0``), for callers that need it.  Reference: IsotropicGauss.sample distr/gauss.py:772-787,
    Delta.sample distr/delta.py:27-31, GaussFull.sample distr/gauss.py:709-713 (all on torch's global generator upstream)."""

    def __init__(self, prior, batch_size: int, device=None):
        if _name(prior) == "IsotropicGauss" and getattr(prior, "truncate_quartile", None) is not None:
            raise UnsupportedByEngine("truncated IsotropicGauss prior: no native sampler")
        self.prior, self.batch_size = prior, int(batch_size)
        self.device = torch.device(device) if device is not None else next(iter(prior.buffers())).device
        self.shape = (self.batch_size, int(prior.dim))
        self.is_cuda = self.device.type == "cuda"

    def desc(self, keep) -> L.Dist:
        ds = dist_desc(self.prior, self.device, keep)
        if _name(self.prior) == "Delta":
            ds.scale = None  # Delta.sample repeats loc (its tiny scale only enters the log-density)
        if ds.kind not in (L.DIST_ISO_GAUSS, L.DIST_GAUSS_DIAG, L.DIST_GAUSS_FULL):
            raise UnsupportedByEngine(f"no native sampler for prior {_name(self.prior)}")
        return ds

    def tensor(self, seed: int, particle0: int = 0) -> torch.Tensor:
        keep = []
        ds = self.desc(keep)
        B, d = self.shape
        out = torch.empty(B, d, dtype=torch.float32, device=self.device)
        L.check(L.lib().sdeng_sample_x0(C.byref(ds), int(seed), int(particle0), B, d, out.data_ptr(), _stream_ptr(self.device)))
        return out


def sample_prior(prior, batch_size: int, seed: int, particle0: int = 0, device=None) -> torch.Tensor:
    """prior.sample((B,)) from the engine's counter-based stream: a pure function of (seed, global particle index)."""
    return InitialDraw(prior, batch_size, device).tensor(seed, particle0)


def resolve_logp(fn):
    """A log-density callable handed to the loss -> (distribution object, clip) or None if opaque."""
    owner = _self_of(fn)
    if owner is None:
        return None
    fname = getattr(fn, "__name__", "")
    if fname == "clipped_target_unnorm_log_prob" and hasattr(owner, "target"):  # solver/oc.py:80-87
        return owner.target, getattr(owner, "clip_target", None)
    if fname in ("log_prob", "unnorm_log_prob") and hasattr(owner, "dim"):
        if fname == "log_prob" and getattr(owner, "log_norm_const", 0.0) not in (0.0, None):
            return None
        return owner, None
    return None


# ------------------------------------------------------------------------------------------------
# drift net
# ------------------------------------------------------------------------------------------------
def _time_embed(te, device, keep) -> L.TimeEmbed:
    out = L.TimeEmbed()
    if _name(te) != "TimeEmbed" or te.channels != 64:
        raise UnsupportedByEngine("time embedding must be TimeEmbed(channels=64)")
    if _name(te.activation) != "GELU" or getattr(te.activation, "approximate", "none") != "none":
        raise UnsupportedByEngine("activation must be exact-erf GELU")
    out.coeff = _dev_f32(te.timestep_coeff.reshape(-1), device, keep)
    out.phase = _dev_f32(te.timestep_phase.reshape(-1), device, keep)
    n_hidden = len(te.hidden_layer)
    if n_hidden > 4:
        raise UnsupportedByEngine("TimeEmbed with more than 5 layers")
    for i, layer in enumerate(te.hidden_layer):
        out.w[i] = _dev_f32(layer.weight, device, keep)
        out.b[i] = _dev_f32(layer.bias, device, keep)
    out.n_hidden = n_hidden
    out.dim_out = int(te.out_layer.weight.shape[0])
    out.w_out = _dev_f32(te.out_layer.weight, device, keep)
    out.b_out = _dev_f32(te.out_layer.bias, device, keep)
    return out


def unwrap_ctrl(ctrl):
    """(control module the kernels know, RemoveReferenceCtrl wrapper or None); the wrapper only in the form upstream's forward can evaluate."""
    rec = R.describe_ctrl(ctrl)
    if rec.wrapper is not None and rec.wrapper.use_rescaling:
        raise UnsupportedByEngine("RemoveReferenceCtrl(use_rescaling=True): upstream's forward needs the `sde` its constructor refuses "
                                  "(models/reparam.py:52, :60) and raises AttributeError; use_rescaling=False is on the HIP path")
    return rec.ctrl, rec.wrapper


def net_desc(ctrl, device, keep) -> L.Net:
    """ClippedCtrl / ScoreCtrl / LerpCtrl / CancelDriftCtrl around FourierMLP(4 layers, 64 channels, GELU) -> sdeng_net."""
    ctrl, _ = unwrap_ctrl(ctrl)
    rec = R.describe_ctrl(ctrl)
    if rec.kind is None:
        raise UnsupportedByEngine(f"control wrapper {_name(ctrl)} has no HIP kernel")
    net = ctrl.base_model
    fault = R.net_fault(net)
    if fault:
        raise UnsupportedByEngine(fault)
    if getattr(ctrl, "hard_constrain", False):
        raise UnsupportedByEngine("LerpCtrl(hard_constrain=True)")
    n = L.Net()
    n.ctrl_kind = rec.kind
    n.w_in, n.b_in = _dev_f32(net.input_embed.weight, device, keep), _dev_f32(net.input_embed.bias, device, keep)
    n.w_h1, n.b_h1 = _dev_f32(net.hidden_layer[0].weight, device, keep), _dev_f32(net.hidden_layer[0].bias, device, keep)
    n.w_h2, n.b_h2 = _dev_f32(net.hidden_layer[1].weight, device, keep), _dev_f32(net.hidden_layer[1].bias, device, keep)
    n.w_out, n.b_out = _dev_f32(net.out_layer.weight, device, keep), _dev_f32(net.out_layer.bias, device, keep)
    n.t_embed = _time_embed(net.timestep_embed, device, keep)
    n.clip_model = float(ctrl.clip_model) if ctrl.clip_model else 0.0
    if n.ctrl_kind != L.CTRL_CLIPPED:
        n.clip_score = float(ctrl.clip_score) if ctrl.clip_score else 0.0
        n.scale_score = float(ctrl.scale_score)
        if ctrl.score_model is not None:
            n.score_model = _time_embed(ctrl.score_model, device, keep)
    return n


def ctrl_target(ctrl):
    """Distribution whose score ScoreCtrl/LerpCtrl mixes in (``target_score`` is a bound ``Distribution.score``)."""
    rec = R.describe_ctrl(unwrap_ctrl(ctrl)[0])
    if rec.kind == L.CTRL_CLIPPED:
        return None, None
    if rec.target is None:
        raise UnsupportedByEngine("ScoreCtrl.target_score must be a bound Distribution.score")
    if rec.kind == L.CTRL_LERP and rec.lerp_prior is None:
        raise UnsupportedByEngine("LerpCtrl.prior_score must be IsotropicGauss.score")
    return rec.target, rec.lerp_prior


# ------------------------------------------------------------------------------------------------
# reference drift
# ------------------------------------------------------------------------------------------------
class _TensorCache:
    """Derived facts about a caller's tensor (shared-variance test, eigendecomposition), keyed by the tensor OBJECT: the entry holds a
    weak reference, so it dies with the tensor and a new tensor the allocator places at the same address can never match; the
    (version, shape, device) part of the key catches in-place edits.  Nothing is ever written into the caller's own containers
    (``reference_distr_utils`` is iterated by ``RDS.state_dict()`` and ``MarginalReference.to()``)."""

    def __init__(self):
        self._d = {}

    def get(self, t: torch.Tensor, compute):
        key = (t._version, tuple(t.shape), str(t.device), t.data_ptr())
        hit = self._d.get(id(t))
        if hit is not None and hit[0]() is t and hit[1] == key:
            return hit[2]
        val = compute(t)
        ident = id(t)
        self._d[ident] = (weakref.ref(t, lambda _r, i=ident: self._d.pop(i, None)), key, val)
        return val


_SHARED_VAR = _TensorCache()
_EIGH = _TensorCache()
_SCALARS = _TensorCache()


def scalar_of(v) -> float:
    """float(v) for a 0-d parameter / buffer that lives on the GPU, read back ONCE per tensor version: a read-back waits for everything
    queued on the stream, so a descriptor that reads four scalars per call serialises consecutive passes (cfg 4: 6.6 ms of GPU work
    per pass became 9.7 ms of wall time)."""
    if not torch.is_tensor(v):
        return float(v)
    if not v.is_cuda:
        return float(v)
    return _SCALARS.get(v, lambda t: float(t.detach().float().cpu()))


def same_reference(a, b) -> bool:
    """Do two ``reference_distr_utils`` dicts describe the same reference (same tensors, or equal contents)?"""
    if a is b:
        return True
    if not isinstance(a, dict) or not isinstance(b, dict) or a.keys() != b.keys():
        return False
    for k in a:
        va, vb = (a[k] if isinstance(a[k], tuple) else (a[k],)), (b[k] if isinstance(b[k], tuple) else (b[k],))
        if len(va) != len(vb):
            return False
        for x, y in zip(va, vb):
            if x is not y and not (x.shape == y.shape and torch.equal(x.detach().cpu(), y.detach().cpu())):
                return False
    return True


def ref_desc(kind, utils, device, keep) -> L.Ref:
    r = L.Ref()
    if kind == "none":
        r.kind = L.REF_NONE
    elif kind == "gaussian" and (isinstance(utils["var_init"], tuple) or utils["var_init"].dim() == 2):
        # score_gauss_full (distr/gauss.py:129-135, eq/sdes.py:274-277) = the full-covariance mixture kernel with one component
        var = utils["var_init"]
        full = dict(means_init=utils["x_init"].reshape(1, -1), weights_init=torch.ones(1),
                    variances_init=(var[0].unsqueeze(0), var[1].unsqueeze(0)) if isinstance(var, tuple) else var.unsqueeze(0))
        return ref_desc("gmm", full, device, keep)
    elif kind == "gaussian":
        r.kind, r.k = L.REF_GAUSS_DIAG, 1
        r.means_init = _dev_f32(utils["x_init"].reshape(-1), device, keep)
        r.vars_init = _dev_f32(utils["var_init"].reshape(-1), device, keep)
    else:
        var = utils["variances_init"]
        r.k = int(utils["means_init"].shape[0])
        r.means_init = _dev_f32(utils["means_init"], device, keep)
        r.weights = _dev_f32(utils["weights_init"], device, keep)
        if isinstance(var, tuple) or var.dim() == 3:
            # full covariances (score_mog_full): the kernel takes the eigen form (D, P) the reference also accepts
            # (eq/sdes.py:228-238); covariance matrices are decomposed once per parameter version
            if isinstance(var, tuple):
                evals, evecs = var
            else:
                eig = _EIGH.get(var, lambda v: torch.linalg.eigh(v.detach().double()))  # once per parameter version
                evals, evecs = eig[0].float(), eig[1].float()
            r.kind = L.REF_GMM_FULL
            r.vars_init = _dev_f32(evals, device, keep)
            r.eigvecs = _dev_f32(evecs, device, keep)
        else:
            r.kind = L.REF_GMM_DIAG
            r.vars_init = _dev_f32(var, device, keep)
            # do all components share one variance vector?  (one read-back per parameter version)
            r.shared_var = 1 if _SHARED_VAR.get(var, lambda v: bool(torch.equal(v, v[:1].expand_as(v)))) else 0
    return r



# ------------------------------------------------------------------------------------------------
# per-step scalar tables
# ------------------------------------------------------------------------------------------------
def _cpu_sde(sde):
    if sde is None:
        return None
    try:
        return copy.deepcopy(sde).to("cpu")
    except Exception:  # modules holding bound methods of other modules (ControlledLangevinSDE)
        return sde


def _transition_gains(sde, s, t, ddpm):
    """(x gain, ctrl gain, noise gain) of the EI / DDPM-like kernels, with the reference's expressions
    (eq/sdes.py:532-555 VP, :658-678 PinnedBM)."""
    n = _name(sde)
    if n in ("VP", "CosineVP"):
        sig, lam = sde.scale_diff_coeff, sde.lambda_(s, t)
        if not ddpm:
            return torch.sqrt(1.0 + lam), 2.0 * sig ** 2 * (torch.sqrt(1.0 + lam) - 1.0), sig * torch.sqrt(lam)
        T = sde.terminal_t
        lam_b = 1.0 - torch.exp(sde.alpha_(T - t) - sde.alpha_(T - s))
        la = 1.0 - torch.exp(-sde.alpha_(T - s))
        lb = 1.0 - torch.exp(-sde.alpha_(T - t))
        half = (sde.alpha_(sde.terminal_t - s) - sde.alpha_(sde.terminal_t - t)) / 2.0
        var = sig ** 2 * lam_b * (lb / la)
        return torch.sqrt(1.0 + lam), 2.0 * sig ** 2 * torch.sinh(half), torch.sqrt(var)
    if n == "PinnedBM":
        g, T = sde.diff_coeff, sde.terminal_t
        var = g ** 2 * ((T - t) / (T - s)) * (t - s) if ddpm else g ** 2 * (t / s) * (t - s)
        return t / s, g ** 2 * (t - s), torch.sqrt(var)
    raise UnsupportedByEngine(f"{n} has no closed-form EI/DDPM transition kernel")


def coef_table(kind, ts, sde=None, *, with_ref=False, lerp=False, cancel=None, ctrl_sde=None, alpha=None, sigma=None, train=False, dim=1,
               rescale=True, ctrl_noise=None, ctrl_dropout=None) -> torch.Tensor:
    """[N,16] fp32 table (column meaning: include/sdeng.h).  ``kind``: 'ei' | 'ddpm' | 'dis_ei' | 'em' |
    'time_reversal' | 'dds' | 'eubo_ei' | 'eubo_em'.  ``ts`` is a CPU tensor; every entry is produced by the reference's scalar formula.
    ``ctrl_noise`` / ``ctrl_dropout`` (the loss's sde_ctrl_noise / sde_ctrl_dropout, forward kinds only) fill columns 12-15: sigma, p and
    drift_coeff_t, diff_coeff_t of ``sde`` at the time the loss hands its control (generative_and_sde_ctrl, losses/oc.py:83-103)."""
    perturb = ctrl_noise is not None or ctrl_dropout is not None
    if perturb and kind not in ("ei", "ddpm", "dis_ei", "em", "time_reversal", "dds"):
        raise UnsupportedByEngine(f"sde_ctrl_noise / sde_ctrl_dropout: forward loops only (table kind {kind!r})")
    linear_sde = sde is not None and hasattr(sde, "drift_coeff_t") and hasattr(sde, "diff_coeff_t")
    if ctrl_dropout is not None and not linear_sde:
        raise ValueError("sde_ctrl_dropout replaces the control by -drift(t, x) / diff(t, x) of the loss's SDE (losses/oc.py:101-102), which "
                         f"needs a linear (OU) SDE; this loss has {_name(sde) if sde is not None else 'sde=None'}")
    ts = ts.detach().to("cpu", torch.float32)
    N = ts.numel() - 1
    if kind == "cmcd_eubo":  # N+1 rows in iteration order: row k is the evaluation at time ts[N-k] (losses/oc.py:782-823)
        out = torch.zeros(N + 1, L.NCOEF, dtype=torch.float32)
        Tstar = sde.terminal_t
        for k in range(N + 1):
            tk = ts[N - k]
            out[k, 0] = tk
            out[k, 4], out[k, 5] = tk / Tstar, 1.0 - tk / Tstar  # eq/sdes.py:103 at this evaluation's time
            out[k, 6], out[k, 7] = out[k, 4], out[k, 5]
            if k < N:
                dt = ts[N - k] - ts[N - 1 - k]
                out[k, 2], out[k, 3] = dt, dt.sqrt()
        return out
    if kind == "cmcd":  # N+1 rows: row k holds the times/weights of step k; the last row only ts[N] (net time)
        out = torch.zeros(N + 1, L.NCOEF, dtype=torch.float32)
        Tstar = sde.terminal_t
        for k in range(N + 1):
            out[k, 0] = ts[k]
            if k < N:
                s, t = ts[k], ts[k + 1]
                dt = t - s
                out[k, 1], out[k, 2], out[k, 3] = t, dt, dt.sqrt()
                out[k, 4], out[k, 5] = s / Tstar, 1.0 - s / Tstar  # eq/sdes.py:103
                out[k, 6], out[k, 7] = t / Tstar, 1.0 - t / Tstar
        return out
    out = torch.zeros(N, L.NCOEF, dtype=torch.float32)
    T = ts[-1]
    for k in range(N):
        s, t = ts[k], ts[k + 1]
        row = out[k]
        row[7] = 1.0
        if kind in ("ei", "ddpm", "dis_ei"):
            tau = T - s
            omega = sde.omega_ddpm(s, t) if kind == "ddpm" else sde.omega(s, t)
            g1, g2, g3 = _transition_gains(sde, s, t, kind == "ddpm")
            row[0], row[1], row[2], row[3] = tau, g1, g2, g3
            row[4], row[5] = 0.5 * omega, torch.sqrt(omega)
        elif kind == "em":
            tau = T - s
            dt = t - s
            g = sde.diff(tau, None)
            row[0], row[1], row[2], row[3] = tau, -sde.drift_coeff_t(tau), g, torch.square(g)
            row[4], row[5] = dt, dt.sqrt()
        elif kind == "time_reversal":
            tau = s
            dt = t - s
            g = sde.diff(s, None)
            row[0], row[1], row[2], row[3] = s, sde.drift_coeff_t(s), g, torch.square(g)
            row[4], row[5] = dt, dt.sqrt()
            if not train:
                row[6] = -(sde.int_drift_coeff_t(s, t) * dim)  # losses/oc.py:1218-1219, eq/sdes.py:137-141
        elif kind in ("eubo_ei", "eubo_em"):
            # compute_eubo (losses/oc.py:325-358, 539-564): iteration k noises from time T - t to T - s with
            # (s, t) = (ts[N-1-k], ts[N-k]); the rows are laid out in iteration order
            s, t = ts[N - 1 - k], ts[N - k]
            tau = T - s
            mean_f, var_f = sde.transition_params(T - t, T - s)
            std_f = var_f.sqrt()
            row[0], row[1], row[2], row[3] = tau, mean_f, 1.0, std_f
            if kind == "eubo_ei":
                omega = sde.omega(s, t)
                row[4], row[5] = omega, torch.sqrt(omega)
            else:
                g = sde.diff(tau, None)
                dt = t - s
                if rescale:
                    row[2] = 1.0 / g
                row[4] = dt * g ** 2
                row[5] = std_f / mean_f
                row[6] = 1.0 / mean_f - 1.0 + sde.drift_coeff_t(tau) * dt
        elif kind == "dds":
            tau = s
            dt = t - s
            beta_k = torch.clip(alpha * dt.sqrt(), 0, 1)
            alpha_k = torch.sqrt(1.0 - beta_k ** 2)
            row[0], row[1] = s, alpha_k
            row[2] = (beta_k ** 2) * (sigma ** 2)
            row[3] = sigma * beta_k
            row[4] = 0.5 * (beta_k ** 2 * sigma ** 2)
            row[5] = sigma * beta_k
        else:
            raise ValueError(kind)
        csde = ctrl_sde if ctrl_sde is not None else sde  # the control's own SDE (DDS has no loss-level SDE)
        if lerp:  # LerpCtrl: weight t/T (reparam.py:175) and gain g(t) (reparam.py:199), at the net's time
            t_net = row[0].clone()
            row[7] = csde.diff(t_net, None)
            row[8] = t_net / csde.terminal_t
        if cancel is not None:  # CancelDriftCtrl (reparam.py:131-145): drift/g + (g/2) score, or drift/g^2 + score/2
            t_net = row[0].clone()
            g = csde.diff(t_net, None)
            row[7] = 0.5 * g if cancel == "rescale" else 0.5
            row[8] = csde.drift_coeff_t(t_net) / (g if cancel == "rescale" else torch.square(g))
        if with_ref:  # eq/sdes.py:228-229, 247
            s_tau = sde.s(tau)
            row[9], row[10], row[11] = s_tau, s_tau ** 2 * sde.sigma_sq(tau), s_tau ** 2
        if perturb:  # the control's perturbation; tau is the time the loss evaluates its control at (T - s, or s for DDS / TimeReversalLoss)
            row[12] = 0.0 if ctrl_noise is None else float(ctrl_noise)
            row[13] = 0.0 if ctrl_dropout is None else float(ctrl_dropout)
            if linear_sde:  # OU.drift = drift_coeff_t(t) x, OU.diff = diff_coeff_t(t) (eq/sdes.py:143-148)
                row[14], row[15] = sde.drift_coeff_t(tau), sde.diff_coeff_t(tau)
    return out



# ------------------------------------------------------------------------------------------------
# launch
# ------------------------------------------------------------------------------------------------
class Workspace:
    """Grow-only device scratch per (device) -- the C ABI never allocates."""

    def __init__(self):
        self.buf = {}

    def get(self, nbytes, device):
        cur = self.buf.get(device)
        if cur is None or cur.numel() < nbytes:
            cur = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            self.buf[device] = cur
        return cur


_WS = Workspace()


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check_supported(rc: int):
    """``L.check`` for the entry points whose callers are told of a combination the library has no kernel for (INTEGRATION.md "Limits,
    first") by the documented exception: E_UNSUPPORTED becomes UnsupportedByEngine with the library's reason."""
    if rc == L.E_UNSUPPORTED:
        raise UnsupportedByEngine(L.lib().sdeng_last_error().decode())
    L.check(rc)


def require_gpu(x: torch.Tensor):
    if not x.is_cuda:
        raise RuntimeError("the sdeng simulate path runs on an MI355X only: move the solver to a cuda device "
                           "(no CPU implementation is shipped)")


def new_desc() -> L.Desc:
    """A fresh sdeng_desc with the ABI version set: the one place it is stamped."""
    return L.Desc(abi_version=L.ABI_VERSION)


@dataclasses.dataclass
class Launched:
    """What a step-loop launch ran on, for the gradient code of the same training call: the loss's declaration of the loop (``decl``, losses/oc.py
    StepLoop), the device table ``coef`` and the compiled parts an adjoint shares with it -- the control's ``net``, the reference drift ``ref``,
    the control's lerp ``prior`` (never a launch's initial density) and, for CMCD, its ``target`` without the terminal clip -- with the tensors
    ``keep`` holds alive for them."""
    coef: torch.Tensor
    net: L.Net
    prior: L.Dist
    ref: L.Ref = None
    target: L.Dist = None
    decl: object = None
    keep: list = dataclasses.field(default_factory=list)


def compile_ctrl(ctrl, coef, device, ref=("none", {}), decl=None) -> Launched:
    """The shared compile step: control, its lerp prior, reference drift and coefficient table as the kernels read them."""
    keep = []
    return Launched(_f32c(coef.to(device=device)), net_desc(ctrl, device, keep), dist_desc(ctrl_target(ctrl)[1], device, keep),
                    ref_desc(ref[0], ref[1], device, keep), decl=decl, keep=keep)


def run(desc: L.Desc, x: torch.Tensor, keep: list, return_traj=False, noise=None, events=None):
    """Fill the I/O pointers of ``desc`` (from ``new_desc``) and launch.  Returns (x_N [B,d], rnd [B,1], xs or None)."""
    require_gpu(x)
    lib = L.lib()
    device = x.device
    B, d, N = x.shape[0], x.shape[1], desc.N
    if isinstance(x, InitialDraw):  # x0 drawn by the engine: no input array
        desc.x_in = None
        desc.x0_dist = x.desc(keep)
        x_out = torch.empty(B, d, dtype=torch.float32, device=device)
    else:
        xin = _f32c(x)
        keep.append(xin)
        desc.x_in = xin.data_ptr()
        x_out = torch.empty_like(xin)
    rnd = torch.empty(B, 1, dtype=torch.float32, device=device)
    xs = torch.empty(N + 1, B, d, dtype=torch.float32, device=device) if return_traj else None
    desc.B, desc.d = B, d
    desc.x_out, desc.rnd_out = x_out.data_ptr(), rnd.data_ptr()
    desc.xs_out = xs.data_ptr() if return_traj else None
    if noise is not None:
        nz = noise.detach().to(device=device, dtype=torch.float32).contiguous()
        assert nz.shape == (N, B, d), f"noise must be [N,B,d] = {(N, B, d)}, got {tuple(nz.shape)}"
        keep.append(nz)
        desc.noise_in = nz.data_ptr()
    else:
        desc.noise_in = None
    need = lib.sdeng_workspace_bytes(C.byref(desc))
    ws = _WS.get(need, device)
    desc.workspace, desc.workspace_bytes = ws.data_ptr(), ws.numel()
    if events is not None:
        desc.ev_start, desc.ev_stop = events.start, events.stop
    _check_supported(lib.sdeng_simulate(C.byref(desc), _stream_ptr(device)))
    return x_out, rnd, xs


def euler_states(sde, timesteps: torch.Tensor, x: torch.Tensor, increments=None, seed: int = 0, particle0: int = 0, events=None):
    """All N+1 Euler-Maruyama states ``[N+1, B, d]`` of ``sde`` on the grid ``timesteps`` in one launch
    (the loop of EulerIntegrator.integrate, eq/integrator.py:113-122: ``xt = xs + drift(s, xs) (t-s) + diff(s, xs) noise``).

    * ``LangevinSDE`` (eq/sdes.py:46-76) and uncontrolled ``OU`` SDEs / ``ControlledSDE(sde, None)`` run the net-free kernel
      (SDENG_CTRL_NONE);
    * ``ControlledSDE(sde, ctrl)`` (eq/sdes.py:681-720; the net is evaluated at ``T - s``) runs the step-loop kernel.
    ``increments`` ``[N,B,d]`` replays Brownian increments (the reference's ``bm(s, t)``); otherwise Philox normals times sqrt(dt).
    """
    require_gpu(x)
    device, keep = x.device, []
    ts = timesteps.detach().to("cpu", torch.float32)
    N = ts.numel() - 1
    desc = new_desc()
    desc.form, desc.flags, desc.N = L.FORM_EM, 0, N
    desc.seed, desc.particle0 = int(seed), int(particle0)
    coef = torch.zeros(N, L.NCOEF, dtype=torch.float32)
    name = _name(sde)
    ctrl = getattr(sde, "ctrl", None) if name == "ControlledSDE" else None
    if name == "LangevinSDE":
        tgt = _self_of(sde.target_score)
        if tgt is None:
            raise UnsupportedByEngine("LangevinSDE.target_score must be a bound Distribution.score")
        desc.target = dist_desc(tgt, device, keep)
        desc.net.ctrl_kind = L.CTRL_NONE
        desc.net.clip_score = float(sde.clip_score) if sde.clip_score else 0.0
        g = sde.diff_coeff.detach().float().cpu()
        coef[:, 2], coef[:, 7] = g, g ** 2 / 2.0  # eq/sdes.py:65
    else:
        base = _cpu_sde(sde.sde if name == "ControlledSDE" else sde)
        if not hasattr(base, "drift_coeff_t"):
            raise UnsupportedByEngine(f"EulerIntegrator: no HIP kernel for SDE {name}")
        T = base.terminal_t
        if ctrl is None:
            desc.net.ctrl_kind = L.CTRL_NONE
        else:
            desc.net = net_desc(ctrl, device, keep)
            tgt, lerp_prior = ctrl_target(ctrl)
            desc.target, desc.prior = dist_desc(tgt, device, keep), dist_desc(lerp_prior, device, keep)
        for k in range(N):
            s = ts[k]
            g = base.diff(s, None)
            coef[k, 0], coef[k, 1], coef[k, 2], coef[k, 3] = T - s, base.drift_coeff_t(s), g, torch.square(g)
            if R.describe_ctrl(ctrl).own_kind == L.CTRL_LERP:  # reparam.py:175, :199 at the net's time T - s
                coef[k, 7], coef[k, 8] = base.diff(T - s, None), (T - s) / T
    dt = ts[1:] - ts[:-1]
    coef[:, 4] = dt
    coef[:, 5] = 1.0 if increments is not None else dt.sqrt()
    coef = coef.to(device)
    keep.append(coef)
    desc.coef = coef.data_ptr()
    _, _, xs = run(desc, x, keep, return_traj=True, noise=increments, events=events)
    return xs


def philox_noise(seed: int, N: int, B: int, d: int, particle0: int, device) -> torch.Tensor:
    """[N,B,d] normals of the step loop's counter-based stream (the kernel draws exactly these when no noise is injected)."""
    lib = L.lib()
    out = torch.empty(N, B, d, dtype=torch.float32, device=device)
    L.check(lib.sdeng_philox_normal_steps(int(seed), 0, N, int(particle0), B, d, 0, out.data_ptr(), _stream_ptr(device)))
    return out


def logz_stats(rnd: torch.Tensor, want_weights=True):
    """sdeng_logz -> (stats[8] device tensor, weights [B,1] or None)."""
    require_gpu(rnd)
    lib = L.lib()
    device = rnd.device
    r = _f32c(rnd).view(-1)
    stats = torch.empty(8, dtype=torch.float32, device=device)
    w = torch.empty(r.numel(), 1, dtype=torch.float32, device=device) if want_weights else None
    ws = torch.empty(lib.sdeng_logz_workspace_bytes(), dtype=torch.uint8, device=device)
    L.check(lib.sdeng_logz(r.data_ptr(), r.numel(), stats.data_ptr(), w.data_ptr() if want_weights else None, ws.data_ptr(),
                           ws.numel(), _stream_ptr(device)))
    return stats, w


# ------------------------------------------------------------------------------------------------
# standalone pieces of the ABI (unit parity tests; also handy for inspection)
# ------------------------------------------------------------------------------------------------
def dist_eval(dist, x: torch.Tensor, want_logp=True, want_score=True):
    """sdeng_dist_eval: log-density [B,1] and score [B,d] of a distribution object, computed in HIP."""
    require_gpu(x)
    lib = L.lib()
    device, keep = x.device, []
    ds = dist_desc(dist, device, keep)
    xin = _f32c(x)
    B, d = xin.shape
    logp = torch.empty(B, 1, dtype=torch.float32, device=device) if want_logp else None
    score = torch.empty(B, d, dtype=torch.float32, device=device) if want_score else None
    need = lib.sdeng_dist_workspace_bytes(C.byref(ds), d)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    L.check(lib.sdeng_dist_eval(C.byref(ds), B, d, xin.data_ptr(), logp.data_ptr() if want_logp else None,
                                score.data_ptr() if want_score else None, ws.data_ptr(), ws.numel(), _stream_ptr(device)))
    return logp, score


def sinkhorn(x: torch.Tensor, y: torch.Tensor, w_x=None, w_y=None, p=2, eps=1e-3, max_iters=100, stop_thresh=1e-5, materialise=True):
    """sdeng_sinkhorn: the entropy-regularised p-Wasserstein distance between the clouds x [n,d] and y [m,d] (eval/sinkhorn.py:64-177).
    Returns a dict: distance (0-d float32 tensor), corr_x_to_y [n], corr_y_to_x [m] (int64), u [n], v [m], iters, max_err_u, max_err_v,
    materialised (the cost matrix was kept in the workspace; ``materialise=False`` asks for the O(n + m) workspace, whose passes
    recompute the costs -- same result)."""
    require_gpu(x)
    require_gpu(y)
    lib = L.lib()
    device = x.device
    xin, yin = _f32c(x), _f32c(y.to(device))
    (n, d), m = xin.shape, yin.shape[0]
    wx = None if w_x is None else _f32c(w_x.to(device))
    wy = None if w_y is None else _f32c(w_y.to(device))
    u, v = torch.empty(n, dtype=torch.float32, device=device), torch.empty(m, dtype=torch.float32, device=device)
    cxy, cyx = torch.empty(n, dtype=torch.int32, device=device), torch.empty(m, dtype=torch.int32, device=device)
    ws = torch.empty(max(lib.sdeng_sinkhorn_workspace_bytes(n, m, d, 1 if materialise else 0), 16), dtype=torch.uint8, device=device)
    res = L.SinkhornResult()
    L.check(lib.sdeng_sinkhorn(xin.data_ptr(), yin.data_ptr(), n, m, d, int(p), float(eps), int(max_iters), float(stop_thresh),
                               wx.data_ptr() if wx is not None else None, wy.data_ptr() if wy is not None else None, u.data_ptr(),
                               v.data_ptr(), cxy.data_ptr(), cyx.data_ptr(), C.byref(res), ws.data_ptr(), ws.numel(), _stream_ptr(device)))
    return {"distance": torch.tensor(res.distance, dtype=torch.float32, device=device), "corr_x_to_y": cxy.long(), "corr_y_to_x": cyx.long(),
            "u": u, "v": v, "iters": res.iters, "max_err_u": res.max_err_u, "max_err_v": res.max_err_v, "materialised": bool(res.materialised)}


def mmd_median(X: torch.Tensor, Y: torch.Tensor):
    """sdeng_mmd_median: (mmd, bandwidth_sq) as 0-d float32 tensors -- the MMD with a Gaussian kernel whose bandwidth is the exact
    lower median of the pooled squared distances (additions/mmd.py:30-59), without an n x n matrix."""
    require_gpu(X)
    require_gpu(Y)
    lib = L.lib()
    device = X.device
    xin, yin = _f32c(X), _f32c(Y.to(device))
    (n, d), m = xin.shape, yin.shape[0]
    out = torch.empty(2, dtype=torch.float32, device=device)
    ws = torch.empty(max(lib.sdeng_mmd_median_workspace_bytes(n, d), 16), dtype=torch.uint8, device=device)
    L.check(lib.sdeng_mmd_median(xin.data_ptr(), yin.data_ptr(), n, m, d, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(device)))
    return out[0], out[1]


def _check_chain_state(who, x, lp, grad, step, n_moves, keep_from, noise, t=None):
    """What every one-launch move kernel indexes (langevin_moves, rwmh_moves, tilted_moves), checked before anything is built or launched.
    ``grad is None``: a move without gradients.  Returns (B, d, n_moves, keep_from)."""
    require_gpu(x)
    if x.dim() != 2:
        raise ValueError(f"{who}: x must be [B, d], got {tuple(x.shape)}")
    B, d = x.shape
    n_moves, keep_from = int(n_moves), int(keep_from)
    if lp.numel() != B or step.numel() != B:
        raise ValueError(f"{who}: lp and step must hold one value per chain (B = {B}), got {lp.numel()} and {step.numel()}")
    if grad is not None and grad.shape != x.shape:
        raise ValueError(f"{who}: grad must have the shape of x {tuple(x.shape)}, got {tuple(grad.shape)}")
    if t is not None and t.numel() not in (1, B):
        raise ValueError(f"{who}: t must hold one tempering weight, or one per chain (B = {B}), got {t.numel()}")
    if not 0 <= keep_from <= n_moves:
        raise ValueError(f"{who}: 0 <= keep_from <= n_moves, got keep_from = {keep_from}, n_moves = {n_moves}")
    injected = isinstance(noise, tuple) and len(noise) == 2 and torch.is_tensor(noise[0])
    if not injected and noise not in ("torch", "philox"):
        raise ValueError("noise: 'torch', 'philox' or the pair (z [n_moves, B, d], u [n_moves, B] or None)")
    state = (("x", x), ("lp", lp), ("step", step)) + ((("grad", grad),) if grad is not None else ())
    if injected:
        if tuple(noise[0].shape) != (n_moves, B, d) or (noise[1] is not None and tuple(noise[1].shape) != (n_moves, B)):
            raise ValueError(f"{who}: injected noise must be z [{n_moves}, {B}, {d}] and u [{n_moves}, {B}]")
        state += (("z", noise[0]),) + ((("u", noise[1]),) if noise[1] is not None else ())
    for ok in (lambda v: v.dtype == torch.float32 and v.is_contiguous(), lambda v: v.is_cuda):
        for name, v in state:
            if not ok(v):
                raise ValueError(f"{who}: {name} must be a contiguous float32 CUDA tensor (the kernel reads and writes it in place)")
    return B, d, n_moves, keep_from


def _move_buffers(noise, n_moves, keep_from, B, d, unadjusted, want_samples, device):
    """(z, u, samples, acc_sum, acc_last) of a one-launch move kernel.  ``noise='torch'``: the reference's consumption order, one randn
    per proposal, then one rand per accept test; a (z, u) pair: the caller's own draws; otherwise z = u = None (Philox in the kernel)."""
    z = u = None
    if isinstance(noise, tuple):
        z, u = noise[0], (noise[1] if not unadjusted else None)
        if u is None and not unadjusted:
            raise ValueError("injected noise: an adjusted move needs the uniforms u as well")
    elif noise == "torch":
        z = torch.empty(n_moves, B, d, dtype=torch.float32, device=device)
        u = torch.empty(n_moves, B, dtype=torch.float32, device=device) if not unadjusted else None
        for m in range(n_moves):
            z[m] = torch.randn((B, d), device=device)
            if u is not None:
                u[m] = torch.rand((B,), device=device)
    samples = torch.empty(n_moves - keep_from, B, d, dtype=torch.float32, device=device) if want_samples else None
    acc = torch.zeros(B, dtype=torch.float32, device=device) if not unadjusted else None
    last = torch.ones(B, dtype=torch.float32, device=device) if not unadjusted else None
    return z, u, samples, acc, last


def _ptr(v):
    return None if v is None else v.data_ptr()


def _chain_moves(who, target, prior, x, lp, grad, step, n_moves, t, keep_from, unadjusted, target_acceptance, noise, seed, chain0, want_samples):
    """The launcher behind langevin_moves and rwmh_moves (``who``; random-walk Metropolis has no prior / grad / t / unadjusted).  Everything
    the kernel indexes is checked here, before anything is built or launched."""
    langevin = who == "langevin_moves"
    B, d, n_moves, keep_from = _check_chain_state(who, x, lp, grad if langevin else None, step, n_moves, keep_from, noise, t)
    if langevin and "Checkerboard" in (_name(target), _name(prior)):
        raise UnsupportedByEngine(f"{who}: no moves on a checkerboard (log-density -inf on a set of positive mass; zero score)")
    lib = L.lib()
    device, keep = x.device, []
    dt = C.byref(dist_desc(target, device, keep))
    dp = C.byref(dist_desc(prior, device, keep)) if prior is not None else None
    z, u, samples, acc, last = _move_buffers(noise, n_moves, keep_from, B, d, unadjusted, want_samples, device)
    tt = None if t is None else t.detach().to(device=device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
    need = lib.sdeng_rwmh_moves_workspace_bytes(dt, d) if not langevin else lib.sdeng_langevin_moves_workspace_bytes(dp, dt, d)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    ptr = _ptr
    tail = (ptr(z), ptr(u), int(seed), int(chain0), ptr(samples), ptr(acc), ptr(last), ws.data_ptr(), ws.numel(), _stream_ptr(device))
    if not langevin:
        L.check(lib.sdeng_rwmh_moves(dt, B, d, n_moves, keep_from, float(target_acceptance), ptr(x), ptr(lp), ptr(step), *tail))
    else:
        L.check(lib.sdeng_langevin_moves(dp, dt, B, d, n_moves, keep_from, int(bool(unadjusted)), float(target_acceptance), ptr(tt), ptr(x), ptr(lp),
                                         ptr(grad), ptr(step), *tail))
    return samples, acc, last


def langevin_moves(target, prior, x, lp, grad, step, n_moves, *, t=None, keep_from=0, unadjusted=False, target_acceptance=0.0, noise="torch",
                   seed=0, chain0=0, want_samples=True):
    """sdeng_langevin_moves: ``n_moves`` MALA / ULA moves of all chains in one launch (include/sdeng.h).  ``x`` [B,d], ``lp`` [B], ``grad``
    [B,d], ``step`` [B] are updated IN PLACE.  ``noise='torch'``: the normals (and uniforms) are drawn from torch's generator move by move in
    the order additions/mcmc.py consumes them (randn((B,d)) then rand_like(lp)), so a chain is the one the reference's loop produces;
    ``noise='philox'``: drawn in the kernel.  Returns (samples [n_moves - keep_from, B, d] or None, acc_sum [B] or None, acc_last [B] or None)."""
    return _chain_moves("langevin_moves", target, prior, x, lp, grad, step, n_moves, t, keep_from, unadjusted, target_acceptance, noise, seed,
                        chain0, want_samples)


def rwmh_moves(target, x, lp, step, n_moves, *, keep_from=0, target_acceptance=0.0, noise="torch", seed=0, chain0=0, want_samples=True):
    """sdeng_rwmh_moves: ``n_moves`` random-walk Metropolis moves of all chains in one launch (include/sdeng.h).  ``x`` [B,d], ``lp`` [B],
    ``step`` [B] are updated IN PLACE.  ``noise='torch'``: per move ``torch.randn((B, d))`` then ``torch.rand((B,))`` on the device, the order
    additions/mcmc.py:rwmh_step consumes them; ``noise='philox'``: drawn in the kernel (streams 6 / 7).  Everything the kernel indexes is
    checked here.  Returns (samples [n_moves - keep_from, B, d] or None, acc_sum [B], acc_last [B])."""
    return _chain_moves("rwmh_moves", target, None, x, lp, None, step, n_moves, None, keep_from, False, target_acceptance, noise, seed, chain0,
                        want_samples)


def _net_only_desc(ctrl, t_unique: torch.Tensor, n_times: int, d: int, device, keep: list, who="ctrl_vjp", own_workspace=False):
    """The descriptor sdeng_ctrl_vjp reads -- the drift net of a ClippedCtrl, a coefficient table that holds only the ``n_times`` times (column 0),
    the shared workspace or one of its ``own`` (its weight images then survive other engine calls) -> (desc, coef, workspace), for the caller to keep alive."""
    desc = new_desc()
    desc.net = net_desc(ctrl, device, keep)
    if desc.net.ctrl_kind != L.CTRL_CLIPPED:
        raise UnsupportedByEngine(f"{who}: ClippedCtrl only")
    desc.d = d
    coef = torch.zeros(n_times, L.NCOEF, dtype=torch.float32, device=device)
    coef[:, 0] = t_unique.detach().to(device=device, dtype=torch.float32).reshape(-1)
    desc.coef = coef.data_ptr()
    need = L.lib().sdeng_ctrl_vjp_workspace_bytes(d, n_times)
    ws = torch.empty(need, dtype=torch.uint8, device=device) if own_workspace else _WS.get(need, device)
    desc.workspace, desc.workspace_bytes = ws.data_ptr(), ws.numel()
    return desc, coef, ws


class _RowArrays:
    """The per-row arrays the three training kernels write and the parameter gradients are built from (include/sdeng.h): the drift net's
    activations a0, a1, a2 and cotangents d0, d1, d2 [rows, 64] and ``dout`` [rows, d], next to the states ``x`` [rows, d] they belong to."""

    def __init__(self, x: torch.Tensor):
        self.x = x
        self.hid = torch.empty(6, x.shape[0], 64, dtype=torch.float32, device=x.device)
        self.dout = torch.empty_like(x)

    def pointers(self, first_row=0, d=0):  # a0 .. d2, dout from row ``first_row`` on: sdeng_ctrl_vjp's arguments, the fields of an Adjoint / CmcdAdjoint
        return [self.hid[i].data_ptr() + 4 * 64 * first_row for i in range(6)] + [self.dout.data_ptr() + 4 * d * first_row]

    def into(self, adj):
        adj.a0, adj.a1, adj.a2, adj.d0, adj.d1, adj.d2, adj.dout = self.pointers()

    def result(self, gx=None, **more):
        h = self.hid
        return dict(x=self.x, a0=h[0], a1=h[1], a2=h[2], d0=h[3], d1=h[4], d2=h[5], dout=self.dout, gx=gx, **more)


def ctrl_vjp(ctrl, t_unique: torch.Tensor, xs: torch.Tensor, cot: torch.Tensor, want_gx=False):
    """sdeng_ctrl_vjp: fused forward + backward of a ClippedCtrl / FourierMLP over all (time, state) rows.  ``xs`` and ``cot`` are
    [N, B, d] (states at the N times ``t_unique`` and the cotangent of the control there).  Returns the per-row arrays the parameter
    gradients are built from (include/sdeng.h): dict(a0, a1, a2, d0, d1, d2 [N*B, 64], dout [N*B, d], gx [N*B, d] or None)."""
    require_gpu(xs)
    device, keep = xs.device, []
    N, B, d = xs.shape
    desc, coef, ws = _net_only_desc(ctrl, t_unique, N, d, device, keep)
    rows = _RowArrays(_f32c(xs).view(N * B, d))
    c2 = _f32c(cot).view(N * B, d)
    gx = torch.empty(N * B, d, dtype=torch.float32, device=device) if want_gx else None
    L.check(L.lib().sdeng_ctrl_vjp(C.byref(desc), N, B, rows.x.data_ptr(), c2.data_ptr(), *rows.pointers(), gx.data_ptr() if want_gx else None,
                                   None, _stream_ptr(device)))
    return rows.result(gx=gx)


class VjpSession:
    """sdeng_ctrl_vjp for a caller that walks the N times one by one (the adjoint recursion of KL training): the weight images are packed
    once, ``forward_u`` evaluates the control on all N * B rows, ``step(k, cot_k)`` runs the fused forward + backward of time k alone
    (cotangent [B, d]) -- its per-row arrays land in row block k of the session's [N * B, .] arrays -- and returns the state gradient
    [B, d].  After the walk the arrays are exactly what ``ctrl_vjp`` returns for the whole batch."""

    def __init__(self, ctrl, t_unique: torch.Tensor, xs: torch.Tensor):
        require_gpu(xs)
        self.lib, self.device, self.keep = L.lib(), xs.device, []
        self.N, self.B, self.d = N, B, d = xs.shape
        self.desc, self.coef, self.ws = _net_only_desc(ctrl, t_unique, N, d, self.device, self.keep, own_workspace=True)  # its own: the images must survive
        self.rows = _RowArrays(_f32c(xs).view(N * B, d))
        self.gx = torch.empty(B, d, dtype=torch.float32, device=self.device)
        self.packed = False

    def forward_u(self) -> torch.Tensor:
        u = torch.empty(self.N * self.B, self.d, dtype=torch.float32, device=self.device)
        self.desc.coef, self.desc.flags = self.coef.data_ptr(), 0
        L.check(self.lib.sdeng_ctrl_vjp(C.byref(self.desc), self.N, self.B, self.rows.x.data_ptr(), None, None, None, None, None, None, None, None, None,
                                        u.data_ptr(), _stream_ptr(self.device)))
        self.packed = True
        return u.view(self.N, self.B, self.d)

    def step(self, k: int, cot: torch.Tensor) -> torch.Tensor:
        B, d = self.B, self.d
        c = _f32c(cot)
        self.keep.append(c)
        self.desc.coef = self.coef.data_ptr() + 4 * L.NCOEF * k
        self.desc.flags = L.FLAG_REUSE_PACK if self.packed else 0
        L.check(self.lib.sdeng_ctrl_vjp(C.byref(self.desc), 1, B, self.rows.x.data_ptr() + 4 * d * B * k, c.data_ptr(), *self.rows.pointers(B * k, d),
                                        self.gx.data_ptr(), None, _stream_ptr(self.device)))
        self.packed = True
        self.keep.clear()
        return self.gx

    def arrays(self):
        return self.rows.result()


def kl_adjoint(ctrl, coef: torch.Tensor, xs: torch.Tensor, z, w: torch.Tensor, lam_n: torch.Tensor, *, lin: bool, ito: bool, ref=("none", {}), parts=None):
    """sdeng_kl_adjoint: the whole adjoint recursion of KL training in one launch (ClippedCtrl, or ScoreCtrl on a diagonal mixture target; no
    reference, or a diagonal Gaussian / mixture reference).  ``coef`` [N,16] on the device, ``xs`` [N,B,d] = x_0 .. x_{N-1}, ``z`` [N,B,d]
    the trajectory's normals (or None), ``w`` [B,1] = d loss / d rnd, ``lam_n`` [B,d] = lambda_N.  ``parts``: the ``Launched`` record of the step
    loop this is the adjoint of -- its net, lerp prior, reference and table as compiled (``coef`` must then be ``parts.coef`` itself and ``ref`` is the
    record's).  The control's own target is compiled here: the step loop's slot holds the terminal target.  Returns (per-row arrays as ``ctrl_vjp``
    -- plus ``dst`` [N,B], the per-particle cotangent of s_theta(t_k), for a ScoreCtrl --, lambda_0)."""
    require_gpu(xs)
    lib = L.lib()
    device, keep = xs.device, []
    N, B, d = xs.shape
    if parts is not None and coef is not parts.coef:
        raise ValueError("kl_adjoint: with parts, coef must be the table of that launch (parts.coef)")
    parts = parts or compile_ctrl(ctrl, coef, device, ref)
    desc = new_desc()
    desc.form = L.FORM_LIN if lin else L.FORM_EM
    desc.flags = L.FLAG_ITO if ito else 0
    desc.B, desc.d, desc.N = B, d, N
    desc.net, desc.prior, desc.ref, desc.coef = parts.net, parts.prior, parts.ref, parts.coef.data_ptr()
    if not adjoint_ctrl_ok(ctrl):
        raise UnsupportedByEngine("kl_adjoint: ClippedCtrl, or ScoreCtrl on a diagonal mixture target")
    score = desc.net.ctrl_kind != L.CTRL_CLIPPED
    ext_score = None
    tgt = ctrl_target(ctrl)[0]  # None for a ClippedCtrl: a SDENG_DIST_NONE descriptor
    if R.dist_kind(tgt) in R.GRAPHLESS_TARGETS:
        _, ext_score = dist_eval(tgt, xs.reshape(N * B, d), want_logp=False, want_score=True)
    else:
        desc.target = dist_desc(tgt, device, keep)
    if desc.ref.kind not in (L.REF_NONE, L.REF_GAUSS_DIAG, L.REF_GMM_DIAG):
        raise UnsupportedByEngine("kl_adjoint: diagonal references only")
    rows = _RowArrays(_f32c(xs).view(N * B, d))
    lam0 = torch.empty(B, d, dtype=torch.float32, device=device)
    wv, ln = _f32c(w).view(B), _f32c(lam_n)
    zz = _f32c(z) if (ito and z is not None) else None
    ws = _WS.get(lib.sdeng_kl_adjoint_workspace_bytes(C.byref(desc)), device)
    desc.workspace, desc.workspace_bytes = ws.data_ptr(), ws.numel()
    adj = L.Adjoint()
    adj.xs, adj.noise, adj.w, adj.lam_in, adj.lam_out = rows.x.data_ptr(), (zz.data_ptr() if zz is not None else None), wv.data_ptr(), ln.data_ptr(), lam0.data_ptr()
    rows.into(adj)
    dst = torch.empty(N, B, dtype=torch.float32, device=device) if score else None
    if score:
        adj.dst, adj.detach_score = dst.data_ptr(), int(bool(ctrl.detach_score))
        adj.score = ext_score.data_ptr() if ext_score is not None else None
    L.check(lib.sdeng_kl_adjoint(C.byref(desc), C.byref(adj), _stream_ptr(device)))
    return rows.result(dst=dst), lam0


def ctrl_forward_rows(ctrl, t_unique: torch.Tensor, xs: torch.Tensor) -> torch.Tensor:
    """u = ctrl(t_k, xs[k]) for a ClippedCtrl over all rows of ``xs`` [M,B,d] in one launch (sdeng_ctrl_vjp without a cotangent): [M,B,d]."""
    require_gpu(xs)
    device, keep = xs.device, []
    M, B, d = xs.shape
    desc, coef, ws = _net_only_desc(ctrl, t_unique, M, d, device, keep, who="ctrl_forward_rows")
    x2 = _f32c(xs).view(M * B, d)
    u = torch.empty(M * B, d, dtype=torch.float32, device=device)
    L.check(L.lib().sdeng_ctrl_vjp(C.byref(desc), M, B, x2.data_ptr(), None, None, None, None, None, None, None, None, None, u.data_ptr(),
                                   _stream_ptr(device)))
    return u.view(M, B, d)


def cmcd_desc(ctrl, sde, coef, device, form=L.FORM_CMCD, parts=None, decl=None):
    """CMCD's descriptor without its sizes, flags and I/O, for the step loop, the EUBO loop and the adjoint alike -> (desc, ``parts``).  Compiled
    here unless ``parts`` (an earlier launch's record) is given: control, target, prior (``Launched.target``: no clip -- a forward launch adds
    the terminal clip to its own copy)."""
    if parts is None:
        keep = []
        net = net_desc(ctrl, device, keep)
        target, prior = _self_of(sde.target_score), _self_of(sde.prior_score)
        if target is None or prior is None:
            raise UnsupportedByEngine("ControlledLangevinSDE.target_score / prior_score must be bound Distribution.score methods")
        parts = Launched(_f32c(coef.to(device=device)), net, dist_desc(prior, device, keep), target=dist_desc(target, device, keep), decl=decl, keep=keep)
    desc = new_desc()
    desc.form = form
    desc.net, desc.target, desc.prior, desc.coef = parts.net, parts.target, parts.prior, parts.coef.data_ptr()
    desc.cmcd_g = scalar_of(sde.diff_coeff)
    desc.cmcd_clip = scalar_of(sde.clip_score) if sde.clip_score else 0.0
    return desc, parts


def cmcd_kl_adjoint(ctrl, sde, coef: torch.Tensor, xs: torch.Tensor, cbar: torch.Tensor, w: torch.Tensor, lam_n: torch.Tensor, score_ext=None, parts=None):
    """sdeng_cmcd_kl_adjoint: the adjoint of CMCD's KL training over the N + 1 evaluation points in one launch.  ``coef`` [N+1,16] the CMCD
    table of the step loop (device), ``xs`` [N+1,B,d] = x_0 .. x_N, ``cbar`` [N,B,d] = cost_j dt_j + db_j, ``w`` [B,1] = d loss / d rnd,
    ``lam_n`` [B,d] = d (sum w (-log pi~(x_N))) / d x_N.  ``score_ext`` [(N+1)*B,d]: the target score of every row for a graph-less target
    (evaluated here when not given).  ``parts``: the ``Launched`` record of the step loop this is the adjoint of (``coef`` must then be
    ``parts.coef`` itself; compiled here otherwise).
    Returns (per-row arrays as ``kl_adjoint`` over the (N+1)*B rows, Lambda_0)."""
    require_gpu(xs)
    if xs.dim() != 3 or cbar.dim() != 3:
        raise ValueError(f"cmcd_kl_adjoint: xs [N+1,B,d] and cbar [N,B,d] expected, got {tuple(xs.shape)} and {tuple(cbar.shape)}")
    M, B, d = xs.shape
    N = M - 1
    if N < 1 or tuple(cbar.shape) != (N, B, d) or w.numel() != B or tuple(lam_n.shape) != (B, d) or tuple(coef.shape) != (M, L.NCOEF):
        raise ValueError(f"cmcd_kl_adjoint: shapes disagree: xs {tuple(xs.shape)}, cbar {tuple(cbar.shape)} (want {(N, B, d)}), w {tuple(w.shape)} "
                         f"(want {B} entries), lam_n {tuple(lam_n.shape)} (want {(B, d)}), coef {tuple(coef.shape)} (want {(M, L.NCOEF)})")
    lib = L.lib()
    device = xs.device
    if parts is not None and coef is not parts.coef:
        raise ValueError("cmcd_kl_adjoint: with parts, coef must be the table of that launch (parts.coef)")
    desc, parts = cmcd_desc(ctrl, sde, coef, device, parts=parts)
    desc.B, desc.d, desc.N = B, d, N
    rows = _RowArrays(_f32c(xs).view(M * B, d))
    if desc.target.kind in R.GRAPHLESS_TARGETS and score_ext is None:
        _, score_ext = dist_eval(_self_of(sde.target_score), rows.x, want_logp=False, want_score=True)
    if score_ext is not None:
        score_ext = _f32c(score_ext)
        if tuple(score_ext.shape) != (M * B, d):
            raise ValueError(f"cmcd_kl_adjoint: score_ext {tuple(score_ext.shape)}, want {(M * B, d)}")
    cb = _f32c(cbar)
    lam0 = torch.empty(B, d, dtype=torch.float32, device=device)
    wv, ln = _f32c(w).view(B), _f32c(lam_n)
    ws = _WS.get(lib.sdeng_cmcd_kl_adjoint_workspace_bytes(C.byref(desc)), device)
    desc.workspace, desc.workspace_bytes = ws.data_ptr(), ws.numel()
    adj = L.CmcdAdjoint()
    adj.xs, adj.cbar, adj.w, adj.lam_in, adj.lam_out = rows.x.data_ptr(), cb.data_ptr(), wv.data_ptr(), ln.data_ptr(), lam0.data_ptr()
    rows.into(adj)
    score = desc.net.ctrl_kind != L.CTRL_CLIPPED
    dst = torch.empty(M, B, dtype=torch.float32, device=device) if score else None
    if score:
        adj.dst, adj.detach_score = dst.data_ptr(), int(bool(ctrl.detach_score))
    adj.score = score_ext.data_ptr() if score_ext is not None else None
    L.check(lib.sdeng_cmcd_kl_adjoint(C.byref(desc), C.byref(adj), _stream_ptr(device)))
    return rows.result(dst=dst), lam0


def ctrl_forward(ctrl, t: float, x: torch.Tensor, score_gain=1.0, lerp_w=0.0):
    """sdeng_ctrl_forward: u = ctrl(t, x) for a ClippedCtrl / ScoreCtrl / LerpCtrl module, computed in HIP."""
    require_gpu(x)
    lib = L.lib()
    device, keep = x.device, []
    desc = new_desc()
    desc.net = net_desc(ctrl, device, keep)
    tgt, prior = ctrl_target(ctrl)
    desc.target = dist_desc(tgt, device, keep)
    desc.prior = dist_desc(prior, device, keep)
    xin = _f32c(x)
    desc.B, desc.d, desc.N = xin.shape[0], xin.shape[1], 1
    out = torch.empty_like(xin)
    need = lib.sdeng_workspace_bytes(C.byref(desc))
    ws = _WS.get(need, device)
    desc.workspace, desc.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(lib.sdeng_ctrl_forward(C.byref(desc), float(t), float(score_gain), float(lerp_w), xin.data_ptr(), out.data_ptr(),
                                   _stream_ptr(device)))
    return out


# ------------------------------------------------------------------------------------------------
# energy-based (tilted-potential) references: GMMTitledPotential / GaussTiltedPotential (models/reparam.py:277-606)
# ------------------------------------------------------------------------------------------------
_TILTS = {"dot": L.TILT_DOT, "sq_norm": L.TILT_SQ_NORM}
_TILTED_CLASSES = R.TILTED_CLASSES


def _tilted_mixture(net):
    """(weights [K], means [K,d], vars [K,d], eigvecs [K,d,d] or None) of the prior of a tilted potential, full covariances in the
    eigen form (D, P): as given (``use_full_decomp``), or decomposed in float64 once per parameter version (``_EIGH``)."""
    if _name(net) == "GaussTiltedPotential":
        weights, means, var = torch.ones(1, device=net.mean.device), net.mean.reshape(1, -1), net.variance.unsqueeze(0)
        full = bool(getattr(net, "is_full_cov_type", False))
    else:
        weights, means, var = net.weights, net.means, net.variances
        full = bool(getattr(net, "is_full_gmm_type", False))
    if not full:
        return weights, means, var, None
    if getattr(net, "use_full_decomp", False):
        D, P = net.cov_D, net.cov_P
        return weights, means, D.reshape(means.shape), P.reshape(means.shape[0], means.shape[1], means.shape[1])
    src = net.variance if _name(net) == "GaussTiltedPotential" else net.variances
    eig = _EIGH.get(src, lambda v: torch.linalg.eigh(v.detach().double()))
    return weights, means, eig[0].float().reshape(means.shape), eig[1].float().reshape(means.shape[0], means.shape[1], means.shape[1])


def tilted_desc(net, device, keep) -> L.Tilted:
    """Tilted-potential object -> sdeng_tilted without its per-call fields (x, tinfo, outputs, workspace).  Accepts this package's
    classes and the reference's own objects, by class name and attributes."""
    if _name(net) not in _TILTED_CLASSES:
        raise UnsupportedByEngine(f"tilted_eval: {_name(net)} is not a GMMTitledPotential / GaussTiltedPotential")
    base = net.base_model
    if _name(base) != "FourierMLP" or not hasattr(base, "timestep_embed"):
        raise UnsupportedByEngine(f"tilted_eval: base_model must be a FourierMLP, got {_name(base)}")
    if _name(base.activation) != "GELU" or getattr(base.activation, "approximate", "none") != "none":
        raise UnsupportedByEngine("tilted_eval: the kernel evaluates the exact GELU only")
    te = base.timestep_embed
    d = L.Tilted()
    d.abi_version = L.ABI_VERSION
    d.d = int(net.dim)
    d.num_layers, d.channels = len(base.hidden_layer) + 2, int(base.channels)
    d.tilt_type = _TILTS.get(net.tilt_type, L.TILT_SUM)
    d.use_scaling_factor, d.use_s_t_scaling = int(bool(net.use_scaling_factor)), int(bool(net.use_s_t_scaling))
    if len(te.hidden_layer) != 1 or int(te.channels) != int(base.channels):
        raise UnsupportedByEngine("tilted_eval: the time embedding must be TimeEmbed(num_layers=2) of the net's width")
    weights, means, var, eigvecs = _tilted_mixture(net)
    d.k, d.full_cov = int(means.shape[0]), int(eigvecs is not None)
    d.w_in, d.b_in = _dev_f32(base.input_embed.weight, device, keep), _dev_f32(base.input_embed.bias, device, keep)
    for i, layer in enumerate(list(base.hidden_layer)[:4]):
        d.w_h[i], d.b_h[i] = _dev_f32(layer.weight, device, keep), _dev_f32(layer.bias, device, keep)
    d.w_out, d.b_out = _dev_f32(base.out_layer.weight, device, keep), _dev_f32(base.out_layer.bias, device, keep)
    d.te_coeff, d.te_phase = _dev_f32(te.timestep_coeff.reshape(-1), device, keep), _dev_f32(te.timestep_phase.reshape(-1), device, keep)
    d.te_w1, d.te_b1 = _dev_f32(te.hidden_layer[0].weight, device, keep), _dev_f32(te.hidden_layer[0].bias, device, keep)
    d.te_w2, d.te_b2 = _dev_f32(te.out_layer.weight, device, keep), _dev_f32(te.out_layer.bias, device, keep)
    d.mean_gauss, d.var_gauss = _dev_f32(net.mean_gauss.reshape(-1), device, keep), _dev_f32(net.var_gauss.reshape(-1), device, keep)
    d.weights, d.means, d.vars = _dev_f32(weights, device, keep), _dev_f32(means, device, keep), _dev_f32(var, device, keep)
    d.eigvecs = _dev_f32(eigvecs, device, keep) if eigvecs is not None else None
    return d


def tilted_times(net, t: torch.Tensor, M: int, per_row=False):
    """``t`` (scalar, (1,1) or M values) -> (n_times, rows_per_time, tinfo [n_times,5] float32 on the CPU).  Runs of equal consecutive
    times of equal length become (N, B); anything else -- or everything, with ``per_row`` -- N = M, B = 1.  The five scalars per time -- t, s(t), sigma_sq(t) and the last two
    at max(t, t_limit) -- are the SDE object's own float32 expressions (models/reparam.py:361, :422-423)."""
    tf = t.detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    if tf.numel() == 1 and not per_row:
        tu, B = tf, M
    elif per_row and tf.numel() in (1, M):
        tu, B = tf.expand(M), 1
    elif tf.numel() == M:
        change = torch.nonzero(tf[1:] != tf[:-1]).reshape(-1) + 1
        starts = torch.cat([torch.zeros(1, dtype=torch.long), change])
        lengths = torch.diff(torch.cat([starts, torch.tensor([M])]))
        if bool((lengths == lengths[0]).all()):
            tu, B = tf[starts], int(lengths[0])
        else:
            tu, B = tf, 1
    else:
        raise ValueError(f"tilted_eval: t has {tf.numel()} values for {M} rows (a scalar, (1, 1) or one per row)")
    sde = _cpu_sde(net.sde)
    tc = tu.reshape(-1, 1)
    tl = torch.maximum(tc, float(net.t_limit) * torch.ones_like(tc))
    cols = [tc, sde.s(tc), sde.sigma_sq(tc), sde.s(tl), sde.sigma_sq(tl)]
    tinfo = torch.cat([c.to(torch.float32).expand(tc.shape[0], 1) if torch.is_tensor(c) else torch.full_like(tc, float(c)) for c in cols], dim=1)
    return int(tu.numel()), B, tinfo.contiguous()


_TILTED_TIMES = _TensorCache()
_TILTED_PACKS = weakref.WeakKeyDictionary()  # net -> (parameter versions, workspace holding its packed images)


def _tilted_versions(net, device):
    return tuple((id(p), p._version, p.data_ptr(), str(p.device)) for p in list(net.parameters()) + list(net.buffers())) + (str(device),)


def tilted_needs_param_grad(net) -> bool:
    return torch.is_grad_enabled() and any(p.requires_grad for p in net.parameters())


def tilted_eval(net, t, x: torch.Tensor, want_grad=True, want_logp=True, per_row_times=False):
    """sdeng_tilted_eval: (log_prob [M], grad [M,d]) of an energy-based reference at the rows (t, x), in one HIP launch -- what
    ``net.unnorm_log_prob_and_grad(t, x)`` computes with autograd in the reference (models/reparam.py:457-476).  The packed weight
    images live in a workspace of the net's own and are re-made only when a parameter or buffer changed.  ``per_row_times``: present the
    rows as N = M times of one row each whatever ``t`` holds (same results; for tests)."""
    if tilted_needs_param_grad(net):
        raise UnsupportedByEngine("tilted_eval computes no gradient with respect to the net's parameters: call it under torch.no_grad() "
                                  "or with requires_grad_(False) parameters; first-order parameter gradients of net.energy / "
                                  "net.unnorm_log_prob are the opt-in net.param_grads = True (tilted_vjp), the score's are not on the HIP path")
    return _tilted_launch(net, t, x, want_grad, want_logp, per_row_times, False)[:2]


def _tilted_rows_desc(net, t, M, dim, device, keep, per_row_times=False):
    """sdeng_tilted of ``net`` over M rows at the times ``t``, without its state, outputs and workspace; and (n_times, B, time table on the
    device).  The time table of a tensor the samplers pass again and again is made once (reading a device tensor back waits for the stream)."""
    t = torch.as_tensor(t)
    def table(tt, per_row=False):
        n, b, info = tilted_times(net, tt, M, per_row)
        return n, b, info.to(device)
    owner, rows, times = _TILTED_TIMES.get(t, lambda tt: (weakref.ref(net), (M, str(device)), table(tt)))
    n_times, B, tdev = times if owner() is net and rows == (M, str(device)) and not per_row_times else table(t, per_row_times)
    d = tilted_desc(net, device, keep)
    if d.d != dim:
        raise ValueError(f"tilted_eval: x has {dim} features, the potential {d.d}")
    d.M, d.n_times, d.rows_per_time = M, n_times, B
    keep.append(tdev)
    d.tinfo = tdev.data_ptr()
    return d, (n_times, B, tdev)


def _tilted_workspace(net, d, need, device):
    """The workspace of a tilted launch into ``d``: the net's own, whose head holds the packed images (every tilted entry point keeps them
    in the same place), re-made only when a parameter or buffer changed or the call needs more room."""
    versions = _tilted_versions(net, device)
    hit = _TILTED_PACKS.get(net)
    if hit is not None and hit[0] == versions and hit[1].numel() >= need:
        ws, d.flags = hit[1], L.FLAG_REUSE_PACK
    else:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        _TILTED_PACKS[net] = (versions, ws)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()


def _tilted_run(net, d, need, launch, device):
    """Launch into ``d`` with the net's workspace of ``need`` bytes; ``need`` 0 means the size query rejected the descriptor: one launch
    without a workspace fetches the code and the reason."""
    if need == 0:
        _check_supported(launch())
    _tilted_workspace(net, d, need, device)
    _check_supported(launch())


def _tilted_launch(net, t, x, want_grad, want_logp, per_row_times, train):
    """The one launch behind tilted_eval (sdeng_tilted_eval) and tilted_vjp (``train``: sdeng_tilted_vjp, with the per-row arrays)."""
    require_gpu(x)
    lib = L.lib()
    device, keep = x.device, []
    xin = _f32c(x)
    if xin.dim() != 2:
        raise ValueError("tilted_eval: x must be [M, d]")
    M, dim = xin.shape
    d, (n_times, B, tdev) = _tilted_rows_desc(net, t, M, dim, device, keep, per_row_times)
    d.x = xin.data_ptr()
    logp = torch.empty(M, dtype=torch.float32, device=device) if want_logp else None
    grad = torch.empty(M, dim, dtype=torch.float32, device=device) if want_grad else None
    d.log_prob, d.grad = (logp.data_ptr() if want_logp else None), (grad.data_ptr() if want_grad else None)
    arrays, rows = None, None
    if train:
        hid, io = torch.empty(10, M, 128, dtype=torch.float32, device=device), torch.empty(2, M, dim, dtype=torch.float32, device=device)
        arrays = {"a": list(hid[:5]), "d": list(hid[5:]), "xs": io[0], "dv": io[1], "a_all": hid[:5], "d_all": hid[5:]}
        rows = L.TiltedRows()
        for l in range(5):
            rows.a[l], rows.d[l] = arrays["a"][l].data_ptr(), arrays["d"][l].data_ptr()
        rows.xs, rows.dv = io[0].data_ptr(), io[1].data_ptr()
        launch = lambda: lib.sdeng_tilted_vjp(C.byref(d), C.byref(rows), _stream_ptr(device))  # noqa: E731
        need = lib.sdeng_tilted_vjp_workspace_bytes(C.byref(d))
    else:
        launch = lambda: lib.sdeng_tilted_eval(C.byref(d), _stream_ptr(device))  # noqa: E731
        need = lib.sdeng_tilted_eval_workspace_bytes(C.byref(d))
    _tilted_run(net, d, need, launch, device)
    return logp, grad, arrays, (n_times, B, tdev[:, 0])


def tilted_refusal(net, device):
    """Why ``tilted_eval`` / ``tilted_moves`` would refuse ``net`` as it stands -- the reason, in words -- or None: the checks of the
    descriptor compiler and of the library on the net, made without a launch.  The samplers' route decision asks this before it commits
    a level to the one-launch path; a refused net stays on the host loop, whose first evaluation raises the error itself."""
    if tilted_needs_param_grad(net):
        return "trainable parameters in grad mode"
    try:
        d = tilted_desc(net, device, [])
    except UnsupportedByEngine as e:
        return str(e)
    if (d.num_layers, d.channels) != (6, 128):
        return f"FourierMLP(num_layers={d.num_layers}, channels={d.channels}): the kernel is built for 6 x 128"
    if d.tilt_type != L.TILT_DOT:
        return f"tilt_type {net.tilt_type!r}: the kernel has 'dot'"
    if d.use_scaling_factor:
        return "use_scaling_factor (DRL)"
    if not 1 <= d.d <= 128 or not 1 <= d.k <= 16:
        return f"d = {d.d}, k = {d.k} outside the kernel's range"
    return None


def tilted_moves(net, t, x, lp, grad, step, n_moves, *, keep_from=0, unadjusted=False, target_acceptance=0.0, noise="torch", seed=0, chain0=0,
                 want_samples=True):
    """sdeng_tilted_moves: ``n_moves`` MALA / ULA moves of all chains over the energy-based reference ``net`` in one launch
    (include/sdeng.h) -- ``langevin_moves`` with the density of ``tilted_eval``.  ``t``: the chains' times, as ``tilted_eval`` takes them (a
    scalar, or one per row; rows of unequal runs become one time per chain).  ``x`` [M,d], ``lp`` [M], ``grad`` [M,d] (``tilted_eval`` at
    ``x``) and ``step`` [M] are updated IN PLACE.  ``noise='torch'``: per move ``randn((M, d))`` then ``rand((M,))`` from torch's generator,
    the order additions/mcmc.py consumes them; ``noise='philox'``: drawn in the kernel (streams 8 / 9, keyed by ``seed`` and ``chain0`` + row);
    a pair ``(z [n_moves, M, d], u [n_moves, M])``: the caller's own draws.  Refusals are ``tilted_eval``'s.
    Returns (samples [n_moves - keep_from, M, d] or None, acc_sum [M] or None, acc_last [M] or None)."""
    who = "tilted_moves"
    M, dim, n_moves, keep_from = _check_chain_state(who, x, lp, grad, step, n_moves, keep_from, noise)
    if tilted_needs_param_grad(net):
        raise UnsupportedByEngine("tilted_moves computes no gradient with respect to the net's parameters: call it under torch.no_grad() "
                                  "or with requires_grad_(False) parameters")
    lib = L.lib()
    device, keep = x.device, []
    d, _ = _tilted_rows_desc(net, t, M, dim, device, keep)
    z, u, samples, acc, last = _move_buffers(noise, n_moves, keep_from, M, dim, unadjusted, want_samples, device)
    mv = L.TiltedMovesState()
    mv.n_moves, mv.keep_from, mv.unadjusted, mv.target_acceptance = n_moves, keep_from, int(bool(unadjusted)), float(target_acceptance)
    mv.x, mv.lp, mv.grad, mv.step = x.data_ptr(), lp.data_ptr(), grad.data_ptr(), step.data_ptr()
    mv.z, mv.u, mv.seed, mv.chain0 = _ptr(z), _ptr(u), int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain0)
    mv.samples, mv.acc_sum, mv.acc_last = _ptr(samples), _ptr(acc), _ptr(last)
    _tilted_run(net, d, lib.sdeng_tilted_moves_workspace_bytes(C.byref(d)),
                lambda: lib.sdeng_tilted_moves(C.byref(d), C.byref(mv), _stream_ptr(device)), device)
    return samples, acc, last


def tilted_simulate(net, ctrl, coef: torch.Tensor, tinfo: torch.Tensor, x: torch.Tensor, *, form=None, flags=None, seed=0, particle0=0,
                    noise=None, return_traj=False, want_ref=False):
    """sdeng_tilted_simulate: all N steps of an RDS ``simulate()`` loop over the energy-based reference ``net`` in one launch
    (include/sdeng.h) -- the reference score of ``tilted_eval`` at (t_k, x_k), the control ``ctrl`` (ClippedCtrl around the 4 x 64
    FourierMLP), the noise of Philox stream 0 keyed by ``seed`` and ``particle0`` + row (``philox_noise`` replays it) or ``noise``
    [N,B,d], the update and the running cost of ``form`` (``L.FORM_LIN``, the default, or ``L.FORM_EM``; ``flags``: ``L.FLAG_ITO``, the
    default, or 0).  ``coef`` [N, NCOEF] is the step loop's table (``coef_table``), ``tinfo`` [N, 5] the reference's times at
    ``coef[:, 0]`` (``tilted_times``).  Terminal costs are the caller's.  Refusals are ``tilted_eval``'s and the entry point's own.
    Returns (x_N [B,d], rnd [B,1], xs [N+1,B,d] or None, ref [N,B,d] or None: the reference score the kernel used at every step)."""
    require_gpu(x)
    if tilted_needs_param_grad(net):
        raise UnsupportedByEngine("tilted_simulate computes no gradient with respect to the reference net's parameters: freeze them "
                                  "(RDS.change_reference_type('nn') does) or call it under torch.no_grad()")
    lib = L.lib()
    device, keep = x.device, []
    xin = _f32c(x)
    if xin.dim() != 2:
        raise ValueError("tilted_simulate: x must be [B, d]")
    B, dim = xin.shape
    coef = coef.detach().to(device=device, dtype=torch.float32).contiguous()
    tdev = tinfo.detach().to(device=device, dtype=torch.float32).contiguous()
    N = coef.shape[0]
    if coef.shape != (N, L.NCOEF) or tdev.shape != (N, 5):
        raise ValueError(f"tilted_simulate: coef must be [N, {L.NCOEF}] and tinfo [N, 5], got {tuple(coef.shape)} and {tuple(tdev.shape)}")
    keep += [xin, coef, tdev]
    d = tilted_desc(net, device, keep)
    if d.d != dim:
        raise ValueError(f"tilted_simulate: x has {dim} features, the potential {d.d}")
    d.M, d.n_times, d.rows_per_time, d.tinfo = B, N, B, tdev.data_ptr()
    run = L.TiltedRds()
    run.form = L.FORM_LIN if form is None else int(form)
    run.flags = L.FLAG_ITO if flags is None else int(flags)
    run.N, run.coef = N, coef.data_ptr()
    run.net = net_desc(ctrl, device, keep)
    run.seed, run.particle0 = int(seed) & 0xFFFFFFFFFFFFFFFF, int(particle0)
    x_out = torch.empty_like(xin)
    rnd = torch.empty(B, 1, dtype=torch.float32, device=device)
    xs = torch.empty(N + 1, B, dim, dtype=torch.float32, device=device) if return_traj else None
    ref = torch.empty(N, B, dim, dtype=torch.float32, device=device) if want_ref else None
    nz = None
    if noise is not None:
        nz = noise.detach().to(device=device, dtype=torch.float32).contiguous()
        if nz.shape != (N, B, dim):
            raise ValueError(f"tilted_simulate: noise must be [N,B,d] = {(N, B, dim)}, got {tuple(nz.shape)}")
    run.x_in, run.noise_in, run.x_out, run.rnd_out = xin.data_ptr(), _ptr(nz), x_out.data_ptr(), rnd.data_ptr()
    run.xs_out, run.ref_out = _ptr(xs), _ptr(ref)
    _tilted_run(net, d, lib.sdeng_tilted_simulate_workspace_bytes(C.byref(d), C.byref(run)),
                lambda: lib.sdeng_tilted_simulate(C.byref(d), C.byref(run), _stream_ptr(device)), device)
    return x_out, rnd, xs, ref


def tilted_vjp(net, t, x: torch.Tensor, want_grad=False, per_row_times=False):
    """sdeng_tilted_vjp: one launch of the training instantiation of the tilted kernel at the rows (t, x).  Returns (log_prob [M],
    grad [M,d] or None, arrays, (N, B, t_unique [N])): the evaluation of ``tilted_eval`` (same bits) and the per-row arrays
    ``tilted_param_grads`` turns into the gradient of any function of the energies E_r = -log_prob_r with respect to the net's
    parameters -- ``arrays`` = {"a": [gelu(h_l)] * 5, "d": [f dh_l] * 5, "xs", "dv"} (include/sdeng.h; "a_all" / "d_all": the same
    memory as [5,M,128] blocks).  Pack cache and time handling
    are tilted_eval's; nothing here is recorded by autograd (``tilted_energy`` is the differentiable entry)."""
    with torch.no_grad():
        return _tilted_launch(net, t, x.detach(), want_grad, True, per_row_times, True)


def tilted_param_grads(net, arrays, cot, N, B, t_unique):
    """Per-row arrays of ``tilted_vjp`` and the cotangent ``cot`` [M] of the energies (dL/dE_r) -> {parameter: gradient} for the
    FourierMLP of a tilted potential (include/sdeng.h: sdeng_tilted_vjp).  Plain torch on whatever device and dtype the arrays have: the
    products are batched over the N times and summed, as in ``losses.training.vjp_param_grads``; the time embedding (2 layers on N rows)
    is differentiated by torch with the cotangent sum_b d[0]."""
    base = net.base_model
    c = cot.detach().reshape(-1, 1).to(arrays["xs"].dtype)
    # the five [M,128] arrays of a kind as one [5,M,128] block (tilted_vjp allocates them so: "a_all", "d_all"): one scaling, one column sum
    # and one batched product for the four hidden layers instead of one each -- at the trainer's shapes this part is bound by launches
    a = arrays["a_all"] if "a_all" in arrays else torch.stack(list(arrays["a"]))
    d = c * (arrays["d_all"] if "d_all" in arrays else torch.stack(list(arrays["d"])))
    dv, H = c * arrays["dv"], a.shape[-1]

    def outer(dl, act):
        return torch.bmm(dl.view(N, B, -1).transpose(1, 2), act.view(N, B, -1)).sum(0)
    db = d.sum(1)
    dw = torch.bmm(d[1:].reshape(4 * N, B, H).transpose(1, 2), a[:4].reshape(4 * N, B, H)).view(4, N, H, H).sum(1)
    grads = {base.out_layer.weight: outer(dv, a[4]), base.out_layer.bias: dv.sum(0),
             base.input_embed.weight: outer(d[0], arrays["xs"]), base.input_embed.bias: db[0]}
    for l, layer in enumerate(list(base.hidden_layer)[:4], start=1):
        grads[layer.weight], grads[layer.bias] = dw[l - 1], db[l]
    te_params = [p for p in base.timestep_embed.parameters() if p.requires_grad]
    if te_params:
        with torch.enable_grad():
            e = base.timestep_embed(t_unique.view(-1, 1).to(c.dtype))
            te_grads = torch.autograd.grad(e, te_params, grad_outputs=d[0].view(N, B, H).sum(1), allow_unused=True)
        grads.update({p: g for p, g in zip(te_params, te_grads) if g is not None})
    return grads


class _TiltedEnergy(torch.autograd.Function):
    """E = net.energy(t, x) with a first-order graph: forward is one tilted_vjp launch, backward the products of tilted_param_grads
    (and -grad_output * score for x).  The arrays stay on the context, so backward may run again (retain_graph, accumulation)."""

    @staticmethod
    def forward(ctx, net, t, x, *params):
        need_x = ctx.needs_input_grad[2]
        logp, score, arrays, layout = tilted_vjp(net, t, x, want_grad=need_x)
        ctx.net, ctx.arrays, ctx.layout, ctx.score, ctx.params = net, arrays, layout, score, params
        ctx.versions = [(p, p._version) for p in net.parameters()]
        return -logp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if any(p._version != v for p, v in ctx.versions):
            raise RuntimeError("tilted_energy: a parameter of the net was modified in place between the forward pass and backward "
                               "(the per-row arrays are those of the old parameters)")
        grads = tilted_param_grads(ctx.net, ctx.arrays, g, *ctx.layout) if any(ctx.needs_input_grad[3:]) else {}
        gx = -g.reshape(-1, 1) * ctx.score if ctx.needs_input_grad[2] else None
        return (None, None, gx) + tuple(grads.get(p) if need else None for p, need in zip(ctx.params, ctx.needs_input_grad[3:]))


def tilted_energy(net, t, x):
    """``net.energy(t, x)`` [M] carrying a graph to the net's trainable parameters and to ``x`` (first order), from one
    ``sdeng_tilted_vjp`` launch: what ``GMMTitledPotential`` returns with ``param_grads = True``."""
    params = [p for p in net.base_model.parameters() if p.requires_grad]
    return _TiltedEnergy.apply(net, t, x, *params)
