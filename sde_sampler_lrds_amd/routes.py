"""What the host knows about a distribution, a control, its target and a reference, and which training route follows from it -- said once, for
``engine.py``, ``losses/oc.py`` and ``losses/training.py``.  Objects are recognised by class name and plain attributes; nothing here copies a
tensor, reads one back or touches a device.  The C validators (``check_adjoint``, ``check_cmcd_adjoint``, ...) stay the authority at the ABI."""
from collections import namedtuple

from . import _lib as L


class UnsupportedByEngine(NotImplementedError):
    pass


def name_of(obj):
    return type(obj).__name__


def self_of(fn):
    return getattr(fn, "__self__", None)


def dist_kind(obj, score_only=False):
    """The ``L.DIST_*`` kind of a distribution object, None when no descriptor is built for it.  ``score_only``: the object is the target of a
    Score / Lerp / CancelDrift control and only its score is evaluated -- the one use a full-covariance mixture has a kernel for."""
    if obj is None:
        return L.DIST_NONE
    n = name_of(obj)
    if n in ("GMM", "TwoModes", "ManyModes", "BracketTwoModes", "Gauss", "Delta"):
        return L.DIST_GAUSS_DIAG if getattr(obj, "mixture_weights", None) is None else L.DIST_GMM_DIAG
    if n == "PhiFour":
        plain = getattr(obj, "dim_phys", 1) == 1 and tuple(getattr(obj, "bc", ("dirichlet", 0))) == ("dirichlet", 0) and not getattr(obj, "tilt", None)
        return L.DIST_PHI4 if plain else None
    if n == "Rings":
        return L.DIST_RINGS if obj.radiuses.shape[0] <= 8 else None
    if n in ("GMMFull", "TwoModesFull"):
        return L.DIST_GMM_FULL if score_only else None
    return {"IsotropicGauss": L.DIST_ISO_GAUSS, "GaussFull": L.DIST_GAUSS_FULL, "LogisticRegression": L.DIST_LOGREG, "SyntheticLogReg": L.DIST_LOGREG,
            "Checkerboard": L.DIST_CHECKERBOARD}.get(n)


TILTED_CLASSES = ("GMMTitledPotential", "GaussTiltedPotential")  # models/reparam.py:277-606, of this package or of the reference


def resolve_reference(reference_ctrl):
    """``reference_ctrl`` callable -> ('none'|'gaussian'|'gmm'|'nn', params).  Recognises the bound ``RDS.reference_ctrl`` (solver/oc.py:590-592 +
    ``reference_distr_utils``) and this package's ``MarginalReference`` objects."""
    if reference_ctrl is None:
        return "none", {}
    owner = self_of(reference_ctrl) or reference_ctrl
    utils = getattr(owner, "reference_distr_utils", None)
    if utils is None:
        raise UnsupportedByEngine("reference_ctrl is an opaque callable: pass RDS.reference_ctrl or a MarginalReference")
    if "means_init" in utils:
        return "gmm", utils  # diagonal [K,d], full [K,d,d] or the eigen form (D, P): ref_desc picks the kernel
    if "x_init" in utils:
        return "gaussian", utils  # diagonal [d], a covariance matrix [d,d] or its eigen form (D, P)
    if "net" in utils:
        if name_of(utils["net"]) in TILTED_CLASSES:
            return "nn", utils  # the step loop over an energy-based reference (sdeng_tilted_simulate); engine.tilted_refusal's findings are raised at the first launch
        raise UnsupportedByEngine(f"EBM ('nn') references on the HIP path are tilted potentials (GMMTitledPotential / GaussTiltedPotential): "
                                  f"{name_of(utils['net'])} needs autograd inside the step")
    raise UnsupportedByEngine("EBM ('nn') references need autograd inside the step: not on the HIP path")


def diagonal_reference(kind, utils) -> bool:
    """No reference drift, or a Gaussian / mixture reference with diagonal covariances (what sdeng_kl_adjoint differentiates in closed form)."""
    if kind == "none":
        return True
    if kind == "gaussian":
        v = utils["var_init"]
        return not isinstance(v, tuple) and v.dim() <= 1
    if kind == "gmm":
        v = utils["variances_init"]
        return not isinstance(v, tuple) and v.dim() == 2
    return False


CTRL_KINDS = {"ClippedCtrl": L.CTRL_CLIPPED, "ScoreCtrl": L.CTRL_SCORE, "LerpCtrl": L.CTRL_LERP, "CancelDriftCtrl": L.CTRL_CANCEL_DRIFT}
Ctrl = namedtuple("Ctrl", [
    "ctrl",            # the control module the kernels know: the EMA wrapper (AveragedModel) and RemoveReferenceCtrl peeled
    "wrapper",         # the RemoveReferenceCtrl that was peeled, or None
    "kind",            # L.CTRL_*, None for a module without a kernel
    "own_kind",        # ``kind`` where nothing was peeled, else None: what a test of the described object's own class name gives
    "score_model_ok",  # its score model is absent or a TimeEmbed
    "target",          # the distribution whose score a Score / Lerp / CancelDrift control mixes in (None: ClippedCtrl, or not a bound score)
    "target_kind",     # dist_kind(target, score_only=True); its score carries no graph where this is in GRAPHLESS_TARGETS
    "lerp_prior",      # the IsotropicGauss a LerpCtrl interpolates from (None: another control, or another prior)
])


def net_fault(net):
    """None when ``net`` is the drift net the kernels take, judged by structure (asked only when a kernel is), else ``net_desc``'s reason."""
    if name_of(net) != "FourierMLP" or net.channels != 64 or len(net.hidden_layer) != 2 or name_of(net.input_embed) != "Linear":
        return "drift net must be FourierMLP(num_layers=4, channels=64, use_angle_encoding=False)"
    if name_of(net.activation) != "GELU" or getattr(net.activation, "approximate", "none") != "none":
        return "activation must be exact-erf GELU"


def describe_ctrl(ctrl) -> Ctrl:
    """The record of a control.  Peels the EMA wrapper (``AveragedModel``, solver/oc.py:69-78) and ``RemoveReferenceCtrl`` (models/reparam.py:46-64:
    ``score(t, x) - ref_score(t, x)``, which the step loop applies as SDENG_FLAG_REMOVE_REF).  Never raises: ``engine.unwrap_ctrl`` / ``net_desc`` /
    ``ctrl_target`` turn what the record lacks into their exceptions."""
    given, wrapper = ctrl, None
    if name_of(ctrl) == "AveragedModel":
        ctrl = ctrl.module
    if name_of(ctrl) == "RemoveReferenceCtrl":
        wrapper, ctrl = ctrl, ctrl.score
        if name_of(ctrl) == "AveragedModel":
            ctrl = ctrl.module
    kind = CTRL_KINDS.get(name_of(ctrl))
    target = self_of(ctrl.target_score) if kind not in (None, L.CTRL_CLIPPED) else None
    prior = self_of(ctrl.prior_score) if kind == L.CTRL_LERP else None
    sm = getattr(ctrl, "score_model", None) if kind != L.CTRL_CLIPPED else None
    return Ctrl(ctrl, wrapper, kind, kind if ctrl is given else None, sm is None or name_of(sm) == "TimeEmbed", target,
                dist_kind(target, score_only=True), prior if name_of(prior) == "IsotropicGauss" else None)


# targets whose ``score`` is the base class's autograd evaluation WITHOUT a graph (distr/base.py:146-154): back-propagation through the
# trajectory sees it as a constant of x, in the reference and here -- and a hipGraph capture refuses the nested autograd call
GRAPHLESS_TARGETS = frozenset({L.DIST_LOGREG})
# log-variance, fused: ClippedCtrl, or a plain ScoreCtrl, whose score part (no state gradient to take in this pass) reaches only its score model,
# through sdeng_dist_eval -- which has every kind but the full-covariance mixture (that one exists as a score inside the step loop only)
LV_FUSED_TARGETS = frozenset(range(L.DIST_GMM_DIAG, L.DIST_CHECKERBOARD + 1)) - {L.DIST_GMM_FULL}
# KL, one launch: ClippedCtrl, or a Score / Lerp (from an IsotropicGauss, no hard_constrain) / CancelDrift control on a target whose score's
# Hessian-vector product sdeng_kl_adjoint has in closed form (BASELINE configs 1 and 3: DDS on TwoModes, PIS on PhiFour) or, the graph-less
# one, is zero (the score of every row comes from the HIP score kernel)
KL_NATIVE_TARGETS = frozenset({L.DIST_GMM_DIAG, L.DIST_PHI4, L.DIST_LOGREG})
# CMCD KL, one launch: ClippedCtrl, or a plain ScoreCtrl on the SDE's own target; the same targets plus the diagonal Gaussian, from an isotropic
# or diagonal Gaussian prior, d <= 128 (logistic regression: d <= 64, its step loop holds the design matrix in LDS); rings, checkerboard and
# full covariances keep the per-step adjoint
CMCD_NATIVE_TARGETS = KL_NATIVE_TARGETS | {L.DIST_GAUSS_DIAG}
CMCD_NATIVE_PRIORS = frozenset({L.DIST_ISO_GAUSS, L.DIST_GAUSS_DIAG})


def _own(ctrl, *kinds):
    """The record of ``ctrl`` when it is itself (a wrapped control is torch's, as a whole) one of ``kinds`` over the kernels' FourierMLP, else None."""
    rec = describe_ctrl(ctrl)
    return rec if rec.own_kind in kinds and net_fault(ctrl.base_model) is None else None


def lv_fused(ctrl) -> bool:
    """Is the batched log-variance pass of this control the fused HIP forward + backward, sdeng_ctrl_vjp (LV_FUSED_TARGETS)?"""
    rec = _own(ctrl, L.CTRL_CLIPPED, L.CTRL_SCORE)
    return rec is not None and (rec.kind == L.CTRL_CLIPPED or (rec.score_model_ok and rec.target_kind in LV_FUSED_TARGETS))


def kl_native(ctrl) -> bool:
    """Does sdeng_kl_adjoint differentiate this control (KL_NATIVE_TARGETS)?"""
    rec = _own(ctrl, *CTRL_KINDS.values())
    if rec is None or rec.kind == L.CTRL_CLIPPED:
        return rec is not None
    if rec.kind == L.CTRL_LERP and (rec.lerp_prior is None or getattr(ctrl, "hard_constrain", False)):
        return False
    return rec.target_kind in KL_NATIVE_TARGETS and rec.score_model_ok


def cmcd_native(loss) -> bool:
    """Does sdeng_cmcd_kl_adjoint differentiate this ControlledLangevinSDELoss (CMCD_NATIVE_TARGETS)?"""
    rec = _own(loss.generative_ctrl, L.CTRL_CLIPPED, L.CTRL_SCORE)
    target, prior = self_of(getattr(loss.sde, "target_score", None)), self_of(getattr(loss.sde, "prior_score", None))
    if rec is None or not getattr(loss, "use_rescaling", True) or dist_kind(prior) not in CMCD_NATIVE_PRIORS or dist_kind(target) not in CMCD_NATIVE_TARGETS:
        return False
    if not 1 <= int(getattr(target, "dim", 0) or 0) <= (64 if dist_kind(target) == L.DIST_LOGREG else 128):
        return False
    return rec.kind == L.CTRL_CLIPPED or (rec.target is target and rec.score_model_ok)


def lv_route(loss):
    """('fused' | 'graphed' | 'eager', control): the batched control pass of a log-variance training call (BaseOCLoss._integral_pass) and the control it
    differentiates -- the loss's own, or the score of its RemoveReferenceCtrl (u = inner - ref_score and ref_score has no parameters, so s -
    s.detach() of the inner control carries the same (zero) value and the same gradient).  A captured graph only for the pure-torch control, a
    ClippedCtrl over any FourierMLP; ControlledLangevinSDELoss builds its cost from an eager pass of its own (two evaluations share a state)."""
    rec = describe_ctrl(loss.generative_ctrl)
    ctrl = rec.ctrl if rec.wrapper is loss.generative_ctrl else loss.generative_ctrl
    if getattr(loss, "kind", None) == "cmcd":
        return "eager", ctrl
    if loss.fused_training and lv_fused(ctrl):
        return "fused", ctrl
    plain = describe_ctrl(ctrl).own_kind == L.CTRL_CLIPPED and name_of(ctrl.base_model) == "FourierMLP"
    return ("graphed" if loss.graph_training and plain else "eager"), ctrl


KL_OVER_NN = "KL training differentiates the reference score: second order in the energy net"


def kl_route(loss, reference_ctrl=None) -> str:
    """'native' | 'fused' | 'stepwise': the adjoint of a KL training call (BaseOCLoss._kl_loss) whose reference drift is ``reference_ctrl`` (resolved
    first: an opaque callable raises whatever the route)."""
    ref = resolve_reference(reference_ctrl)
    if ref[0] == "nn":
        raise UnsupportedByEngine(KL_OVER_NN)
    if diagonal_reference(*ref) and loss.native_adjoint and kl_native(loss.generative_ctrl):
        return "native"
    return "fused" if loss.fused_training and _own(loss.generative_ctrl, L.CTRL_CLIPPED) else "stepwise"


def cmcd_kl_route(loss) -> str:
    """'native' | 'stepwise': the adjoint of CMCD's KL training call (ControlledLangevinSDELoss._kl_loss_cmcd)."""
    return "native" if loss.native_adjoint and cmcd_native(loss) else "stepwise"


def graph_capturable(ctrl, *score_fns) -> bool:
    """Can one stepwise adjoint step of this control be captured as a hipGraph?  Not with a GRAPHLESS_TARGETS score in it: one of ``score_fns``, or
    the target of the control (of the four kinds) or of the score of a RemoveReferenceCtrl itself; an EMA copy is not looked into: capture is tried."""
    inner = ctrl.score if name_of(ctrl) == "RemoveReferenceCtrl" else ctrl
    rec = describe_ctrl(inner)
    return not any(dist_kind(t) in GRAPHLESS_TARGETS for t in [rec.target if rec.own_kind is not None else None] + [self_of(f) for f in score_fns])
