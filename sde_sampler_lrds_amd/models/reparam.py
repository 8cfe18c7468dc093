"""Control wrappers (mirror of ``sde_sampler/models/reparam.py``: ClippedCtrl :18-43, RemoveReferenceCtrl :46-64, ScoreCtrl :67-117, CancelDriftCtrl :120-145,
LerpCtrl :148-199) and the energy-based references GMMTitledPotential :277-482, GaussTiltedPotential :485-606 (one
``sdeng_tilted_eval`` launch per evaluation).  See models/mlp.py for how the controls relate to the HIP path."""
from __future__ import annotations

from typing import Callable

import torch
from torch.nn import Module


def _clip(v, m):
    return v if m is None else v.clip(min=-1.0 * m, max=m)


class ClippedCtrl(Module):
    def __init__(self, base_model: Module, clip_model: float | None = None, name: str = "ctrl", **kwargs):
        super().__init__()
        self.base_model, self.clip_model, self.name = base_model, clip_model, name

    def clipped_base_model(self, t, x):
        return _clip(self.base_model(t, x), self.clip_model)

    def forward(self, t, x):
        return self.clipped_base_model(t, x)


class RemoveReferenceCtrl(Module):
    """models/reparam.py:46-64: ``score(t, x) - ref_score(t, x)`` (``use_rescaling=False``) or ``- sde.diff(t, x) * ref_score(t, x)``
    (``use_rescaling=True``; upstream's constructor then forbids passing the ``sde`` its forward needs, so that branch raises
    AttributeError when called -- kept).  "Only used for Langevin init", i.e. around a CancelDriftCtrl.  The step-loop kernel runs the
    ``use_rescaling=False`` form as a control modifier (SDENG_FLAG_REMOVE_REF: u -= reference score, which the tail already holds)."""

    def __init__(self, score, ref_score, use_rescaling=True, sde=None):
        super().__init__()
        assert not (use_rescaling and (sde is not None))
        self.score, self.ref_score, self.use_rescaling, self.sde = score, ref_score, use_rescaling, sde

    def forward(self, t, x):
        ret = self.score(t, x)
        if self.use_rescaling:
            ret -= self.sde.diff(t, x) * self.ref_score(t, x)
        else:
            ret -= self.ref_score(t, x)
        return ret


class ScoreCtrl(ClippedCtrl):
    """base_model(t,x) + scale * clip(target_score(x)) * clip(score_model(t))."""

    def __init__(self, *args, target_score: Callable, score_model: Module | None = None, detach_score: bool = True,
                 scale_score: float = 1.0, clip_score: float | None = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.score_model, self.target_score = score_model, target_score
        self.detach_score, self.scale_score, self.clip_score = detach_score, scale_score, clip_score

    def clipped_target_score(self, t, x):
        x = x.detach() if self.detach_score else x
        return _clip(self.target_score(x, create_graph=self.detach_score), self.clip_score)

    def clipped_score_model(self, t, x):
        return _clip(self.score_model(t, x), self.clip_model)

    def forward(self, t, x):
        score = self.scale_score * self.clipped_target_score(t, x)
        if self.score_model is not None:
            score = score * self.clipped_score_model(t, x)
        return self.clipped_base_model(t, x) + score


class LerpCtrl(ScoreCtrl):
    """base_model + g(t) * scale * clip(lerp(prior_score, target_score, t/T)) * clip(score_model(t))."""

    def __init__(self, *args, sde, prior_score: Callable, hard_constrain: bool = False, scale_lerp: float = 1.0, **kwargs):
        super().__init__(*args, **kwargs)
        if hard_constrain:
            raise NotImplementedError("hard_constrain is not part of the engine (conf/model/lerp.yaml leaves it off)")
        self.sde, self.prior_score, self.hard_constrain, self.scale_lerp = sde, prior_score, hard_constrain, scale_lerp

    def clipped_interpolated_score(self, t, x):
        x = x.detach() if self.detach_score else x
        mix = torch.lerp(self.prior_score(x), self.target_score(x, create_graph=self.detach_score), t / self.sde.terminal_t)
        return _clip(mix, self.clip_score)

    def forward(self, t, x):
        score = self.scale_score * self.clipped_interpolated_score(t, x)
        if self.score_model is not None:
            score = score * self.clipped_score_model(t, x)
        return self.clipped_base_model(t, x) + self.sde.diff(t, x) * score


class CancelDriftCtrl(ScoreCtrl):
    """Langevin initialisation (models/reparam.py:120-145): a ScoreCtrl that also subtracts the denoising SDE's drift,
    base_model + drift(t,x)/g(t) + g(t)/2 * scale * clip(target_score) * clip(score_model(t))  (``use_rescaling``; otherwise
    drift/g^2 + score/2)."""

    def __init__(self, *args, sde, langevin_init: bool = True, use_rescaling: bool = True, **kwargs):
        super().__init__(*args, **kwargs)
        if sde is None or getattr(sde, "noise_type", None) not in ("diagonal", "scalar"):  # reparam.py:125-126 (DDS has no SDE)
            raise ValueError(f"Invalid sde for CancelDriftCtrl: {sde!r}")
        self.sde, self.langevin_init, self.use_rescaling = sde, langevin_init, use_rescaling

    def forward(self, t, x):
        ctrl = self.clipped_base_model(t, x)
        g, f = self.sde.diff(t, x), self.sde.drift(t, x)
        score = self.scale_score * self.clipped_target_score(t, x)
        if self.score_model is not None:
            score = score * self.clipped_score_model(t, x)
        if self.use_rescaling:
            return ctrl + (f / g) + 0.5 * g * score
        return ctrl + (f / torch.square(g)) + 0.5 * score


class GMMTitledPotential(Module):
    """Energy-based reference as a tilted potential (mirror of models/reparam.py:277-482, the reference's spelling of the name kept):
    E(t, x) = -log GMM_t(x) + f(t) <NN(t, xs), xs> with the Gaussian mixture noised by the SDE to max(t, t_limit) as the prior and xs the
    Karras-style scaled state.  Same constructor, buffers and parameter names as the reference, so its ``state_dict`` loads.

    Every evaluation -- ``unnorm_log_prob``, ``unnorm_log_prob_and_grad``, ``energy``, ``forward`` (the score) -- is ONE
    ``engine.tilted_eval`` launch on the GPU; nothing is differentiated by autograd, so the results carry no graph.  A call that would
    need gradients with respect to the net's parameters (grad mode with parameters that require grad) raises ``UnsupportedByEngine``:
    there is no torch fallback.  ``scaling_factor`` (DRL) is not supported.

    ``param_grads = True`` (off by default; ``MaximumLikelihoodEBM.train`` switches it on for its duration) lets ``energy`` and
    ``unnorm_log_prob`` carry a first-order graph in grad mode -- to the net's trainable parameters and to ``x`` -- from one
    ``engine.tilted_vjp`` launch (``engine.tilted_energy``).  ``unnorm_log_prob_and_grad`` and ``forward`` keep raising with trainable
    parameters: differentiating the score is second order."""

    param_grads = False

    def __init__(self, base_model, sde, weights, means, variances, t_limit=0.0, use_s_t_scaling=False, tilt_type="dot",
                 use_scaling_factor=False):
        super().__init__()
        from ..distr.gauss import GMM, GMMFull
        self.tilt_type, self.base_model, self.use_s_t_scaling, self.sde = tilt_type, base_model, use_s_t_scaling, sde
        self.dim, self.t_limit = means.shape[-1], t_limit
        self.is_full_gmm_type = isinstance(variances, tuple) or (len(variances.shape) == 3)
        self.register_buffer("weights", weights)
        self.register_buffer("means", means)
        self.use_full_decomp = isinstance(variances, tuple)
        if self.use_full_decomp:
            self.register_buffer("cov_D", variances[0])
            self.register_buffer("cov_P", variances[1])
            self.register_buffer("variances", torch.einsum("...ik,...k,...jk->...ij", self.cov_P, self.cov_D, self.cov_P))
        else:
            self.register_buffer("variances", variances)
        if self.is_full_gmm_type:
            self.prior_final = GMMFull(dim=self.dim, loc=self.means, cov=self.variances, mixture_weights=self.weights)
            comp = torch.distributions.MultivariateNormal(self.means, covariance_matrix=self.variances)
        else:
            self.prior_final = GMM(dim=self.dim, loc=self.means, scale=self.variances.sqrt(), mixture_weights=self.weights)
            comp = torch.distributions.Independent(torch.distributions.Normal(self.means, self.variances.sqrt()), 1)
        mix = torch.distributions.MixtureSameFamily(torch.distributions.Categorical(self.weights / self.weights.sum()), comp)
        self.register_buffer("mean_gauss", mix.mean)       # the Gaussian approximation of the prior (reparam.py:334-335)
        self.register_buffer("var_gauss", mix.variance)
        self.use_scaling_factor = use_scaling_factor
        self.has_unnorm_log_prob_and_grad = True
        self.has_sample_prior = True

    # ---- prior ----
    def _clamped(self, t):
        return torch.maximum(t, self.t_limit * torch.ones_like(t))

    def get_gmm_params(self, t, scaling_factor=1.0):
        """(weights, means, variances) of the mixture noised to max(t, t_limit) (reparam.py:354-365, eq/sdes.py:281-307); for the eigen
        form the variances are the tuple (precisions, log-determinants)."""
        var = (scaling_factor ** 2 * self.cov_D, self.cov_P) if self.use_full_decomp else scaling_factor ** 2 * self.variances
        means, variances = self.sde.marginal_params(self._clamped(t), scaling_factor * self.means, var_init=var, is_mixture=True)
        return self.weights, means, variances

    def sample_prior(self, ts):
        """Samples of the noised prior at the times ``ts`` (reparam.py:367-374)."""
        x0 = self.prior_final.sample((ts.shape[0],))
        loc, var = self.sde.marginal_params(self._clamped(ts).view((-1, 1)), x0)
        return loc + torch.sqrt(var) * torch.randn_like(loc)

    # ---- evaluations: one launch each ----
    def _eval(self, t, x, scaling_factor, want_grad):
        from .. import engine as E
        if self.use_scaling_factor or not (isinstance(scaling_factor, (int, float)) and float(scaling_factor) == 1.0):
            raise E.UnsupportedByEngine("tilted potentials: scaling_factor / use_scaling_factor (DRL) is not on the HIP path")
        return E.tilted_eval(self, t, x, want_grad=want_grad)

    def _with_graph(self, x):
        from .. import engine as E
        return self.param_grads and torch.is_grad_enabled() and (E.tilted_needs_param_grad(self) or (torch.is_tensor(x) and x.requires_grad))

    def unnorm_log_prob(self, t, x, scaling_factor=1.0):
        if self._with_graph(x):
            return -self.energy(t, x, scaling_factor=scaling_factor)
        return self._eval(t, x, scaling_factor, False)[0]

    def energy(self, t, x, scaling_factor=1.0):
        if self._with_graph(x):
            from .. import engine as E
            if self.use_scaling_factor or not (isinstance(scaling_factor, (int, float)) and float(scaling_factor) == 1.0):
                raise E.UnsupportedByEngine("tilted potentials: scaling_factor / use_scaling_factor (DRL) is not on the HIP path")
            return E.tilted_energy(self, t, x)
        return -self.unnorm_log_prob(t, x, scaling_factor=scaling_factor)

    def unnorm_log_prob_and_grad(self, t, x, scaling_factor=1.0, retain_graph=False):
        return self._eval(t, x, scaling_factor, True)

    def forward(self, t, x, scaling_factor=1.0):
        """The score of the model (reparam.py:478-482)."""
        return self._eval(t, x, scaling_factor, True)[1]


class GaussTiltedPotential(GMMTitledPotential):
    """The single-Gaussian case (mirror of models/reparam.py:485-606): buffers ``mean``, ``variance`` ([d], [d,d] or the (D, P) tuple)."""

    def __init__(self, base_model, sde, mean, variance, t_limit=0.0, tilt_type="dot", use_s_t_scaling=False, use_scaling_factor=False):
        Module.__init__(self)
        from ..distr.gauss import Gauss, GaussFull
        self.tilt_type, self.base_model, self.use_s_t_scaling, self.sde = tilt_type, base_model, use_s_t_scaling, sde
        self.dim, self.t_limit = mean.shape[-1], t_limit
        self.is_full_cov_type = isinstance(variance, tuple) or (len(variance.shape) == 2)
        self.register_buffer("mean", mean)
        self.register_buffer("mean_gauss", mean)
        self.use_full_decomp = isinstance(variance, tuple)
        if self.use_full_decomp:
            self.register_buffer("cov_D", variance[0])
            self.register_buffer("cov_P", variance[1])
            self.register_buffer("variance", torch.einsum("...ik,...k,...jk->...ij", self.cov_P, self.cov_D, self.cov_P))
        else:
            self.register_buffer("variance", variance)
        if self.is_full_cov_type:
            self.prior_final = GaussFull(dim=self.dim, loc=self.mean, cov=self.variance)
            self.register_buffer("var_gauss", torch.diagonal(self.variance).clone())
        else:
            self.prior_final = Gauss(dim=self.dim, loc=self.mean, scale=self.variance.sqrt())
            self.register_buffer("var_gauss", self.variance.clone())
        self.use_scaling_factor = use_scaling_factor
        self.has_unnorm_log_prob_and_grad = True
        self.has_sample_prior = True

    def get_gauss_params(self, t, scaling_factor=1.0):
        var = (scaling_factor ** 2 * self.cov_D, self.cov_P) if self.use_full_decomp else scaling_factor ** 2 * self.variance
        return self.sde.marginal_params(self._clamped(t), scaling_factor * self.mean, var_init=var)

    def get_gmm_params(self, t, scaling_factor=1.0):
        mean, var = self.get_gauss_params(t, scaling_factor)
        var = tuple(v.unsqueeze(0) for v in var) if isinstance(var, tuple) else var.unsqueeze(0)
        return torch.ones(1, device=mean.device), mean.unsqueeze(0), var
