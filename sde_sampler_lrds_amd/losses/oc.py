"""Drop-in loss classes for the reference's ``sde_sampler/losses/oc.py`` (``conf/loss/*.yaml:_target_``).

Same class names, constructor arguments, ``simulate`` / ``eval`` / ``state_dict`` surface and return types as
the reference (``BaseOCLoss`` :14-200 and its seven subclasses), but ``simulate`` is ONE call into the HIP
engine (csrc/) instead of a Python step loop: every step's drift-net forward, scores, noise, integrator
update and log-RND accumulation run inside a single persistent gfx950 kernel.

What is on the HIP path: the eval / sampling direction (``change_sde_ctrl=False``), i.e. what
``Trainable.evaluate`` times as ``eval/sample_time`` (solver/oc.py:148-158); ``x`` may be an ``engine.InitialDraw`` (x0 drawn by the
kernel) and ``loss.dist`` a torch.distributed module (sharded run: global estimators and weights).  ``compute_eubo`` (the noising loops of
SURVEY.md 8f-2) is a HIP launch too (RDS losses, DiscreteTimeReversalLossEI, CMCD on mixture targets).  The training direction (``__call__``,
8f-1): the HIP step loop for the value; the gradient from one batched pass of the control for the log-variance methods (``_lv_loss``) and
from the discrete adjoint of the step loop for the KL methods (``_kl_loss``, ``_kl_loss_cmcd``).  What those calls share -- the rollout, the KL
weights, the parameter gradients from a kernel's per-row arrays, the hand-off to autograd, the adjoints themselves -- is ``losses/training.py``.

Each class states its step loop ONCE, in ``_step_loop`` (-> ``StepLoop``: form, flags, table options, reference, whether the initial log-density
enters and the EMA control is honoured); ``simulate``, ``eval``, ``compute_eubo`` and the training call hand that declaration to ``_launch``, which
takes seed and control perturbation as arguments and returns, next to (x_N, rnd, xs), the record of what it ran (``engine.Launched``: declaration,
device table, compiled net / reference / lerp prior).  The gradient code reads lin, ito, table and reference from that record: it differentiates
the recursion the kernel integrated.  (The parts are compiled before the launch's own checks, so where several refusals apply to one call the
table's or the control's may now come before the RemoveReferenceCtrl / terminal / initial-density ones; each refusal is unchanged.)

Extra, engine-only knobs (keyword-only, default to the reference behaviour):
  * ``noise=[N,B,d]`` injects the normals (replays the reference's ``randn_like`` stream, parity mode);
    without it the kernel draws counter-based Philox normals keyed by ``self.seed`` and the global
    particle index ``self.particle0 + row`` (independent of how the batch is sharded over GPUs);
  * ``call`` (``simulate`` only; INTERNAL to the training calls, ``training.launch_call``): a training call's seed and perturbation in, the
    launch's record out (``call.ran``) -- arguments of that one call, where the loss object used to be written to.  Leave it unset.
"""
from __future__ import annotations

import logging
from typing import Callable, NamedTuple

import torch

from .. import _lib as L
from .. import engine as E
from .. import parallel
from .. import routes as R
from ..utils.common import Results, make_results
from . import training as T
from .training import _capturable, _FusedIntegral, _GraphedAdjointStep, _graphed_step, _IntegralPass, ctrl_batched, fused_net_view, fused_training_ok, vjp_param_grads  # noqa: F401  (all stay reachable here)


class StepLoop(NamedTuple):
    """A loss class's declaration of its step loop for one direction (``_step_loop``); the gradient code reads it back from ``engine.Launched.decl``."""
    form: int                   # L.FORM_*
    flags: int                  # L.FLAG_ITO, or 0 (CMCD: its three flags)
    coef_kw: dict               # table kind (default: the class's ``kind``) and options of ``_coef``
    ref: tuple = ("none", {})   # the resolved reference drift
    ref_ctrl: object = None     # the same as the callable the torch adjoints differentiate (None without a reference drift)
    init: bool = True           # does the initial log-density enter (dropped for KL training in the DIS family)
    ema: bool = True            # is ``use_ema`` honoured
    lin = property(lambda self: self.form == L.FORM_LIN)
    ito = property(lambda self: bool(self.flags & L.FLAG_ITO))


class BaseOCLoss:
    """Mirror of losses/oc.py:14-200."""

    kind = None  # coefficient-table kind of the subclass
    optional_ito = False  # does simulate() take ``compute_ito_int`` (eval() then asks for the Ito integral only with the weights)

    def __init__(self, generative_ctrl: Callable, generative_ctrl_ema: Callable, sde=None, method: str = "kl",
                 traj_per_sample: int = 1, filter_samples: Callable | None = None, max_rnd: float | None = None,
                 sde_ctrl_dropout: float | None = None, sde_ctrl_noise: float | None = None, **kwargs):
        self.generative_ctrl = generative_ctrl
        self.generative_ctrl_ema = generative_ctrl_ema
        self.sde = sde
        if method not in ["kl", "kl_ito", "lv", "lv_traj"]:
            raise ValueError("Unknown loss method.")
        self.method = method
        if traj_per_sample == 1 and self.method == "lv_traj":
            raise ValueError("Cannot compute variance over a single trajectory.")
        self.traj_per_sample = traj_per_sample
        self.filter_samples = filter_samples
        self.max_rnd = max_rnd
        self.sde_ctrl_noise = sde_ctrl_noise
        self.sde_ctrl_dropout = sde_ctrl_dropout
        if self.method in ["kl", "kl_ito"]:
            for attr in ["sde_ctrl_noise", "sde_ctrl_dropout"]:
                if getattr(self, attr) is not None:
                    logging.warning("%s should only be used for the log-variance loss.", attr)
        self.n_filtered = 0
        # engine state
        self.seed = 1
        self.particle0 = 0
        self.train_calls = 0
        self._coef_cache = {}
        self._cpu_sde = None
        self.timing_events = None  # optional _lib.HipEvents: times the step-loop kernel alone
        self.graph_adjoint = True  # KL training where the adjoint runs step by step in torch (CMCD; controls / targets / references the adjoint kernel does not cover): each step replayed as a hipGraph; False: eager
        self.native_adjoint = True  # KL training of a ClippedCtrl with no / a diagonal reference: the adjoint recursion as ONE launch (sdeng_kl_adjoint; CMCD: sdeng_cmcd_kl_adjoint); False: one sdeng_ctrl_vjp per step (CMCD: one torch VJP per step)
        self.last_adjoint_path = None  # KL training, which adjoint the last call ran: 'native' (one launch) | 'fused' (sdeng_ctrl_vjp per step; not CMCD) | 'stepwise' (torch VJP per step)
        self.fused_training = True  # ClippedCtrl over a FourierMLP: the batched control pass of training as ONE fused HIP forward + backward (sdeng_ctrl_vjp); False: the eager torch pass
        self.graph_training = False  # True: the batched control pass of log-variance training (forward + backward) is replayed as a hipGraph (_IntegralPass)
        self._graphed = {}
        self.split_tiles = False  # True: small batches (<= _lib.SPLIT_TILES_MAX_B = 8 192, the library's own gate) ask for the low-latency kernels (SDENG_FLAG_SPLIT_TILES; fp32-round-off, not bit, equal to the standard kernel); the solvers switch it on (cfg 'split_tiles', default True)
        self.dist = None  # torch.distributed of a sharded run: eval() then returns global estimators and globally normalised weights
        self._nn_times = None  # an energy-based ('nn') reference: (coefficient table, net, its time table [N, 5] on the device) of the last grid

    # ---- reference surface -----------------------------------------------------------------
    def filter(self, rnd, samples=None):
        mask = True
        if samples is not None and self.filter_samples is not None:
            mask = self.filter_samples(samples)
        if self.max_rnd is None:
            return mask & rnd.isfinite()
        return mask & (rnd < self.max_rnd)

    def compute_loss(self, rnd, samples=None):
        mask = self.filter(rnd, samples=samples)
        assert mask.shape == rnd.shape
        if parallel.is_sharded(self.dist):
            return self._compute_loss_global(rnd, mask)
        if self.method == "lv_traj":
            rnd = rnd.reshape(self.traj_per_sample, -1, 1)
            mask = mask.reshape(self.traj_per_sample, -1, 1).all(dim=0)
            self.n_filtered += self.traj_per_sample * (mask.numel() - mask.sum()).item()
            loss = rnd[:, mask].var(dim=0).mean()
        else:
            self.n_filtered += (mask.numel() - mask.sum()).item()
            loss = rnd[mask].var() if self.method == "lv" else rnd[mask].mean()
        return loss, {"train/n_filtered_cumulative": self.n_filtered}

    def _compute_loss_global(self, rnd, mask):
        """``compute_loss`` of a sharded run (``self.dist``: a process group of more than one rank): ``rnd`` is this rank's shard, the value
        the objective over ALL ranks' particles -- the same bits on every rank -- from ONE 32-byte all-gather (``parallel.global_moments``:
        per-shard (n, mean, M2) in float64 on the device, combined with Chan's update).  It enters autograd as value.detach() + (local -
        local.detach()), ``local`` being this shard's terms of the global expression with the global mean and count as constants: each
        rank's gradient is its exact partial sum of the global one (for 'lv' because sum_i (rnd_i - mean) = 0 over the global batch), so
        ``parallel.all_reduce_grads`` with SUM completes it.  'lv_traj': the variance over a sample's trajectories stays local (they live on
        one rank), the mean runs over the global count of kept samples.  An empty shard is legal; n <= 1 gives NaN, as ``torch.var`` does."""
        tps = 1
        if self.method == "lv_traj":
            tps = self.traj_per_sample
            rnd = rnd.reshape(tps, -1, 1)
            mask = mask.reshape(tps, -1, 1).all(dim=0)
            kept = rnd[:, mask].double().var(dim=0)  # [kept samples of this shard]
            with torch.no_grad():
                per_sample = torch.zeros(mask.shape, dtype=torch.float64, device=rnd.device)
                per_sample[mask] = kept
            mom = parallel.global_moments(per_sample, mask, self.dist)
            value, local = parallel.kept_mean(mom), kept.sum() / mom[parallel.M_N]
        else:
            mom = parallel.global_moments(rnd, mask, self.dist)
            if self.method == "lv":
                value = parallel.unbiased_var(mom)
                local = ((rnd[mask].double() - mom[parallel.M_MEAN]) ** 2).sum() / (mom[parallel.M_N] - 1)
            else:
                value, local = parallel.kept_mean(mom), rnd[mask].double().sum() / mom[parallel.M_N]
        self.n_filtered += tps * int(mom[parallel.M_ROWS] - mom[parallel.M_N])
        loss = (value.detach() + (local - local.detach())).to(rnd.dtype)
        return loss, {"train/n_filtered_cumulative": self.n_filtered}

    @staticmethod
    def compute_results(rnd, compute_weights=False, ts=None, samples=None, xs=None, dist=None) -> Results:
        """losses/oc.py:134-173 on the device: one sdeng_logz call gives elbo, logsumexp, variance, weights.
        ``dist`` (an initialised torch.distributed module, set as ``loss.dist`` by a sharded caller): ``rnd`` is this rank's shard;
        the estimators and the importance weights are then those of ALL ranks' particles (one 36-byte all-gather,
        ``parallel.global_weights``), so ``Results.weights`` concatenated over the ranks is the reference's ``softmax(-rnd, 0)``."""
        if dist is not None and dist.is_initialized() and dist.get_world_size() > 1:
            from .. import parallel
            if compute_weights:
                w, res = parallel.global_weights(rnd, dist)
            else:
                w, res = None, parallel.global_results(rnd, dist)
            metrics = {"eval/elbo": res["elbo"], "eval/n_particles": res["n"]}  # (the count over all ranks: what the estimators are over)
            preds = {}
            if compute_weights:
                preds["log_norm_const_is"] = res["log_norm_const_is"]
                metrics["eval/lv_loss"] = res["lv_loss"]
                metrics["eval/norm_effective_sample_size"] = res["ess"]
            return make_results(samples=samples, weights=w, log_norm_const_preds=preds, ts=ts, xs=xs, metrics=metrics)
        stats, w = E.logz_stats(rnd, want_weights=compute_weights)
        host = stats.cpu()
        metrics = {"eval/elbo": host[0].item()}
        preds = {}
        if compute_weights:
            preds["log_norm_const_is"] = host[1].item()
            metrics["eval/lv_loss"] = host[2].item()
            metrics["eval/norm_effective_sample_size"] = host[3].item()  # eval/metrics.py:135-140
        return make_results(samples=samples, weights=w, log_norm_const_preds=preds, ts=ts, xs=xs, metrics=metrics)

    def eval(self, ts, x, terminal_unnorm_log_prob, reference_log_prob=None, compute_weights=True, return_traj=True,
             use_ema=True, *, noise=None) -> Results:
        """eval() of the losses that end in ``reference_log_prob`` (the DIS / CMCD families start from ``initial_log_prob``: _InitialLogProbLoss)."""
        kw = dict(compute_ito_int=compute_weights) if self.optional_ito else {}
        samples, rnd, xs = self.simulate(ts, x, terminal_unnorm_log_prob=terminal_unnorm_log_prob, reference_log_prob=reference_log_prob,
                                         change_sde_ctrl=False, return_traj=return_traj, use_ema=use_ema, noise=noise, **kw)
        return BaseOCLoss.compute_results(rnd, compute_weights=compute_weights, ts=ts, samples=samples, xs=xs, dist=self.dist)

    def __call__(self, ts, x, *args, **kwargs):
        raise E.UnsupportedByEngine(
            f"{type(self).__name__} has no training call: the subclasses implement loss(ts, x, ...) for the log-variance methods "
            "(BaseOCLoss._lv_loss: HIP step loop + one batched autograd pass, SURVEY.md 8f-1)")

    def load_state_dict(self, state_dict: dict):
        self.n_filtered = state_dict["n_filtered"]

    def state_dict(self) -> dict:
        return {"n_filtered": self.n_filtered}

    def _train(self, ts, x, terminal_unnorm_log_prob, sim_kw, rnd0=None):
        """The training call of the FORM_LIN / FORM_EM losses: the step loop is ``simulate(**sim_kw)`` with the trajectory kept, handed the call's
        seed and perturbation by ``training.rollout`` (``call``).  It never adds the initial log-density: log-variance training adds ``rnd0``."""
        reference_log_prob = sim_kw.get("reference_log_prob")

        def launch(xx, call):
            return self.simulate(ts, xx, terminal_unnorm_log_prob, return_traj=True, call=call, **sim_kw)
        if self.method not in ("kl", "kl_ito"):
            return self._lv_loss(ts, x, launch, rnd0=rnd0)
        if reference_log_prob is None:
            return self._kl_loss(ts, x, launch, lambda xn: -terminal_unnorm_log_prob(xn).view(-1, 1))
        return self._kl_loss(ts, x, launch, lambda xn: reference_log_prob(xn).view(-1, 1) - terminal_unnorm_log_prob(xn).view(-1, 1))

    def _lv_loss(self, ts, x, launch, *, rnd0=None):
        """Log-variance training value (losses/oc.py ``__call__`` of every loss, method in ('lv', 'lv_traj')).  The
        trajectories are driven by the DETACHED control (generative_and_sde_ctrl, :83-103), so the states carry no graph
        and the step loop is exactly the eval path: it runs as one HIP launch (``launch(x)`` with the trajectory kept) and its log-weights ARE the loss's
            rnd = rnd0 + sum_k c_k <u_k, u_k.detach() - u_k/2> + c'_k <u_k, z_k> + terminal(x_N);
        their gradient comes from ONE batched pass of the control over all N*B (time, state) pairs
        (:269-271, :284 EM; :490-491, :499 EI / DDPM-like; :957-958, :965 DIS; :1361-1383 DDS).  KL training differentiates
        through the trajectory and is not on this path."""
        assert self.method in ("lv", "lv_traj")
        # sde_ctrl_noise / sde_ctrl_dropout (generative_and_sde_ctrl, :97-102): the step loop perturbs the control it integrates with --
        # the perturbed control then IS the control of every term of the value (the reference writes it in place through the detached
        # alias), while the gradient below is unchanged: c'_k z_k back through the net, along the perturbed trajectory
        # VALUE: the step loop already integrates exactly this rnd (the detached control is the control), terminal terms included.  (the kernel draws the normals
        # of stream seed_c itself -- bit for bit the z below -- so small batches may take the low-latency split-tile kernel, which does not replay noise)
        x, x_n, rnd_sim, xs, ran, seed_c, N, B, d = T.rollout(self, ts, x, launch, perturb=self._ctrl_perturbation())
        z = E.philox_noise(seed_c, N, B, d, self.particle0, x.device)
        with torch.no_grad():
            rnd_val = rnd_sim.reshape(B, 1)
            if rnd0 is not None:
                rnd_val = rnd_val + self._logp(rnd0, x)
        # GRADIENT: d rnd_b / d u_kb = c_k (u.detach() - u) + c'_k z_kb = c'_k z_kb -- the running-cost term has zero gradient at
        # u.detach() = u (in fp32 too: (u - u/2) - u/2 = 0 exactly, which is what the reference's autograd produces).  So the only
        # part of rnd that needs a graph is the stochastic integral s_b = sum_k c'_k <u_kb, z_kb>, from one batched pass of the
        # control; it enters with value zero (s - s.detach()), and compute_loss / backward() do the rest as upstream.
        coef = ran.coef  # coef[:, 0]: the net's time of step k, coef[:, 5]: c'_k (the table the step loop ran on)
        zc = (z.view(N, B, d) * coef[:, 5].view(N, 1, 1)).view(N * B, d)
        s = self._integral_pass(coef[:, 0].contiguous(), xs[:-1], zc)
        return self.compute_loss(rnd_val + (s - s.detach()).view(B, 1), samples=x_n)

    def _ctrl_perturbation(self) -> dict:
        """The coefficient-table options of sde_ctrl_noise / sde_ctrl_dropout ({} when both are unset), checked.  Dropout replaces the control
        by -drift(t, x) / diff(t, x) of the loss's SDE: a loss without a linear SDE (DDS: sde=None) cannot have it -- the reference fails there
        too, with an AttributeError."""
        out = {}
        if self.sde_ctrl_noise is not None:
            out["ctrl_noise"] = float(self.sde_ctrl_noise)
        if self.sde_ctrl_dropout is not None:
            if not (hasattr(self.sde, "drift_coeff_t") and hasattr(self.sde, "diff_coeff_t")):
                raise ValueError(f"{type(self).__name__}: sde_ctrl_dropout replaces the control by -drift(t, x) / diff(t, x) of the loss's SDE "
                                 f"(losses/oc.py:101-102), which needs a linear (OU) SDE; this loss has "
                                 f"{type(self.sde).__name__ if self.sde is not None else 'sde=None'}")
            out["ctrl_dropout"] = float(self.sde_ctrl_dropout)
        return out

    def _integral_pass(self, t_unique, xs, zc):
        """The batched control pass, eager or -- ``graph_training`` -- as a captured graph per (shape, control): at the reference's
        training sizes the ~150 small kernels of its forward + backward are host-launch bound (tools/probe_training.py).  ``routes.lv_route`` decides."""
        route, ctrl = R.lv_route(self)
        if route == "fused":
            # the drift net of every RDS / LRDS solver (conf/model/basic.yaml), and the ScoreCtrl of PIS / DDS / DIS (conf/model/score.yaml):
            # fused HIP forward + backward of the net (csrc/grad_kernel.hpp); the score model's N cotangents from the HIP score kernel
            params = [p for p in ctrl.parameters() if p.requires_grad]
            return _FusedIntegral.apply(ctrl, t_unique, xs.contiguous(), zc.view(xs.shape), *params)
        key = (id(ctrl), tuple(xs.shape), str(xs.device))
        fn = self._graphed.get(key)
        if fn is None:
            fn = _IntegralPass(ctrl)
            if route == "graphed":
                try:
                    sample = (t_unique.detach().clone(), xs.detach().clone(), zc.detach().clone())
                    fn = torch.cuda.make_graphed_callables(fn, sample)
                except Exception as e:  # noqa: BLE001 -- capture is an optimisation: fall back to the eager pass, say so once
                    import warnings
                    warnings.warn(f"log-variance training: graph capture of the batched control pass failed ({type(e).__name__}: {e}); running it eagerly")
                    fn = _IntegralPass(ctrl)
            self._graphed[key] = fn
        return fn(t_unique, xs.contiguous(), zc)

    def _kl_loss(self, ts, x, launch, terminal):
        """KL training value and gradient (``method in ('kl', 'kl_ito')``): loss = mean of the log-weights over the particles that pass
        ``filter``, differentiated THROUGH the trajectory (BaseOCLoss.compute_loss losses/oc.py:105-131 on ``simulate(change_sde_ctrl=
        False)``, where the control that drives the SDE is the un-detached control: :258-260, :478-484, :1361-1365).

        VALUE: the HIP step loop -- one launch with the trajectory kept (and the noise of this call's Philox stream, redrawn below).
        GRADIENT: the discrete adjoint of exactly the recursion the kernel integrates (include/sdeng.h, FORM_LIN / FORM_EM with the
        host's per-step coefficients):
            lambda_N = d terminal / d x_N ;   for k = N-1 .. 0:  S_k = <lambda_{k+1}, x_{k+1}(x_k, theta)> + sum_b w_b d rnd_k,b(x_k, theta)
            lambda_k = dS_k/dx_k ,   dL/dtheta += dS_k/dtheta
        with the HIP states x_k as constants, no graph through the loop.  Three adjoints (losses/training.py), named by ``last_adjoint_path``:
        'native', the recursion as ONE launch (kl_grads_native, sdeng_kl_adjoint: DESIGN f-1); 'fused', one sdeng_ctrl_vjp per step
        (kl_grads_fused); 'stepwise', one torch vector-Jacobian product per step (kl_grads_stepwise).  This is the same number the
        reference's ``loss.backward()`` produces (fixtures ``train_kl_*``: loss to 6 digits, gradients to fp32 round-off)."""
        if self.sde_ctrl_noise is not None or self.sde_ctrl_dropout is not None:
            raise E.UnsupportedByEngine("sde_ctrl_noise / sde_ctrl_dropout perturb the simulated control (losses/oc.py:97-101): not built")
        x, x_n, rnd_sim, xs, ran, seed_c, N, B, d = T.rollout(self, ts, x, launch)
        z = E.philox_noise(seed_c, N, B, d, self.particle0, x.device)  # bit for bit the normals the kernel drew
        _, w, value = T.kl_weights(self, rnd_sim.reshape(B, 1), x_n)
        ctrl = self.generative_ctrl
        params = [p for p in ctrl.parameters() if p.requires_grad]
        with torch.enable_grad():
            xN = x_n.detach().requires_grad_(True)
            lam, = torch.autograd.grad((w * terminal(xN).view(B, 1)).sum(), xN)
        self.last_adjoint_path = R.kl_route(self, ran.decl.ref_ctrl)
        if self.last_adjoint_path == "native":
            grads = T.kl_grads_native(ctrl, params, ran, xs, z, w, lam)
        elif self.last_adjoint_path == "fused":
            grads = T.kl_grads_fused(ctrl, params, ran, xs, z, w, lam)
        else:
            grads = T.kl_grads_stepwise(self, ctrl, params, ran, xs, z, w, lam)
        return T.hand_to_autograd(self, value, params, grads)

    # ---- engine plumbing ---------------------------------------------------------------------
    @staticmethod
    def _logp(fn, x):
        """Gradient-free log-density ``fn(x)`` as [B,1]: one ``sdeng_dist_eval`` launch when ``fn`` is a method of a
        distribution the engine knows (a torch.distributions evaluation costs ~1 ms of host time per call, mostly argument
        validation with device read-backs); the callable itself otherwise."""
        res = E.resolve_logp(fn)
        if res is not None:
            try:
                logp, _ = E.dist_eval(res[0], x, want_logp=True, want_score=False)
                return logp if not res[1] else logp.clip(min=-res[1], max=res[1])  # clipped_target_unnorm_log_prob, solver/oc.py:80-87
            except E.UnsupportedByEngine:
                pass
        return fn(x).view((-1, 1))

    def _ctrl(self, use_ema):
        return self.generative_ctrl_ema if use_ema else self.generative_ctrl

    def _x0(self, x, seed=None):
        """``x`` as a tensor: an ``engine.InitialDraw`` (x0 left to the engine) is materialised with this loss's seed (a training call:
        that call's seed) and shard offset -- the same x0 sdeng_simulate draws itself when handed an InitialDraw."""
        return x.tensor(self.seed if seed is None else seed, self.particle0) if isinstance(x, E.InitialDraw) else x

    def _next_train_seed(self):
        seed_c = (int(self.seed) + 0x9E3779B97F4A7C15 * self.train_calls) & 0xFFFFFFFFFFFFFFFF
        self.train_calls += 1
        return seed_c

    def _sde_cpu(self):
        """CPU copy of the SDE for the per-step scalar tables, rebuilt when a buffer of the SDE changes (load_state_dict, edits)."""
        sig = tuple((b.data_ptr(), b._version) for b in self.sde.buffers()) if isinstance(self.sde, torch.nn.Module) else ()
        if self._cpu_sde is None or self._cpu_sde[0] != sig:
            self._cpu_sde = (sig, E._cpu_sde(self.sde))
            self._coef_cache = {}
        return self._cpu_sde[1]

    def _coef(self, ts, device, **kw):
        # per-step gains of the control wrapper itself (LerpCtrl: g(t) and t/T; CancelDriftCtrl: drift/g and g/2), whatever the loss
        rec = R.describe_ctrl(self.generative_ctrl)
        if rec.kind in (L.CTRL_LERP, L.CTRL_CANCEL_DRIFT) and kw.get("kind", self.kind) not in ("cmcd", "cmcd_eubo"):
            if rec.kind == L.CTRL_LERP:
                kw.setdefault("lerp", True)
            else:
                kw.setdefault("cancel", "rescale" if rec.ctrl.use_rescaling else "plain")
            if getattr(self, "_ctrl_sde_cpu", None) is None or self._ctrl_sde_cpu[0] is not rec.ctrl.sde:
                self._ctrl_sde_cpu = (rec.ctrl.sde, E._cpu_sde(rec.ctrl.sde))
            kw["ctrl_sde"] = self._ctrl_sde_cpu[1]
        sde_cpu = self._sde_cpu()  # (may clear the cache)
        # the entry holds `ts` itself: while it is cached its address cannot be handed to another grid, so (address, version) is an
        # identity -- a fresh ts per call with other values can never hit a stale table
        key = (ts.data_ptr(), ts._version, ts.numel(), str(device), tuple(sorted((k, str(v)) for k, v in kw.items())))
        hit = self._coef_cache.get(key)
        if hit is not None and hit[1] is ts:
            return hit[0]
        # another tensor object: compare by CONTENT (one small read-back) before paying for a new table
        kwkey = key[3:]
        ts_cpu = ts.detach().to("cpu", torch.float32)
        for old in self._coef_cache.values():
            if old[3] == kwkey and old[2].shape == ts_cpu.shape and torch.equal(old[2], ts_cpu):
                hit = (old[0], ts, old[2], kwkey)
                break
        else:
            kw2 = dict(kw)
            table = E.coef_table(kw2.pop("kind", self.kind), ts_cpu, sde_cpu, **kw2)
            hit = (table.to(device), ts, ts_cpu, kwkey)
        self._coef_cache = {key: hit}
        return hit[0]

    def _terminal(self, desc, keep, device, terminal_unnorm_log_prob, reference_log_prob):
        """Fill target / ref_dist + flags; returns the callables that stay opaque (evaluated with torch after)."""
        late = []
        res = E.resolve_logp(terminal_unnorm_log_prob) if terminal_unnorm_log_prob is not None else None
        ctrl_tgt, _ = E.ctrl_target(self.generative_ctrl)
        if res is not None:
            try:
                desc.target = E.dist_desc(res[0], device, keep, clip=res[1])
                desc.flags |= L.FLAG_TERM_TARGET
            except E.UnsupportedByEngine:
                res = None
        if res is None and terminal_unnorm_log_prob is not None:
            late.append((-1.0, terminal_unnorm_log_prob))
            desc.target = E.dist_desc(ctrl_tgt, device, keep, score_only=True)  # (SDENG_DIST_NONE where the control has no target)
        if reference_log_prob is not None:
            rr = E.resolve_logp(reference_log_prob)
            ok = False
            if rr is not None and desc.flags & L.FLAG_TERM_TARGET:
                try:
                    desc.ref_dist = E.dist_desc(rr[0], device, keep)
                    desc.flags |= L.FLAG_TERM_REF
                    ok = True
                except E.UnsupportedByEngine:
                    pass
            if not ok:
                late.append((1.0, reference_log_prob))
        return late

    @staticmethod
    def _apply_late(rnd, x, late):
        # opaque user callables: evaluated once on the device tensors, like the reference does (losses/oc.py:290)
        if late:
            term = 0.0
            for sign, fn in sorted(late, key=lambda p: -p[0]):
                term = term + sign * fn(x).view((-1, 1))
            rnd += term
        return rnd

    def _launch(self, loop, ts, x, *, terminal_unnorm_log_prob, reference_log_prob=None, initial_log_prob=None, use_ema=False, return_traj=False,
                noise=None, seed=None, perturb=None):
        """The step loop ``loop`` (a ``StepLoop``) as one launch -> (x_N, rnd, xs or None, ``engine.Launched``: what it ran on).  ``seed``: the Philox
        stream (default: the eval stream ``self.seed``); ``perturb``: ``_ctrl_perturbation()`` of a log-variance training call."""
        E.require_gpu(x)
        form, ref = loop.form, loop.ref
        seed = int(self.seed if seed is None else seed)
        coef_kw = dict(loop.coef_kw, **(perturb or {}))
        ctrl = self._ctrl(use_ema and loop.ema)
        if ref[0] == "nn":  # an energy-based reference: the step loop of sdeng_tilted_simulate
            return self._launch_nn(loop, ts, x, ctrl, coef_kw, terminal_unnorm_log_prob, reference_log_prob, initial_log_prob, return_traj, noise, seed,
                                   perturb)
        if isinstance(x, E.InitialDraw) and (form == L.FORM_EUBO or (initial_log_prob is not None and E.resolve_logp(initial_log_prob) is None)):
            x = self._x0(x, seed)  # an opaque initial log-density needs x0 as a tensor; the noising loops start from data anyway
        device = x.device
        ran = E.compile_ctrl(ctrl, self._coef(ts, device, **coef_kw), device, ref, decl=loop)
        keep, desc = ran.keep, E.new_desc()
        desc.form = form
        desc.N = ts.numel() - 1
        desc.seed = seed
        desc.particle0 = int(self.particle0)
        desc.flags = loop.flags | (L.FLAG_SPLIT_TILES if self.split_tiles and x.shape[0] <= L.SPLIT_TILES_MAX_B else 0)
        desc.net, desc.ref, desc.prior, desc.coef = ran.net, ran.ref, ran.prior, ran.coef.data_ptr()  # (the prior slot: a LerpCtrl's prior, SDENG_DIST_NONE without one, unless the kernel adds the initial log-density)
        _, remove = E.unwrap_ctrl(ctrl)
        if remove is not None:  # RemoveReferenceCtrl: u = ctrl - ref_score, with the reference score the step loop already evaluates
            if ref[0] == "none" or not E.same_reference(E.resolve_reference(remove.ref_score)[1], ref[1]):
                raise E.UnsupportedByEngine("RemoveReferenceCtrl.ref_score must be the loss's own reference_ctrl (the kernel subtracts the "
                                            "reference score it evaluates for the drift)")
            desc.flags |= L.FLAG_REMOVE_REF
        late = self._terminal(desc, keep, device, terminal_unnorm_log_prob, reference_log_prob)
        if desc.target.kind == L.DIST_GMM_FULL and (ref[0] != "none" or form == L.FORM_EUBO):
            raise E.UnsupportedByEngine("a full-covariance mixture target inside a Score / Lerp / CancelDrift control is evaluated in the kernel's "
                                        "reference slot: forward passes of the solvers without a reference drift (PIS / DDS / DIS) only")
        rnd0 = None
        if initial_log_prob is not None:
            pr = E.resolve_logp(initial_log_prob)
            try:
                if pr is None:
                    raise E.UnsupportedByEngine("opaque")
                desc.prior = E.dist_desc(pr[0], device, keep)
                desc.flags |= L.FLAG_INIT_LOGP
            except E.UnsupportedByEngine:
                rnd0 = initial_log_prob if form == L.FORM_EUBO else initial_log_prob(x).view((-1, 1))  # EUBO: at the noised samples
        if perturb:  # log-variance training with sde_ctrl_noise / sde_ctrl_dropout (BaseOCLoss._lv_loss)
            desc.flags |= (L.FLAG_CTRL_NOISE if "ctrl_noise" in perturb else 0) | (L.FLAG_CTRL_DROPOUT if "ctrl_dropout" in perturb else 0)
        x_out, rnd, xs = E.run(desc, x, keep, return_traj=return_traj, noise=noise, events=self.timing_events)
        if callable(rnd0):
            rnd0 = rnd0(x_out).view((-1, 1))
        if rnd0 is not None:
            rnd += rnd0
        rnd = self._apply_late(rnd, x if form == L.FORM_EUBO else x_out, late)  # EUBO: the cost at the data, x_in
        assert rnd.shape == (x.shape[0], 1)
        return x_out, rnd, xs, ran

    def _run(self, loop, ts, x, call, **kw):
        """simulate()'s launch -> (x_N, rnd, xs).  ``call`` is internal to the training calls (``training.launch_call``; None for every other
        caller): it carries a training call's seed and perturbation in and the launch's record out (``call.ran``)."""
        call = call or T.launch_call()
        *out, call.ran = self._launch(loop, ts, x, seed=call.seed, perturb=call.perturb, **kw)
        return tuple(out)

    def _nn_refusal(self, ctrl, form=None, perturb=None):
        """Why this loss cannot run over an energy-based ('nn') reference -- the reason, in words -- or None.  The kernel of
        sdeng_tilted_simulate holds the reference score and a ClippedCtrl; everything that would need the reference score inside the
        control, a perturbed control or the noising direction has no kernel there."""
        rec = R.describe_ctrl(ctrl)
        if rec.wrapper is not None:
            return "RemoveReferenceCtrl over an energy-based ('nn') reference: the kernel does not subtract the EBM's score from the control"
        if rec.kind != L.CTRL_CLIPPED:
            return (f"{R.name_of(rec.ctrl)} over an energy-based ('nn') reference: the one-launch step loop holds a ClippedCtrl only "
                    "(Score / Lerp / CancelDrift controls need the target score next to the EBM walk)")
        if self.sde_ctrl_noise is not None or self.sde_ctrl_dropout is not None or perturb:
            return "sde_ctrl_noise / sde_ctrl_dropout over an energy-based ('nn') reference: the kernel has no control-perturbation stage"
        if form == L.FORM_EUBO:
            return "compute_eubo over an energy-based ('nn') reference: no noising loop is built around the EBM walk"
        return None

    def _launch_nn(self, loop, ts, x, ctrl, coef_kw, terminal_unnorm_log_prob, reference_log_prob, initial_log_prob, return_traj, noise, seed, perturb):
        """``_launch`` over an energy-based reference (RDS.change_reference_type('nn'), solver/oc.py:577-585): one
        sdeng_tilted_simulate launch for the N steps, then the terminal costs with the launches that exist -- ``reference_log_prob``
        (WrapperDistrNN.log_prob: sdeng_tilted_eval at eps) and the target's log-density (sdeng_dist_eval) -- as losses/oc.py:290, :505, :645."""
        net, form = loop.ref[1]["net"], loop.form
        why = self._nn_refusal(ctrl, form, perturb)
        if why is None and initial_log_prob is not None:
            why = "an initial log-density over an energy-based ('nn') reference: the RDS losses have none"
        if why is None:
            why = E.tilted_refusal(net, x.device)
            why = why and f"energy-based ('nn') reference: {why}"
        if why is not None:
            raise E.UnsupportedByEngine(why)
        x = self._x0(x, seed)
        coef = self._coef(ts, x.device, **coef_kw)
        hit = self._nn_times
        if hit is None or hit[0] is not coef or hit[1] is not net:  # the reference's times of this grid: read back once per table
            t_net = coef[:, 0].detach().to("cpu")
            hit = self._nn_times = (coef, net, E.tilted_times(net, t_net, t_net.numel(), per_row=True)[2].to(x.device))
        x_out, rnd, xs, _ = E.tilted_simulate(net, ctrl, coef, hit[2], x, form=form, flags=loop.flags & L.FLAG_ITO, seed=seed,
                                              particle0=int(self.particle0), noise=noise, return_traj=return_traj)
        term = 0.0  # rnd += reference_log_prob(x) - terminal_unnorm_log_prob(x): the difference first, as upstream
        if reference_log_prob is not None:
            term = term + self._logp(reference_log_prob, x_out)
        if terminal_unnorm_log_prob is not None:
            term = term - self._logp(terminal_unnorm_log_prob, x_out)
        rnd += term
        assert rnd.shape == (x.shape[0], 1)
        return x_out, rnd, xs, E.Launched(coef, None, None, decl=loop)  # (log-variance training reads the table; no adjoint runs over an EBM)

    def _no_train(self, change_sde_ctrl):
        if change_sde_ctrl:
            raise E.UnsupportedByEngine("simulate(change_sde_ctrl=True) is the reference's internal training call: log-variance training "
                                        "runs through loss(ts, x, ...) here (BaseOCLoss._lv_loss: the HIP step loop with the detached "
                                        "control + one batched autograd pass, SURVEY.md 8f-1)")


class EMReferenceSDELoss(BaseOCLoss):
    """losses/oc.py:203-428 (RDS with Euler-Maruyama; PIS when ``reference_ctrl`` is None)."""

    kind = "em"

    def __init__(self, *args, reference_ctrl: Callable | None = None, use_rescaling: bool = True, **kwargs):
        super().__init__(*args, **kwargs)
        self.reference_ctrl = reference_ctrl
        self.use_rescaling = use_rescaling

    def _step_loop(self, train=False, ito=True, eubo=False, dim=None):
        ref = E.resolve_reference(self.reference_ctrl)
        if eubo:
            return StepLoop(L.FORM_EUBO, 0, dict(with_ref=True, kind="eubo_ei" if self.kind == "ei" else "eubo_em", rescale=bool(self.use_rescaling)), ref)
        if not self.use_rescaling and type(self) is EMReferenceSDELoss:
            raise E.UnsupportedByEngine("EMReferenceSDELoss(use_rescaling=False) scales the control twice upstream "
                                        "(losses/oc.py:265-267); not reproduced")
        with_ref = ref[0] != "none"  # (the Ito term is always part of these losses, :284, :499)
        return StepLoop(L.FORM_EM if self.kind == "em" else L.FORM_LIN, L.FLAG_ITO, dict(with_ref=with_ref), ref, self.reference_ctrl if with_ref else None)

    def simulate(self, ts, x, terminal_unnorm_log_prob, reference_log_prob, change_sde_ctrl=False, return_traj=False,
                 use_ema=False, *, noise=None, call=None):
        self._no_train(change_sde_ctrl)
        return self._run(self._step_loop(), ts, x, call, terminal_unnorm_log_prob=terminal_unnorm_log_prob, reference_log_prob=reference_log_prob,
                         use_ema=use_ema, return_traj=return_traj, noise=noise)

    def __call__(self, ts, x, terminal_unnorm_log_prob, reference_log_prob):
        """[TRAINING] losses/oc.py:364-394 with change_sde_ctrl = False (see BaseOCLoss._train)."""
        if E.resolve_reference(self.reference_ctrl)[0] == "nn":  # an energy-based reference: log-variance training of a ClippedCtrl only, refused before any rollout
            why = R.KL_OVER_NN if self.method in ("kl", "kl_ito") else self._nn_refusal(self.generative_ctrl)
            if why is not None:
                raise E.UnsupportedByEngine(why)
        return self._train(ts, x, terminal_unnorm_log_prob, dict(reference_log_prob=reference_log_prob))

    def compute_eubo(self, ts, x, terminal_unnorm_log_prob, reference_log_prob, use_ema=False, *, noise=None):
        """losses/oc.py:298-362 (EM; inherited by the DDPM-like loss) and :512-568 (EI): noising trajectories started at
        target samples ``x`` and the density log-ratio along them, as ONE HIP launch (SDENG_FORM_EUBO).  Like the
        reference, ``x`` is noised in place."""
        loop = self._step_loop(eubo=True)
        if loop.ref[0] == "none":
            raise E.UnsupportedByEngine("compute_eubo needs a reference control (RDS losses)")
        if loop.ref[0] == "nn":
            raise E.UnsupportedByEngine(R.KL_OVER_NN if self.method in ("kl", "kl_ito") else self._nn_refusal(self._ctrl(use_ema), L.FORM_EUBO))
        x_out, rnd, _, _ = self._launch(loop, ts, x, terminal_unnorm_log_prob=terminal_unnorm_log_prob, reference_log_prob=reference_log_prob,
                                        use_ema=use_ema, noise=noise)
        x.copy_(x_out)
        return rnd


class EIReferenceSDELoss(EMReferenceSDELoss):
    """losses/oc.py:431-568 (RDS with the exponential integrator)."""

    kind = "ei"

    def __init__(self, *args, reference_ctrl: Callable | None = None, **kwargs):
        kwargs.pop("use_rescaling", None)
        super().__init__(*args, reference_ctrl=reference_ctrl, use_rescaling=False, **kwargs)


class DDPMLikeReferenceSDELoss(EMReferenceSDELoss):
    """losses/oc.py:571-651 (RDS with DDPM-like transition kernels)."""

    kind = "ddpm"

    def __init__(self, *args, reference_ctrl: Callable | None = None, **kwargs):
        kwargs.pop("use_rescaling", None)
        super().__init__(*args, reference_ctrl=reference_ctrl, use_rescaling=False, **kwargs)


class _InitialLogProbLoss(BaseOCLoss):
    """Shared eval() of the losses that start from ``initial_log_prob`` (DIS / CMCD families)."""

    def compute_eubo(self, *a, **k):
        raise E.UnsupportedByEngine("no HIP noising loop for this loss's compute_eubo (TimeReversalLoss / ExponentialIntegratorSDELoss; the "
                                    "reference switches EUBO off for PIS and DDS too, solver/oc.py:356,436); the RDS losses', "
                                    "DiscreteTimeReversalLossEI's and ControlledLangevinSDELoss's are HIP launches")

    def eval(self, ts, x, terminal_unnorm_log_prob, initial_log_prob=None, compute_weights=True, return_traj=True,
             use_ema=True, *, noise=None) -> Results:
        kw = dict(compute_ito_int=compute_weights) if self.optional_ito else {}
        samples, rnd, xs = self.simulate(ts, x, terminal_unnorm_log_prob=terminal_unnorm_log_prob, initial_log_prob=initial_log_prob, train=False,
                                         return_traj=return_traj, use_ema=use_ema, noise=noise, **kw)
        return BaseOCLoss.compute_results(rnd, compute_weights=compute_weights, ts=ts, samples=samples, xs=xs, dist=self.dist)


class ControlledLangevinSDELoss(_InitialLogProbLoss):
    """losses/oc.py:654-894 (CMCD)."""

    kind = "cmcd"

    def __init__(self, *args, use_rescaling: bool = True, **kwargs):
        super().__init__(*args, **kwargs)
        self.use_rescaling = use_rescaling

    def _step_loop(self, train=False, ito=True, eubo=False, dim=None):
        if not self.use_rescaling:
            raise E.UnsupportedByEngine("ControlledLangevinSDELoss(use_rescaling=False) scales the control twice upstream "
                                        "(losses/oc.py:716-719); not reproduced")
        return StepLoop(L.FORM_CMCD_EUBO if eubo else L.FORM_CMCD, L.FLAG_ITO | L.FLAG_INIT_LOGP | L.FLAG_TERM_TARGET, dict(kind="cmcd_eubo") if eubo else {})

    def _launch(self, loop, ts, x, *, terminal_unnorm_log_prob, initial_log_prob=None, use_ema=False, return_traj=False, noise=None, seed=None, perturb=None):
        """CMCD's step loop (the kernel adds the initial log-density and the terminal target itself) -> (x_N, rnd, xs or None, what it ran on)."""
        E.require_gpu(x)
        seed = int(self.seed if seed is None else seed)
        if loop.form == L.FORM_CMCD_EUBO:
            x = self._x0(x, seed)
        desc, ran = E.cmcd_desc(self._ctrl(use_ema), self.sde, self._coef(ts, x.device, **loop.coef_kw), x.device, loop.form, decl=loop)
        res = E.resolve_logp(terminal_unnorm_log_prob)
        if res is None or res[0] is not R.self_of(self.sde.target_score):
            raise E.UnsupportedByEngine("CMCD: terminal_unnorm_log_prob must be the log-density of sde.target_score's distribution")
        pr = E.resolve_logp(initial_log_prob) if initial_log_prob is not None else None
        if pr is None or pr[0] is not R.self_of(self.sde.prior_score):
            raise E.UnsupportedByEngine("CMCD: initial_log_prob must be the log-density of sde.prior_score's distribution")
        desc.target.clip = float(res[1]) if res[1] else 0.0  # (clipped_target_unnorm_log_prob, solver/oc.py:80-87: the terminal term's, not the adjoint's)
        desc.flags, desc.N = loop.flags, ts.numel() - 1
        desc.seed, desc.particle0 = seed, int(self.particle0)
        return E.run(desc, x, ran.keep, return_traj=return_traj, noise=noise, events=self.timing_events) + (ran,)

    def simulate(self, ts, x, terminal_unnorm_log_prob, initial_log_prob=None, train=True, change_sde_ctrl=False,
                 return_traj=False, use_ema=False, *, noise=None, eubo=False, call=None):
        self._no_train(change_sde_ctrl)
        if train and self.method in ["kl", "kl_ito"]:
            raise E.UnsupportedByEngine("CMCD KL-training start (rnd0 = 0) is part of the training direction")
        return self._run(self._step_loop(eubo=eubo), ts, x, call, terminal_unnorm_log_prob=terminal_unnorm_log_prob, initial_log_prob=initial_log_prob,
                         use_ema=use_ema, return_traj=return_traj, noise=noise)

    def compute_eubo(self, ts, x, terminal_unnorm_log_prob, initial_log_prob=None, use_ema=False, *, noise=None):
        """losses/oc.py:757-828: the CMCD loop run from target samples with the control subtracted, one HIP launch
        (SDENG_FORM_CMCD_EUBO; diagonal Gaussian / mixture, rings and checkerboard targets -- the ones that can be sampled).  ``x`` is NOT modified
        (upstream rebinds it, :820)."""
        _, rnd, _ = self.simulate(ts, x, terminal_unnorm_log_prob, initial_log_prob=initial_log_prob, train=False, use_ema=use_ema,
                                  noise=noise, eubo=True)
        return rnd

    def __call__(self, ts, x, terminal_unnorm_log_prob, initial_log_prob=None):
        """[TRAINING] losses/oc.py:830-857, log-variance methods.  The trajectory is driven by the detached control
        (:704-705, :722), so it is the eval trajectory: one HIP launch (trajectory and noise kept).  The target / prior
        scores along it come from the HIP distribution kernels (no graph needed: the states are constants), and one batched
        autograd pass of the control over the (N+1)*B (time, state) pairs rebuilds (:736-742)
            cost_k = (b_k + b'_k)/g + u_k - u_{k+1},   rnd = rnd0 + sum_k 0.5|cost_k|^2 dt + <cost_k, u_k.detach() - u_k> dt + <cost_k, db_k> - log pi~(x_N)
        with b_k = drift(t_k, x_k), b'_k = drift(t_{k+1}, x_{k+1})."""
        if self.sde_ctrl_noise is not None or self.sde_ctrl_dropout is not None:
            raise E.UnsupportedByEngine("sde_ctrl_noise / sde_ctrl_dropout perturb the simulated control: not built")
        if self.method in ("kl", "kl_ito"):
            return self._kl_loss_cmcd(ts, x, terminal_unnorm_log_prob, initial_log_prob)
        x, _, _, _, _, seed_c, N, B, d = T.rollout(self, ts, x)  # (the step loop below replays the injected z on the eval stream: no seed in its call)
        z = E.philox_noise(seed_c, N, B, d, self.particle0, x.device)
        g = float(self.sde.diff_coeff)
        call = T.launch_call()
        with torch.no_grad():
            x_n, _, xs = self.simulate(ts, x, terminal_unnorm_log_prob, initial_log_prob=initial_log_prob, train=False,
                                       return_traj=True, use_ema=False, noise=z, call=call)
            b_all, _ = self._cmcd_drifts(call.ran.coef, xs)  # eq/sdes.py:101-110 at every (ts[j], xs[j]); the table the step loop ran on
            b_s, b_t = b_all[:-1], b_all[1:]
            const = -terminal_unnorm_log_prob(x_n)
            if initial_log_prob is not None:
                const = const + initial_log_prob(x).view((-1, 1))
        u = ctrl_batched(self.generative_ctrl, ts.to(x.device), xs).view(N + 1, B, d)
        dt = (ts[1:] - ts[:-1]).view(N, 1, 1)
        db = dt.sqrt() * z
        cost = (b_s + b_t) / g + u[:-1] - u[1:]
        rnd = (0.5 * (cost ** 2).sum(-1) * dt.view(N, 1) + (cost * (u[:-1].detach() - u[:-1])).sum(-1) * dt.view(N, 1)
               + (cost * db).sum(-1)).sum(0).view(B, 1) + const
        return self.compute_loss(rnd, samples=x_n)

    def _cmcd_drifts(self, coef, xs):
        """The annealed drift b_j = clip(0.5 g^2 (tau_j s_pi(x_j) + (1 - tau_j) s_prior(x_j))) (eq/sdes.py:101-110) at all N + 1 evaluation points
        of the HIP states ``xs`` [N+1,B,d], without a graph: target and prior scores of all rows from the distribution kernels, the annealing
        weights tau_j = ts[j]/T from the step loop's own table ``coef`` (columns 4-7).  -> (b [N+1,B,d], target scores [(N+1)*B, d]).  Shared by
        log-variance training and by the cost pass of the KL adjoint."""
        M, B, d = xs.shape
        N = M - 1
        target, prior = R.self_of(self.sde.target_score), R.self_of(self.sde.prior_score)
        flat = xs.reshape(M * B, d)
        _, s_tgt = E.dist_eval(target, flat, want_logp=False)
        _, s_pri = E.dist_eval(prior, flat, want_logp=False)
        g = float(self.sde.diff_coeff)
        tau = torch.cat([coef[:N, 4], coef[N - 1:N, 6]]).view(M, 1, 1)
        omt = torch.cat([coef[:N, 5], coef[N - 1:N, 7]]).view(M, 1, 1)
        b = (s_tgt.view(M, B, d) * tau + s_pri.view(M, B, d) * omt) * (0.5 * g ** 2)
        if self.sde.clip_score:
            b = b.clip(-float(self.sde.clip_score), float(self.sde.clip_score))
        return b, s_tgt

    def _cmcd_step_costs(self, ctrl, coef, xs, z):
        """cost_j dt_j + db_j [N,B,d] of the CMCD steps on the HIP states ``xs`` [N+1,B,d] (losses/oc.py:722-742), without a graph: the drifts
        of ``_cmcd_drifts``, the drift net from one forward launch, the rest elementwise.  Also returns the target scores [(N+1)*B, d]."""
        from ..models.reparam import _clip
        M, B, d = xs.shape
        N = M - 1
        g = float(self.sde.diff_coeff)
        b, s_tgt = self._cmcd_drifts(coef, xs)
        u = E.ctrl_forward_rows(fused_net_view(ctrl), coef[:, 0], xs)
        if R.describe_ctrl(ctrl).own_kind == L.CTRL_SCORE:
            sc = ctrl.scale_score * _clip(s_tgt, ctrl.clip_score).view(M, B, d)
            if ctrl.score_model is not None:
                sc = sc * ctrl.clipped_score_model(coef[:, 0].contiguous().view(-1, 1), None).view(M, 1, 1)
            u = u + sc
        cost = (b[:-1] + b[1:]) / g + u[:-1] - u[1:]
        return cost * coef[:N, 2].view(N, 1, 1) + coef[:N, 3].view(N, 1, 1) * z, s_tgt

    def _kl_loss_cmcd(self, ts, x, terminal_unnorm_log_prob, initial_log_prob):
        """[TRAINING] KL methods of CMCD (losses/oc.py:830-857 on simulate(train=True): rnd0 = 0, :695-699; the un-detached control drives
        the SDE, :706-709).  VALUE: the HIP step loop (its log-weight minus the initial log-density it adds).  GRADIENT: the discrete
        adjoint of the reference's own step (:711-742) -- y = x + (b_s(x) + g u_s(x)) dt + g db, cost = (b_s(x) + b_t(y))/g + u_s(x) - u_t(y),
        rnd += 0.5 |cost|^2 dt + <cost, db> -- over the HIP states: as ONE launch where sdeng_cmcd_kl_adjoint covers the loss
        (``last_adjoint_path`` 'native'), else one torch vector-Jacobian product per step ('stepwise': two control evaluations share the
        state y, so the step is differentiated as a whole; the target / prior scores are differentiated exactly where the reference's are:
        closed-form scores carry a graph, autograd-made ones do not, distr/base.py:146-154).  The shared pieces: losses/training.py."""
        x, x_n, rnd_sim, xs, ran, seed_c, N, B, d = T.rollout(self, ts, x, lambda xx, call: self.simulate(
            ts, xx, terminal_unnorm_log_prob, initial_log_prob=initial_log_prob, train=False, return_traj=True, call=call))
        z = E.philox_noise(seed_c, N, B, d, self.particle0, x.device)  # bit for bit the normals the kernel drew
        _, w, value = T.kl_weights(self, rnd_sim.reshape(B, 1) - self._logp(initial_log_prob, x), x_n)  # (the evaluation pass starts from log p_prior(x0), training from 0)
        ctrl = self.generative_ctrl
        params = [p for p in ctrl.parameters() if p.requires_grad]
        g = self.sde.diff_coeff
        # lambda_N = d (sum_b w_b (-log pi~(x_N,b))) / d x_N.  A piecewise-constant density (the checkerboard) builds no graph to x_N: its
        # terminal term contributes nothing to the reference's backward() either.
        with torch.enable_grad():
            xN = x_n.detach().requires_grad_(True)
            out = (w * (-terminal_unnorm_log_prob(xN).view(B, 1))).sum()
            lam = torch.autograd.grad(out, xN)[0] if out.requires_grad else torch.zeros_like(xN)

        self.last_adjoint_path = R.cmcd_kl_route(self)
        if self.last_adjoint_path == "native":
            # the kernel's input, the per-step cost cotangents, is one batched forward pass over the HIP states; parameter gradients as in _kl_loss
            coef = ran.coef
            with torch.no_grad():
                cbar, s_tgt = self._cmcd_step_costs(ctrl, coef, xs, z)
            graphless = R.dist_kind(R.self_of(self.sde.target_score)) in R.GRAPHLESS_TARGETS
            arrays, _ = E.cmcd_kl_adjoint(ctrl, self.sde, coef, xs, cbar, w, lam, score_ext=s_tgt if graphless else None, parts=ran)
            return T.hand_to_autograd(self, value, params, T.param_grads(ctrl, coef[:, 0].contiguous(), arrays, N + 1, B, params))
        grads = [torch.zeros_like(p) for p in params]

        def step(lam_in, x_in, z_in, s, t, w_in):
            """One step of the adjoint: lambda_k and the parameter-gradient contributions of step k (accumulated into ``grads``)."""
            with torch.enable_grad():
                dt = t - s
                db = dt.sqrt() * z_in
                xk = x_in.detach().requires_grad_(True)
                u_s, b_s = ctrl(s, xk), self.sde.drift(s, xk)
                y = xk + (b_s + u_s * g) * dt + g * db
                cost = (b_s + self.sde.drift(t, y)) / g + u_s - ctrl(t, y)
                dr = 0.5 * (cost ** 2).sum(-1, keepdim=True) * dt + (cost * db).sum(-1, keepdim=True)
                got = torch.autograd.grad((lam_in * y).sum() + (w_in * dr).sum(), [xk] + params, allow_unused=True)
            for acc, gk in zip(grads, got[1:]):
                if gk is not None:
                    acc.add_(gk)
            return got[0]

        tdev = ts.to(x.device)  # (the ~130 small kernels of a step are launch-bound, 2048 x 100: 5 ms per step: walk_adjoint replays them as a hipGraph)
        found = T.walk_adjoint(self, ("cmcd", id(ctrl), B, d, str(x.device)), step, grads, lam, lambda k: (xs[k], z[k], tdev[k], tdev[k + 1], w), N,
                               self.graph_adjoint and R.graph_capturable(ctrl, self.sde.target_score))
        return T.hand_to_autograd(self, value, params, found)


class DiscreteTimeReversalLossEI(_InitialLogProbLoss):
    """losses/oc.py:897-1102 (DIS with the exponential integrator)."""

    kind = "dis_ei"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.use_rescaling = False

    def _step_loop(self, train=False, ito=True, eubo=False, dim=None):
        if eubo:
            return StepLoop(L.FORM_EUBO, 0, dict(kind="eubo_ei"))
        return StepLoop(L.FORM_LIN, L.FLAG_ITO, {}, init=not (train and self.method in ("kl", "kl_ito")))  # rnd0 = 0 for the KL methods (:935-939)

    def simulate(self, ts, x, terminal_unnorm_log_prob, initial_log_prob=None, train=True, change_sde_ctrl=False,
                 return_traj=False, use_ema=False, *, noise=None, call=None):
        self._no_train(change_sde_ctrl)
        loop = self._step_loop(train)
        return self._run(loop, ts, x, call, terminal_unnorm_log_prob=terminal_unnorm_log_prob, initial_log_prob=initial_log_prob if loop.init else None,
                         use_ema=use_ema, return_traj=return_traj, noise=noise)

    def __call__(self, ts, x, terminal_unnorm_log_prob, initial_log_prob=None):
        """[TRAINING] losses/oc.py:1038-1066 (log-variance: rnd0 = log p_prior(x0); terminal -log pi~)."""
        return self._train(ts, x, terminal_unnorm_log_prob, {}, rnd0=initial_log_prob)

    def compute_eubo(self, ts, x, terminal_unnorm_log_prob, initial_log_prob=None, use_ema=False, *, noise=None):
        """losses/oc.py:980-1036: noising trajectories from target samples (no reference; cost 0.5|u|^2 omega, Ito term,
        + log p_prior of the noised samples), one HIP launch.  ``x`` is noised in place like upstream."""
        if initial_log_prob is None:
            raise ValueError("compute_eubo needs initial_log_prob (the reference calls it unconditionally, losses/oc.py:1032)")
        x_out, rnd, _, _ = self._launch(self._step_loop(eubo=True), ts, x, terminal_unnorm_log_prob=terminal_unnorm_log_prob,
                                        initial_log_prob=initial_log_prob, use_ema=use_ema, noise=noise)
        x.copy_(x_out)
        return rnd


class TimeReversalLoss(_InitialLogProbLoss):
    """losses/oc.py:1105-1307 (original DIS, without inference control)."""

    kind = "time_reversal"
    optional_ito = True

    def __init__(self, *args, inference_ctrl: Callable | None = None, div_estimator: str | None = None,
                 use_rescaling: bool = True, **kwargs):
        super().__init__(*args, **kwargs)
        if not use_rescaling:
            raise ValueError("use_rescaling must be True for TimeReversalLoss.")
        self.inference_ctrl, self.div_estimator, self.use_rescaling = inference_ctrl, div_estimator, use_rescaling

    def _step_loop(self, train=False, ito=True, eubo=False, dim=None):
        if self.inference_ctrl is not None:
            raise E.UnsupportedByEngine("a learned inference control needs the divergence of a net (autograd): not on the HIP path")
        lerp = R.describe_ctrl(self.generative_ctrl).own_kind == L.CTRL_LERP
        # ema=False: quirk kept, TimeReversalLoss.simulate never uses the EMA net (losses/oc.py:1177-1180)
        return StepLoop(L.FORM_EM, L.FLAG_ITO if ito else 0, dict(train=train, dim=dim, lerp=lerp),
                        init=not (train and self.method in ("kl", "kl_ito")), ema=False)

    def simulate(self, ts, x, terminal_unnorm_log_prob, initial_log_prob=None, train=True, compute_ito_int=False,
                 change_sde_ctrl=False, return_traj=False, use_ema=False, *, noise=None, call=None):
        self._no_train(change_sde_ctrl)
        loop = self._step_loop(train, compute_ito_int, dim=x.shape[-1])
        return self._run(loop, ts, x, call, terminal_unnorm_log_prob=terminal_unnorm_log_prob, initial_log_prob=initial_log_prob if loop.init else None,
                         use_ema=use_ema, return_traj=return_traj, noise=noise)

    def __call__(self, ts, x, terminal_unnorm_log_prob, initial_log_prob=None):
        """[TRAINING] losses/oc.py:1240-1272, no inference control: cost <u, u.detach() - u/2> dt + <u, db>; :1251 compute_ito_int = self.method != "kl"."""
        return self._train(ts, x, terminal_unnorm_log_prob, dict(compute_ito_int=self.method != "kl"), rnd0=initial_log_prob)


class ExponentialIntegratorSDELoss(BaseOCLoss):
    """losses/oc.py:1310-1467 (DDS)."""

    kind = "dds"
    optional_ito = True

    def __init__(self, *args, alpha: float, sigma: float, **kwargs):
        super().__init__(*args, **kwargs)
        self.alpha, self.sigma = alpha, sigma

    def _step_loop(self, train=False, ito=True, eubo=False, dim=None):
        return StepLoop(L.FORM_LIN, L.FLAG_ITO if ito else 0, dict(alpha=self.alpha, sigma=self.sigma))

    def simulate(self, ts, x, terminal_unnorm_log_prob, reference_log_prob, compute_ito_int=False, change_sde_ctrl=False,
                 return_traj=False, use_ema=False, *, noise=None, call=None):
        self._no_train(change_sde_ctrl)
        return self._run(self._step_loop(ito=compute_ito_int), ts, x, call, terminal_unnorm_log_prob=terminal_unnorm_log_prob,
                         reference_log_prob=reference_log_prob, use_ema=use_ema, return_traj=return_traj, noise=noise)

    def __call__(self, ts, x, terminal_unnorm_log_prob, reference_log_prob):
        """[TRAINING] losses/oc.py:1399-1428; :1414 compute_ito_int = self.method != "kl"."""
        return self._train(ts, x, terminal_unnorm_log_prob, dict(reference_log_prob=reference_log_prob, compute_ito_int=self.method != "kl"))
