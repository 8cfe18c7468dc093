"""What the training calls of ``oc.py`` share (host Python only; the loss classes keep their own mathematics): the batched control pass of
log-variance training (``ctrl_batched``, ``_IntegralPass``, the fused ``_FusedIntegral``), the rollout, the KL weights, the parameter gradients from
a training kernel's per-row arrays, the hand-off to autograd, the three adjoints of ``_kl_loss`` and the graph-captured per-step runner."""
from __future__ import annotations

import types

import torch

from .. import _lib as L
from .. import engine as E
from .. import parallel
from .. import routes as R


def ctrl_batched(ctrl, t_unique: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """``ctrl(t, x)`` (with autograd) for M distinct times and B states per time, x [M,B,d] -> [M*B,d].  Same operations
    as the modules' own forward (models/mlp.py, models/reparam.py), except that the time embeddings -- functions of t only --
    are evaluated once per distinct time instead of once per row (the reference recomputes them for every particle,
    models/mlp.py:136-137); other control types fall back to the plain per-row call."""
    from ..models.reparam import _clip
    M, B, d = x.shape
    flat = x.reshape(M * B, d)
    t_rows = t_unique.repeat_interleave(B).view(-1, 1)
    rec = R.describe_ctrl(ctrl)
    if rec.own_kind is None or R.name_of(ctrl.base_model) != "FourierMLP":  # (a wrapped control is called as a whole)
        return ctrl(t_rows, flat)
    kind, net = rec.kind, ctrl.base_model
    h = net.input_embed(flat) + net.timestep_embed(t_unique.view(-1, 1)).repeat_interleave(B, dim=0)
    for layer in net.hidden_layer:
        h = layer(net.activation(h))
    out = _clip(net.out_layer(net.activation(h)), ctrl.clip_model)
    if kind == L.CTRL_CLIPPED:
        return out
    if kind == L.CTRL_LERP:
        score = ctrl.scale_score * ctrl.clipped_interpolated_score(t_rows, flat)
    else:
        score = ctrl.scale_score * ctrl.clipped_target_score(t_rows, flat)
    if ctrl.score_model is not None:
        score = score * _clip(ctrl.score_model(t_unique.view(-1, 1)), ctrl.clip_model).repeat_interleave(B, dim=0)
    if kind == L.CTRL_CANCEL_DRIFT:  # reparam.py:142-145
        g, f = ctrl.sde.diff(t_rows, flat), ctrl.sde.drift(t_rows, flat)
        return out + (f / g) + 0.5 * g * score if ctrl.use_rescaling else out + (f / torch.square(g)) + 0.5 * score
    return out + (ctrl.sde.diff(t_rows, flat) * score if kind == L.CTRL_LERP else score)


class _FusedIntegral(torch.autograd.Function):
    """s_b = sum_k <u_theta(t_k, x_kb), zc_kb> for a ClippedCtrl over a FourierMLP, with the gradient w.r.t. the net's parameters from
    ONE fused HIP forward + backward over all N * B rows (``sdeng_ctrl_vjp``, csrc/grad_kernel.hpp) and six skinny GEMMs -- instead of
    the ~150 small kernels of the eager torch pass.  The VALUE of s is not needed by the losses (it enters as ``s - s.detach()``), so
    ``forward`` returns zeros and all the work happens in ``backward``, where the cotangent of s_b (one number per particle) is known."""

    @staticmethod
    def forward(ctx, ctrl, t_unique, xs, zc, *params):
        ctx.ctrl, ctx.shape = ctrl, tuple(xs.shape)
        ctx.save_for_backward(t_unique, xs, zc)
        return torch.zeros(xs.shape[1], dtype=xs.dtype, device=xs.device)

    @staticmethod
    def backward(ctx, grad_s):
        t_unique, xs, zc = ctx.saved_tensors
        N, B, d = ctx.shape
        cot = zc.view(N, B, d) * grad_s.view(1, B, 1)  # d loss / d u_kb
        ctrl = ctx.ctrl
        net_view = fused_net_view(ctrl)
        grads = vjp_param_grads(net_view, t_unique, E.ctrl_vjp(net_view, t_unique, xs, cot), N, B)
        sm_params = _score_model_params(ctrl) if net_view is not ctrl else []
        if sm_params:
            # ScoreCtrl: u = clip(net) + scale clip(score_pi(x)) s_theta(t).  The states are constants, so the score part only reaches the
            # score model: d loss / d s_theta(t_k) = sum_b <cot_kb, scale clip(score_pi(x_kb))> (HIP score kernel, one launch for all rows)
            from ..models.reparam import _clip
            _, sc = E.dist_eval(E.ctrl_target(ctrl)[0], xs.reshape(N * B, d), want_logp=False, want_score=True)
            dst = (cot.reshape(N * B, d) * (ctrl.scale_score * _clip(sc, ctrl.clip_score))).sum(-1).view(N, B).sum(1)
            grads.update(score_model_grads(ctrl, t_unique, sm_params, dst))
        params = [p for p in ctrl.parameters() if p.requires_grad]
        return (None, None, None, None) + tuple(grads.get(p) for p in params)


_NET_VIEWS = {}
fused_training_ok, _capturable = R.lv_fused, R.graph_capturable  # (the names they have here)


def fused_net_view(ctrl):
    """The ClippedCtrl part of a ScoreCtrl (same drift net, same clip) as sdeng_ctrl_vjp wants it; a ClippedCtrl is its own view."""
    if R.describe_ctrl(ctrl).own_kind == L.CTRL_CLIPPED:
        return ctrl
    view = _NET_VIEWS.get(id(ctrl))
    if view is None or view[0]() is not ctrl or view[1].clip_model != ctrl.clip_model:
        import weakref

        from ..models.reparam import ClippedCtrl
        view = (weakref.ref(ctrl), ClippedCtrl(base_model=ctrl.base_model, clip_model=ctrl.clip_model))
        _NET_VIEWS[id(ctrl)] = view
    return view[1]


def vjp_param_grads(ctrl, t_unique, r, N, B):
    """Per-row arrays of ``sdeng_ctrl_vjp`` (include/sdeng.h) -> {parameter: gradient} for a ClippedCtrl over a FourierMLP."""
    net = ctrl.base_model

    def outer(dl, act):
        # dl^T act over all N * B rows.  As ONE GEMM this is 64 x 64 (or d x 64) with K = N * B: hipBLASLt runs it on a handful of
        # workgroups (180 us each at 512 x 100 rows, rocprofv3); batched over the N times and summed it fills the chip (~10 us).
        return torch.bmm(dl.view(N, B, -1).transpose(1, 2), act.view(N, B, -1)).sum(0)
    grads = {net.out_layer.weight: outer(r["dout"], r["a2"]), net.out_layer.bias: r["dout"].sum(0),
             net.hidden_layer[1].weight: outer(r["d2"], r["a1"]), net.hidden_layer[1].bias: r["d2"].sum(0),
             net.hidden_layer[0].weight: outer(r["d1"], r["a0"]), net.hidden_layer[0].bias: r["d1"].sum(0),
             net.input_embed.weight: outer(r["d0"], r["x"]), net.input_embed.bias: r["d0"].sum(0)}
    # time embedding e_t = timestep_embed(t_k): its cotangent is the sum over the particles of d0; the small module itself (2 layers on
    # N rows) is differentiated by torch
    te_params = [p for p in net.timestep_embed.parameters() if p.requires_grad]
    if te_params:
        with torch.enable_grad():
            e = net.timestep_embed(t_unique.view(-1, 1))
            te_grads = torch.autograd.grad(e, te_params, grad_outputs=r["d0"].view(N, B, 64).sum(1), allow_unused=True)
        grads.update({p: g for p, g in zip(te_params, te_grads) if g is not None})
    return grads


class _IntegralPass(torch.nn.Module):
    """s_b = sum_k <u(t_k, x_kb), zc_kb>: the one part of the log-variance loss that carries a graph (BaseOCLoss._lv_loss)."""

    def __init__(self, ctrl):
        super().__init__()
        self.ctrl = ctrl

    def forward(self, t_unique, xs, zc):
        u = ctrl_batched(self.ctrl, t_unique, xs)
        return (u * zc).sum(dim=-1).view(xs.shape[0], xs.shape[1]).sum(dim=0)


# ---- the pieces every training call shares -----------------------------------------------------------------------------------------
def launch_call(seed=None, perturb=None):
    """The internal ``call`` argument of the losses' ``simulate``: a training call's Philox seed and perturbation options in (None: the eval
    stream, no perturbation), the launch's record out (``ran``: ``engine.Launched``)."""
    return types.SimpleNamespace(seed=seed, perturb=perturb, ran=None)


def rollout(loss, ts, x, simulate=None, perturb=None):
    """The front of every training call: one fresh Philox stream (the reference consumes torch's global generator; call c here uses seed + c *
    golden-ratio increment for the step noise AND for an x0 left to the engine, call 0 being the eval stream of ``seed``), x0 as a tensor, the
    ``traj_per_sample`` repeat.  With ``simulate`` (a callable of x0 and ``call``) the HIP step loop runs on that stream and with the table options
    ``perturb`` of a perturbed log-variance call -- both travel as the argument ``call``, which comes back holding the launch's record ``ran``
    (``engine.Launched``); a caller that needs the kernel's normals redraws them bit for bit with ``E.philox_noise(seed_c, N, B, d,
    loss.particle0, x.device)``.  -> (x, x_n, rnd_sim, xs, ran, seed_c, N, B, d)."""
    E.require_gpu(x)
    seed_c = loss._next_train_seed()
    x = loss._x0(x, seed_c)
    if loss.traj_per_sample != 1:
        x = x.repeat(loss.traj_per_sample, 1, 1).reshape(-1, x.shape[-1])
    N, (B, d) = ts.numel() - 1, x.shape
    x_n = rnd_sim = xs = None
    call = launch_call(seed_c, perturb)
    if simulate is not None:
        with torch.no_grad():
            x_n, rnd_sim, xs = simulate(x, call)
    return x, x_n, rnd_sim, xs, call.ran, seed_c, N, B, d


def kl_weights(loss, rnd_val, x_n):
    """KL value of the particles that pass ``loss.filter`` and its cotangent: -> (mask, w = d mean(rnd[mask]) / d rnd_b, value).  A sharded run
    (``loss.dist``: a process group of more than one rank): the mean is over ALL ranks' kept particles (``parallel.global_moments``, one 32-byte
    all-gather), so w divides by the global count and every adjoint downstream yields this rank's exact partial sum of the global gradient."""
    mask = loss.filter(rnd_val, samples=x_n)
    assert mask.shape == rnd_val.shape
    if parallel.is_sharded(loss.dist):
        mom = parallel.global_moments(rnd_val, mask, loss.dist)
        n = mom[parallel.M_N]
        loss.n_filtered += int(mom[parallel.M_ROWS] - n)
        return mask, mask.to(rnd_val.dtype) / n.to(rnd_val.dtype), parallel.kept_mean(mom).to(rnd_val.dtype)
    loss.n_filtered += (mask.numel() - mask.sum()).item()
    w = mask.to(rnd_val.dtype) / mask.sum()
    return mask, w, rnd_val[mask].mean()


def score_model_grads(ctrl, t_unique, sm_params, dst):
    """{parameter: gradient} of a Score control's score model from the cotangents ``dst`` [M] of s_theta(t_k): the small module is torch's to differentiate."""
    with torch.enable_grad():
        st = ctrl.clipped_score_model(t_unique.view(-1, 1), None).view(-1)
        sm_grads = torch.autograd.grad(st, sm_params, grad_outputs=dst, allow_unused=True)
    return {p: g for p, g in zip(sm_params, sm_grads) if g is not None}


def _score_model_params(ctrl):
    sm = getattr(ctrl, "score_model", None)
    return [p for p in sm.parameters() if p.requires_grad] if sm is not None else []


def param_grads(ctrl, t_unique, arrays, M, B, params):
    """Per-row arrays of sdeng_ctrl_vjp / sdeng_kl_adjoint / sdeng_cmcd_kl_adjoint over M times x B rows -> the gradients, ordered as ``params`` (zeros
    where there is none): the drift net's from ``vjp_param_grads``, the score model's from the cotangents ``dst`` [M,B] of s_theta(t_k) when the kernel wrote them."""
    found = vjp_param_grads(ctrl, t_unique, arrays, M, B)
    sm_params = _score_model_params(ctrl) if arrays.get("dst") is not None else []
    if sm_params:
        found.update(score_model_grads(ctrl, t_unique, sm_params, arrays["dst"].sum(1)))
    return [found.get(p, torch.zeros_like(p)) for p in params]


def hand_to_autograd(loss, value, params, grads):
    """The training call's return value: value + sum <p - p.detach(), dL/dp> (zero-valued, gradient dL/dp), and the metrics dict."""
    surrogate = sum(((p - p.detach()) * g).sum() for p, g in zip(params, grads))
    return value.detach() + surrogate, {"train/n_filtered_cumulative": loss.n_filtered}


def walk_adjoint(loss, key, step, grads, lam, rest, N, graph):
    """The adjoint recursion one torch step at a time, k = N-1 .. 0: ``lam = step(lam, *rest(k))``, with ``step`` accumulating the parameter
    gradients into ``grads``.  The step is launch-bound (60 - 130 small kernels): with ``graph`` it is captured once per ``key`` as a hipGraph
    and replayed N times; a capture that fails runs the steps eagerly, and says so.  -> the gradients."""
    runner = _graphed_step(loss, key, step, grads, (lam,) + rest(0)) if graph else None
    for k in range(N - 1, -1, -1):
        args = (lam,) + rest(k)
        lam = runner(*args) if runner is not None else step(*args)
    return [gr.clone() for gr in runner.grads] if runner is not None else grads


# ---- the three adjoints of BaseOCLoss._kl_loss: each -> the gradients, ordered as ``params`` -------------------------------------------------
def kl_grads_native(ctrl, params, ran, xs, z, w, lam):
    """A control ``routes.kl_native`` accepts, no / a diagonal reference: the whole recursion is ONE launch (sdeng_kl_adjoint: lambda in registers, u
    recomputed, closed-form Hessian-vector products) over the parts the step loop's launch compiled; the parameter gradients come from the
    per-row arrays, as in log-variance training."""
    coef, lin, ito = ran.coef, ran.decl.lin, ran.decl.ito
    N, B = xs.shape[0] - 1, xs.shape[1]
    arrays, _ = E.kl_adjoint(ctrl, coef, xs[:-1], z if ito else None, w, lam, lin=lin, ito=ito, parts=ran)
    return param_grads(ctrl, coef[:, 0].contiguous(), arrays, N, B, params)


def kl_grads_fused(ctrl, params, ran, xs, z, w, lam):
    """ClippedCtrl over the FourierMLP with a reference the one-launch kernel does not differentiate: the control's part of each step's
    vector-Jacobian product is the fused HIP forward + backward of that time step (sdeng_ctrl_vjp; weights packed once per call), the
    reference score's part a small torch VJP; the parameter gradients come from the per-row arrays at the end."""
    coef, lin, ito, reference_ctrl = ran.coef, ran.decl.lin, ran.decl.ito, ran.decl.ref_ctrl
    N, B = xs.shape[0] - 1, xs.shape[1]
    sess = E.VjpSession(ctrl, coef[:, 0], xs[:-1])
    u_all = sess.forward_u()
    with torch.enable_grad():
        for k in range(N - 1, -1, -1):
            c, u, zk = coef[k], u_all[k], z[k]
            if lin:
                g = c[2] * lam + w * (2.0 * c[4] * u + (c[5] * zk if ito else 0.0))
            else:
                g = (c[2] * c[4]) * lam + w * (c[4] * u + (c[5] * zk if ito else 0.0))
            gx = sess.step(k, g)
            jl = None
            if reference_ctrl is not None:
                xk = xs[k].detach().requires_grad_(True)
                jl, = torch.autograd.grad((reference_ctrl(c[0], xk) * lam).sum(), xk)
            if lin:
                lam = c[1] * lam + gx if jl is None else c[1] * lam + c[2] * jl + gx
            else:
                lam = (1.0 + c[4] * c[1]) * lam + gx if jl is None else (1.0 + c[4] * c[1]) * lam + (c[4] * c[3]) * jl + gx
    return param_grads(ctrl, coef[:, 0].contiguous(), sess.arrays(), N, B, params)


def kl_grads_stepwise(loss, ctrl, params, ran, xs, z, w, lam):
    """Every other control / target / reference: one torch vector-Jacobian product of the kernel's own step per SDE step (FORM_LIN / FORM_EM
    with the host's per-step coefficients, include/sdeng.h), the HIP states as constants."""
    coef, lin, ito, reference_ctrl = ran.coef, ran.decl.lin, ran.decl.ito, ran.decl.ref_ctrl
    grads = [torch.zeros_like(p) for p in params]

    def step(lam_in, x_in, z_in, c, w_in):
        with torch.enable_grad():
            xk = x_in.detach().requires_grad_(True)
            u = ctrl(c[0], xk)
            ref = reference_ctrl(c[0], xk) if reference_ctrl is not None else None
            uu, uz = (u * u).sum(-1, keepdim=True), (u * z_in).sum(-1, keepdim=True)
            if lin:   # x' = c1 x + c2 (u [+ ref]) + c3 z ;  rnd += c4 <u,u> + c5 <u,z>
                x_next = c[1] * xk + c[2] * (u if ref is None else ref + u) + c[3] * z_in
                dr = c[4] * uu + (c[5] * uz if ito else 0.0)
            else:     # x' = x + ((c1 x [+ c3 ref]) + c2 u) c4 + c2 (c5 z) ;  rnd += 0.5 <u,u> c4 + c5 <u,z>
                drift = c[1] * xk if ref is None else c[1] * xk + c[3] * ref
                x_next = xk + (drift + c[2] * u) * c[4] + c[2] * (c[5] * z_in)
                dr = 0.5 * uu * c[4] + (c[5] * uz if ito else 0.0)
            got = torch.autograd.grad((lam_in * x_next).sum() + (w_in * dr).sum(), [xk] + params, allow_unused=True)
        for acc, gk in zip(grads, got[1:]):
            if gk is not None:
                acc.add_(gk)
        return got[0]

    N, B, d = xs.shape[0] - 1, xs.shape[1], xs.shape[2]
    key = ("kl", id(ctrl), id(getattr(reference_ctrl, "__self__", reference_ctrl)), B, d, bool(lin), bool(ito), str(xs.device))
    return walk_adjoint(loss, key, step, grads, lam, lambda k: (xs[k], z[k], coef[k], w), N, loss.graph_adjoint and R.graph_capturable(ctrl))


def _graphed_step(loss, key, step, grads, example):
    """``step`` captured as a hipGraph with static inputs / outputs (torch.cuda.graphs), cached on the loss per key; None if capture is not
    possible (the caller then runs the step eagerly)."""
    import weakref
    cache = loss.__dict__.setdefault("_step_graphs", {})
    ctrl_now = loss.generative_ctrl
    hit = cache.get(key)
    if hit is not None and hit is not False and hit.owner() is not ctrl_now:
        hit = None  # (another control object at a recycled id: the captured graph reads the old one's parameters)
    if hit is None:
        try:
            hit = _GraphedAdjointStep(step, grads, example)
            hit.owner = weakref.ref(ctrl_now)
        except Exception as e:  # noqa: BLE001 -- capture is an optimisation: run the steps eagerly, say so once
            import warnings
            warnings.warn(f"KL training: graph capture of the adjoint step failed ({type(e).__name__}: {e}); running it eagerly")
            hit = False
        cache[key] = hit
    if hit is False:
        return None
    hit.reset()
    return hit


class _GraphedAdjointStep:
    """One adjoint step (forward of the step's formulas + torch.autograd.grad) captured as a hipGraph.  The step function closes over
    per-call tensors (the accumulators); the captured graph keeps its own static accumulators and inputs, refreshed per call."""

    def __init__(self, step, grads, example):
        self.static_in = [t.detach().clone() for t in example]
        self.grads = [torch.zeros_like(g) for g in grads]
        grads_backup = [g.clone() for g in grads]
        self._swap(grads, self.grads)  # the closure accumulates into `grads`: make those our static buffers during warm-up / capture
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step(*self.static_in)
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_out = step(*self.static_in)
        finally:  # whatever happened, the caller's accumulators get their own storage and their values back
            torch.cuda.synchronize()
            self._unswap(grads, grads_backup)

    def _swap(self, grads, mine):
        self._held = [g.data for g in grads]
        for g, m in zip(grads, mine):
            g.data = m.data

    def _unswap(self, grads, backup):
        for g, h, b in zip(grads, self._held, backup):
            g.data = h
            g.copy_(b)

    def reset(self):
        for g in self.grads:
            g.zero_()

    def __call__(self, *inputs):
        for s, i in zip(self.static_in, inputs):
            s.copy_(i)
        self.graph.replay()
        return self.static_out
