"""Log-variance training direction: the HIP step loop + one batched autograd pass of the control must
reproduce the reference's loss value and its gradient w.r.t. every drift-net parameter (fixtures generated from the real
reference by tests/golden/gen_golden.py, same counter-based noise)."""
import pytest
import torch

from sde_sampler_lrds_amd import _lib as L
from sde_sampler_lrds_amd import engine as E
from tests import build_cases as bc
from tests import golden_cases as gc


KINDS = {"train_lv": "rds_gmm", "train_lv_dis": "dis_ei", "train_lv_dis_orig": "dis_orig", "train_lv_dds": "dds", "train_lv_pis": "pis_phi4", "train_lv_cmcd": "cmcd_gmm"}  # objects as in the simulate cases


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["train_lv_ei_gmm_d16", "train_lv_em_gmm_d16", "train_lv_dis_ei_d8", "train_lv_dds_d2", "train_lv_pis_phi4_d100", "train_lv_dis_orig_d8", "train_lv_cmcd_gmm_d16"])
def test_lv_training_loss_and_gradients_match_reference(gpu, name):
    c = gc.load(name)
    c.meta["kind"] = KINDS[c.meta["kind"]]
    b = bc.build(c, gpu)
    loss = b["loss"]
    loss.method = "lv"
    ctrl = loss.generative_ctrl
    for p in ctrl.parameters():
        p.grad = None
    kw = {k: v for k, v in b["kwargs"].items() if k == "initial_log_prob"}
    value, metrics = loss(b["ts"], b["x0"], *b["args"], **kw)
    value.backward()
    # tolerances = 10 x the worst achieved over the seven fixtures on MI355X (loss value 1.2e-6 relative, gradients 5.0e-6 of the largest entry)
    loss_err = abs(float(value.detach()) - c.meta["loss"]) / max(1.0, abs(c.meta["loss"]))
    assert loss_err < 1e-5, (float(value.detach()), c.meta["loss"])
    worst = 0.0
    for k, p in ctrl.named_parameters():
        if "grad." + k not in c.a:
            continue
        ref = c["grad." + k]
        err = float((p.grad.cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
        worst = max(worst, err)
        assert err < 5e-5, (k, err)
    print(f"{name}: loss {float(value.detach()):.6f} vs {c.meta['loss']:.6f} (rel {loss_err:.1e}); worst relative gradient error {worst:.2e}")
    assert "train/n_filtered_cumulative" in metrics


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["train_kl_dds_d2", "train_kl_ei_gmm_d16", "train_kl_em_gmm_d16", "train_kl_dis_ei_d8", "train_kl_dis_orig_d8",
                                  "train_kl_pis_phi4_d100", "train_kl_cmcd_gmm_d16"])
def test_kl_training_loss_and_gradients_match_reference(gpu, name):
    """method='kl' -- BaseOCLoss's default, BASELINE cfg 1's loss: back-propagation through the whole trajectory (losses/oc.py:105-131).
    Fixtures: the reference's own ``loss(...)`` + ``backward()`` under the replayed noise.  Here: the HIP trajectory + the discrete
    adjoint (BaseOCLoss._kl_loss)."""
    c = gc.load(name)
    assert c.meta["method"] == "kl"
    c.meta["kind"] = KINDS[c.meta["kind"]]
    b = bc.build(c, gpu)
    loss = b["loss"]
    loss.method, loss.max_rnd = "kl", None
    ctrl = loss.generative_ctrl
    for p in ctrl.parameters():
        p.grad = None
    kw = {k: v for k, v in b["kwargs"].items() if k == "initial_log_prob"}
    value, metrics = loss(b["ts"], b["x0"], *b["args"], **kw)
    value.backward()
    loss_err = abs(float(value.detach()) - c.meta["loss"]) / max(1.0, abs(c.meta["loss"]))
    worst, n = 0.0, 0
    for k, p in ctrl.named_parameters():
        if "grad." + k not in c.a:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        ref = c["grad." + k]
        err = float((p.grad.cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
        worst, n = max(worst, err), n + 1
    # tolerance: 5e-5 (10 x the worst achieved on the well-conditioned fixtures), or 10 x the fixture's own conditioning -- how far the
    # REFERENCE's gradient moves when every normal is perturbed by 1.2e-6, recorded by gen_golden.py (train_kl_dds_d2: 1.0e-4, the
    # sharp TwoModes target; the others ~1e-6)
    tol = max(5e-5, 10 * c.meta.get("grad_sensitivity", 0.0))
    print(f"{name}: loss {float(value.detach()):.6f} vs {c.meta['loss']:.6f} (rel {loss_err:.1e}); worst relative gradient error {worst:.2e} over {n} "
          f"parameters (tolerance {tol:.1e}; reference's own sensitivity {c.meta.get('grad_sensitivity', 0.0):.1e})")
    assert n >= 8 and loss_err < 1e-5 and worst < tol
    assert "train/n_filtered_cumulative" in metrics


@pytest.mark.gpu
def test_sde_ctrl_noise_is_refused_in_training(gpu):
    """What the training direction still refuses: a perturbed simulated control (sde_ctrl_noise / sde_ctrl_dropout, losses/oc.py:97-101)."""
    c = gc.load("train_lv_cmcd_gmm_d16")
    c.meta["kind"] = KINDS[c.meta["kind"]]
    b = bc.build(c, gpu)
    b["loss"].sde_ctrl_noise = 0.1
    for method in ("lv", "kl"):
        b["loss"].method = method
        with pytest.raises(E.UnsupportedByEngine):
            b["loss"](b["ts"], b["x0"], *b["args"], initial_log_prob=b["kwargs"]["initial_log_prob"])


@pytest.mark.gpu
def test_training_steps_reduce_the_loss(gpu):
    """make_model -> TrainableWrapper.run(): a few hundred Adam steps of log-variance training on a small mixture."""
    from sde_sampler_lrds_amd.additions.hacking import TrainableWrapper
    from sde_sampler_lrds_amd.experiments.benchmark_utils import make_model, make_target_details
    tgt = make_target_details("many_modes", dim=8, n_modes=4)
    K, d = 4, 8
    model = make_model("vp-ref", "default", "lv", "ei", "base_zero_init", "uniform", dict(sigma=2.0), tgt,
                       dict(train_steps=150, train_batch_size=512, eval_batch_size=2048), optim_details=dict(lr=3e-3), n_steps=32)
    before = model.evaluate().metrics["eval/lv_loss"]
    res, train = TrainableWrapper(model, verbose=False).run(keep_training_metrics=True)
    after = res.metrics["eval/lv_loss"]
    print(f"eval/lv_loss {before:.3f} -> {after:.3f} after {len(train['train/loss'])} steps; eubo {res.metrics.get('eval/eubo')}")
    assert len(train["train/loss"]) == 150 and after < 0.7 * before


@pytest.mark.gpu
def test_ema_weights_are_used_for_evaluation(gpu):
    from sde_sampler_lrds_amd.experiments.benchmark_utils import make_model, make_target_details
    tgt = make_target_details("many_modes", dim=8, n_modes=4)
    model = make_model("vp-ref", "default", "lv", "ei", "base_zero_init", "uniform", dict(sigma=2.0), tgt,
                       dict(train_steps=20, train_batch_size=256, eval_batch_size=512), optim_details=dict(lr=3e-3), n_steps=16, use_ema=True)
    assert type(model.generative_ctrl_ema).__name__ == "AveragedModel"
    model.run()
    w, w_ema = model.generative_ctrl.base_model.out_layer.weight, model.generative_ctrl_ema.module.base_model.out_layer.weight
    assert not torch.equal(w, w_ema) and int(model.generative_ctrl_ema.n_averaged) >= 2
    a = model.evaluate(use_ema=True).metrics["eval/elbo"]
    b = model.evaluate(use_ema=False).metrics["eval/elbo"]
    assert a != b  # the EMA copy and the live net drive different samplers


@pytest.mark.gpu
@pytest.mark.parametrize("d,N,B,clip", [(128, 7, 37, 1e4), (100, 5, 64, 0.05), (16, 9, 20, None), (2, 3, 5, 1e4), (61, 4, 48, 0.03)])
def test_fused_forward_backward_of_the_drift_net_matches_autograd(gpu, d, N, B, clip):
    """sdeng_ctrl_vjp (csrc/grad_kernel.hpp): per-row activations / cotangents of the drift net, the six parameter-gradient products built
    from them and the state gradient, against torch autograd of the same ClippedCtrl in fp64.  Rows per time not a multiple of the
    16-row tile, an ACTIVE clip (its mask must gate the cotangent exactly like torch.clip's backward), small cotangents (1e-6)."""
    import copy

    from sde_sampler_lrds_amd.experiments import baseline_configs as cfgs
    from sde_sampler_lrds_amd.models.reparam import ClippedCtrl
    torch.manual_seed(d + N)
    ctrl = ClippedCtrl(base_model=cfgs._net(d), clip_model=clip).to(gpu)
    ts = torch.linspace(0.05, 0.9, N, device=gpu)
    xs = 1.5 * torch.randn(N, B, d, device=gpu)
    cot = 1e-6 * torch.randn(N, B, d, device=gpu) * (1.0 + 10.0 * torch.rand(N, B, 1, device=gpu))
    r = E.ctrl_vjp(ctrl, ts, xs, cot, want_gx=True)
    net = ctrl.base_model
    got = {"out_layer.weight": r["dout"].t() @ r["a2"], "out_layer.bias": r["dout"].sum(0), "hidden_layer.1.weight": r["d2"].t() @ r["a1"],
           "hidden_layer.1.bias": r["d2"].sum(0), "hidden_layer.0.weight": r["d1"].t() @ r["a0"], "hidden_layer.0.bias": r["d1"].sum(0),
           "input_embed.weight": r["d0"].t() @ r["x"], "input_embed.bias": r["d0"].sum(0)}
    # fp64 autograd of the same module
    c64 = copy.deepcopy(ctrl).double()
    x64 = xs.double().requires_grad_(True)
    u = torch.stack([c64(ts[k].double(), x64[k]) for k in range(N)])
    (u * cot.double()).sum().backward()
    worst = 0.0
    for k, v in got.items():
        ref = dict(c64.base_model.named_parameters())[k].grad
        err = float((v.double() - ref).abs().max() / ref.abs().max().clamp(min=1e-30))
        worst = max(worst, err)
        assert err < 2e-5, (k, err)
    egx = float((r["gx"].view(N, B, d).double() - x64.grad).abs().max() / x64.grad.abs().max())
    with torch.no_grad():  # outputs of the un-clipped net beyond the clip: where torch.clip's backward blocks the cotangent
        n_clipped = int(sum((c64.base_model(ts[k].double(), x64[k]).abs() > clip).sum() for k in range(N))) if clip else 0
    print(f"ctrl_vjp d={d} N={N} B={B} clip={clip}: worst parameter-gradient error {worst:.2e}, state gradient {egx:.2e} (vs fp64 autograd; {n_clipped} clipped outputs)")
    assert egx < 2e-5
    if clip is not None and clip < 1.0:
        assert n_clipped > 0


@pytest.mark.gpu
@pytest.mark.parametrize("d,K,lin,ito,N,B,clip,score", [
    (5, 0, True, True, 6, 37, 1e4, None), (16, 1, False, True, 9, 20, 1e4, None), (40, 3, True, False, 5, 64, 0.05, None),
    (128, 4, True, True, 7, 37, 1e4, None), (100, 2, False, True, 4, 48, 1e4, None),
    # ScoreCtrl on a diagonal mixture target (BASELINE config 1 is DDS on TwoModes d=2): (components, detach_score, clip_score)
    (2, 0, True, True, 8, 50, 1e4, (2, False, 1e4)), (16, 0, False, True, 6, 33, 1e4, (3, False, 2.0)), (8, 2, True, True, 5, 40, 1e4, (4, True, 1e4)),
    (128, 0, True, True, 4, 24, 1e4, (2, False, 1e4)),
    # ScoreCtrl on the phi^4 lattice (BASELINE config 3 is PIS on PhiFour d=100): tridiagonal Hessian, neighbours across lanes and tiles
    (100, 0, False, True, 5, 24, 1e4, ("phi4", False, 1e4)), (36, 0, False, False, 6, 40, 1e4, ("phi4", False, 30.0)), (17, 0, True, True, 4, 20, 1e4, ("phi4", True, 1e4))])
def test_native_kl_adjoint_matches_autograd(gpu, d, K, lin, ito, N, B, clip, score):
    """sdeng_kl_adjoint (csrc/grad_kernel.hpp k_kl_adjoint): the whole adjoint recursion of KL training in one launch -- lambda_0 and every
    parameter gradient against fp64 torch autograd of the same recursion (one step at a time, the control and the noised reference score
    as torch expressions).  K = 0: no reference drift; K = 1: Gaussian; K > 1: diagonal mixture (closed-form Hessian-vector product).
    The bound: 2e-5, or 6 x what the SAME recursion in fp32 torch autograd differs from fp64 by (the recursion amplifies round-off)."""
    import copy

    from sde_sampler_lrds_amd.distr.gauss import GMM, score_mog
    from sde_sampler_lrds_amd.distr.phi_four import PhiFour
    from sde_sampler_lrds_amd.experiments import baseline_configs as cfgs
    from sde_sampler_lrds_amd.losses.oc import vjp_param_grads
    from sde_sampler_lrds_amd.models.mlp import TimeEmbed
    from sde_sampler_lrds_amd.models.reparam import ClippedCtrl, ScoreCtrl
    torch.manual_seed(3 * d + K)
    tgt_par = None
    if score is None:
        ctrl = ClippedCtrl(base_model=cfgs._net(d), clip_model=clip).to(gpu)
    else:
        Kt, detach, clip_score = score
        if Kt == "phi4":
            target = PhiFour(a=0.1, b=0.05, dim=d, beta=20.0).to(gpu)
        else:
            tgt_par = dict(loc=1.5 * torch.randn(Kt, d), scale=0.5 + torch.rand(Kt, d), mixture_weights=0.5 + torch.rand(Kt))
            target = GMM(dim=d, **{k: v.clone() for k, v in tgt_par.items()}).to(gpu)
        sm = TimeEmbed(dim_out=1, activation=torch.nn.GELU(), num_layers=4, channels=64)
        torch.nn.init.normal_(sm.out_layer.weight, std=0.1)
        torch.nn.init.constant_(sm.out_layer.bias, 0.3)
        ctrl = ScoreCtrl(base_model=cfgs._net(d), score_model=sm, target_score=target.score, detach_score=detach, clip_score=clip_score,
                         clip_model=clip, scale_score=0.7).to(gpu)
    coef = torch.zeros(N, L.NCOEF, device=gpu)
    coef[:, 0] = torch.linspace(0.9, 0.1, N)
    coef[:, 1] = (0.9 + 0.2 * torch.rand(N)) if lin else -0.5 * torch.rand(N)
    coef[:, 2] = 0.3 + 0.5 * torch.rand(N)
    coef[:, 3] = 0.2 + 0.3 * torch.rand(N)
    coef[:, 4] = 0.05 + 0.1 * torch.rand(N)
    coef[:, 5] = 0.2 + 0.2 * torch.rand(N)
    coef[:, 9], coef[:, 10], coef[:, 11] = 0.5 + 0.5 * torch.rand(N), 0.1 + 0.5 * torch.rand(N), 0.3 + 0.6 * torch.rand(N)
    xs = 1.2 * torch.randn(N, B, d, device=gpu)
    z = torch.randn(N, B, d, device=gpu)
    w = torch.rand(B, 1, device=gpu) / B
    w[::5] = 0.0  # filtered particles
    lam_n = 0.1 * torch.randn(B, d, device=gpu)
    ref = ("none", {})
    if K == 1:
        ref = ("gaussian", dict(x_init=torch.randn(d, device=gpu), var_init=0.5 + torch.rand(d, device=gpu)))
    elif K > 1:
        ref = ("gmm", dict(means_init=1.5 * torch.randn(K, d, device=gpu), variances_init=0.4 + torch.rand(K, d, device=gpu), weights_init=0.5 + torch.rand(K, device=gpu)))
    arrays, lam0 = E.kl_adjoint(ctrl, coef, xs, z, w, lam_n, lin=lin, ito=ito, ref=ref)
    arrays2, lam0_again = E.kl_adjoint(ctrl, coef, xs, z, w, lam_n, lin=lin, ito=ito, ref=ref)
    assert torch.equal(lam0, lam0_again) and torch.equal(arrays["d0"], arrays2["d0"]) and torch.equal(arrays["dout"], arrays2["dout"]), "rerun differs"
    found = vjp_param_grads(ctrl, coef[:, 0].contiguous(), arrays, N, B)
    if score is not None:
        sm_params = list(ctrl.score_model.parameters())
        st = ctrl.clipped_score_model(coef[:, 0].contiguous().view(-1, 1), None).view(N)
        found.update(dict(zip(sm_params, torch.autograd.grad(st, sm_params, grad_outputs=arrays["dst"].sum(1)))))

    def recursion(dtype):  # torch autograd of the same recursion, one step at a time
        if score is None:
            cc = copy.deepcopy(ctrl).to(dtype)
        else:
            if score[0] == "phi4":
                t2 = PhiFour(a=0.1, b=0.05, dim=d, beta=20.0).to(gpu).to(dtype)
            else:
                t2 = GMM(dim=d, **{k: v.clone().to(dtype) for k, v in tgt_par.items()}).to(gpu).to(dtype)
            cc = ScoreCtrl(base_model=copy.deepcopy(ctrl.base_model).to(dtype), score_model=copy.deepcopy(ctrl.score_model).to(dtype), target_score=t2.score,
                           detach_score=ctrl.detach_score, clip_score=ctrl.clip_score, clip_model=ctrl.clip_model, scale_score=ctrl.scale_score)
        params = list(cc.parameters())
        grads = [torch.zeros_like(p) for p in params]
        lam, c_, wd = lam_n.to(dtype), coef.to(dtype), w.to(dtype)
        for k in range(N - 1, -1, -1):
            c = c_[k]
            xk = xs[k].to(dtype).requires_grad_(True)
            u = cc(c[0], xk)
            rf = None
            if K == 1:
                rf = -(xk - c[9] * ref[1]["x_init"].to(dtype)) / (c[10] + c[11] * ref[1]["var_init"].to(dtype))
            elif K > 1:
                rf = score_mog(xk, ref[1]["weights_init"].to(dtype), c[9] * ref[1]["means_init"].to(dtype), c[10] + c[11] * ref[1]["variances_init"].to(dtype))
            zk = z[k].to(dtype)
            uu, uz = (u * u).sum(-1, keepdim=True), (u * zk).sum(-1, keepdim=True)
            if lin:
                x_next = c[1] * xk + c[2] * (u if rf is None else rf + u) + c[3] * zk
                dr = c[4] * uu + (c[5] * uz if ito else 0.0)
            else:
                drift = c[1] * xk if rf is None else c[1] * xk + c[3] * rf
                x_next = xk + (drift + c[2] * u) * c[4] + c[2] * (c[5] * zk)
                dr = 0.5 * uu * c[4] + (c[5] * uz if ito else 0.0)
            got = torch.autograd.grad((lam * x_next).sum() + (wd * dr).sum(), [xk] + params, allow_unused=True)
            lam = got[0]
            for acc, gk in zip(grads, got[1:]):
                if gk is not None:
                    acc += gk
        return lam, dict(zip([n for n, _ in cc.named_parameters()], grads))

    lam64, g64 = recursion(torch.float64)
    lam32, g32 = recursion(torch.float32)
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max().clamp(min=1e-30))  # noqa: E731
    e_lam, t_lam = rel(lam0, lam64), rel(lam32, lam64)
    worst, t_worst = 0.0, 0.0
    for name, p in ctrl.named_parameters():
        if p not in found:
            assert float(g64[name].abs().max()) == 0.0, name
            continue
        worst, t_worst = max(worst, rel(found[p], g64[name])), max(t_worst, rel(g32[name], g64[name]))
    print(f"kl_adjoint d={d} K={K} {'LIN' if lin else 'EM'} ito={ito} N={N} B={B} clip={clip} score={score}: lambda_0 error {e_lam:.2e} (fp32 torch autograd: "
          f"{t_lam:.2e}), worst parameter-gradient error {worst:.2e} (fp32 torch: {t_worst:.2e}), vs fp64 autograd")
    assert e_lam < max(2e-5, 6 * t_lam) and worst < max(2e-5, 6 * t_worst)


@pytest.mark.gpu
def test_kl_training_native_adjoint_equals_the_stepwise_one(gpu):
    """The one-launch adjoint and the step-by-step one (sdeng_ctrl_vjp per step + torch VJP of the reference score) give the same gradients."""
    c = gc.load("train_kl_ei_gmm_d16")
    c.meta["kind"] = KINDS["train_lv"]
    out = {}
    for native in (True, False):
        b = bc.build(c, gpu)
        loss = b["loss"]
        loss.method, loss.native_adjoint = "kl", native
        loss.seed = c.meta["seed"]
        value, _ = loss(b["ts"], b["x0"], *b["args"])
        value.backward()
        assert loss.last_adjoint_path == ("native" if native else "fused")  # (a ClippedCtrl: its per-step form is one sdeng_ctrl_vjp per step)
        out[native] = (float(value.detach()), {k: p.grad.clone() for k, p in loss.generative_ctrl.named_parameters() if p.grad is not None})
    assert out[True][0] == out[False][0]
    worst = max(float((out[True][1][k] - g).abs().max() / g.abs().max().clamp(min=1e-30)) for k, g in out[False][1].items())
    print(f"native vs stepwise adjoint: worst relative gradient difference {worst:.2e}")
    assert worst < 1e-5


@pytest.mark.gpu
def test_the_three_kl_adjoints_run_and_agree(gpu):
    """One fixture through each adjoint of BaseOCLoss._kl_loss -- the one-launch kernel, one sdeng_ctrl_vjp per step, one torch
    vector-Jacobian product per step (a ClippedCtrl reaches the last only with fused_training off) -- from the fixture's seed: the call says
    which one ran, the value (the same step-loop launch) is equal bit for bit, and every gradient set meets the bound
    test_kl_training_loss_and_gradients_match_reference holds this fixture to against the reference's ``backward()``."""
    c = gc.load("train_kl_ei_gmm_d16")
    c.meta["kind"] = KINDS["train_lv"]
    tol = max(5e-5, 10 * c.meta.get("grad_sensitivity", 0.0))
    values = []
    for native, fused, path in ((True, True, "native"), (False, True, "fused"), (False, False, "stepwise")):
        b = bc.build(c, gpu)
        loss = b["loss"]
        loss.method, loss.max_rnd, loss.native_adjoint, loss.fused_training = "kl", None, native, fused
        loss.seed = c.meta["seed"]
        value, _ = loss(b["ts"], b["x0"], *b["args"])
        value.backward()
        assert loss.last_adjoint_path == path
        values.append(float(value.detach()))
        worst, n = 0.0, 0
        for k, p in loss.generative_ctrl.named_parameters():
            if "grad." + k not in c.a:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, (path, k)
                continue
            ref = c["grad." + k]
            worst, n = max(worst, float((p.grad.cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)), n + 1
        print(f"train_kl_ei_gmm_d16 through the {path} adjoint: worst relative gradient error {worst:.2e} over {n} parameters (tolerance {tol:.1e})")
        assert n >= 8 and worst < tol, path
    assert abs(values[0] - c.meta["loss"]) / max(1.0, abs(c.meta["loss"])) < 1e-5
    assert values[0] == values[1] == values[2]


@pytest.mark.gpu
@pytest.mark.parametrize("solver,ref,integ,mtype,details,ctrl_name", [
    ("dis_orig", "default", "em", "target_informed_lerp_tempering", dict(sigma=1.0), "LerpCtrl"),
    ("dis_orig", "default", "em", "target_informed_langevin_init", dict(sigma=1.0), "CancelDriftCtrl"),
    ("pis_orig", "default", "em", "target_informed_zero_init", dict(sigma=0.4472135954999579), "ScoreCtrl"),
    ("vp-ref", "default", "ei", "base_zero_init", dict(sigma=1.5), "ClippedCtrl"),
    ("vp-ref", "gmm", "em", "base_zero_init", dict(means_ref=torch.tensor([[1.0] * 8, [-1.0] * 8]), variances_ref=0.5 * torch.ones(2, 8), weights_ref=torch.ones(2)), "ClippedCtrl")])
def test_native_adjoint_equals_stepwise_for_every_control(gpu, solver, ref, integ, mtype, details, ctrl_name):
    """make_model(...) with method='kl' for each control wrapper / reference kind the one-launch adjoint covers: same loss value, and every
    gradient equal to the step-by-step adjoint's (torch vector-Jacobian products of the module itself, i.e. of the reference's formulas)."""
    from sde_sampler_lrds_amd.experiments.benchmark_utils import make_model, make_target_details
    tgt = make_target_details("many_modes", dim=8, n_modes=4)
    out = {}
    for native in (True, False):
        torch.manual_seed(0)
        model = make_model(solver, ref, "kl", integ, mtype, "uniform", details, tgt, dict(train_steps=2, train_batch_size=300, eval_batch_size=300),
                           optim_details=dict(lr=1e-3), n_steps=24)
        ctrl = model.loss.generative_ctrl
        assert type(ctrl).__name__ == ctrl_name and E.adjoint_ctrl_ok(ctrl)
        with torch.no_grad():
            g = torch.Generator(device="cpu").manual_seed(1)
            ctrl.base_model.out_layer.weight.copy_(0.05 * torch.randn(ctrl.base_model.out_layer.weight.shape, generator=g))
        model.loss.native_adjoint = native
        model.setup_optim()
        loss, _ = model.compute_loss()
        loss.backward()
        assert model.loss.last_adjoint_path == ("native" if native else ("fused" if ctrl_name == "ClippedCtrl" else "stepwise"))
        out[native] = (float(loss.detach()), {k: p.grad.clone() for k, p in ctrl.named_parameters() if p.grad is not None})
    assert out[True][0] == out[False][0] and out[True][1].keys() == out[False][1].keys()
    worst = max(float((out[True][1][k] - g).abs().max() / g.abs().max().clamp(min=1e-30)) for k, g in out[False][1].items())
    print(f"{solver} / {ctrl_name}: native vs stepwise adjoint, worst relative gradient difference {worst:.2e} over {len(out[False][1])} parameters")
    assert worst < 2e-5


@pytest.mark.gpu
def test_kl_training_at_baseline_config_1_size(gpu):
    """BASELINE config 1 as the reference runs it (DDS on TwoModes d=2, KL loss, 4 096 particles x 64 steps, cosine time grid): the one-launch
    adjoint against the step-by-step one (torch vector-Jacobian products of the whole ScoreCtrl) on the SAME trajectory -- every gradient --
    and two consecutive training calls must differ (fresh x0 / noise per call)."""
    from sde_sampler_lrds_amd.experiments.benchmark_utils import make_model, make_target_details
    tgt = make_target_details("two_modes", dim=2)
    grads = {}
    for native in (True, False):
        torch.manual_seed(0)
        model = make_model("dds_orig", "default", "kl", "em", "target_informed_zero_init", "uniform", dict(sigma=1.0), tgt,
                           dict(train_steps=2, train_batch_size=4096, eval_batch_size=4096), optim_details=dict(lr=1e-3), n_steps=64)
        with torch.no_grad():  # a drift net that does something (make_model zero-initialises the last layer)
            g = torch.Generator(device="cpu").manual_seed(1)
            model.generative_ctrl.base_model.out_layer.weight.copy_(0.05 * torch.randn(model.generative_ctrl.base_model.out_layer.weight.shape, generator=g))
        model.loss.native_adjoint = native
        model.setup_optim()
        loss, _ = model.compute_loss()
        loss.backward()
        assert model.loss.last_adjoint_path == ("native" if native else "stepwise")
        grads[native] = (float(loss.detach()), {k: p.grad.clone() for k, p in model.generative_ctrl.named_parameters() if p.grad is not None})
    assert grads[True][0] == grads[False][0]
    worst = max(float((grads[True][1][k] - g).abs().max() / g.abs().max().clamp(min=1e-30)) for k, g in grads[False][1].items())
    print(f"cfg 1 size: native vs stepwise adjoint, worst relative gradient difference {worst:.2e} over {len(grads[False][1])} parameters")
    assert len(grads[False][1]) >= 20 and worst < 2e-4  # (the reference's own conditioning on this target: 1e-4, fixture train_kl_dds_d2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pis_logreg_d61", "dds_logreg_d61"])
def test_native_adjoint_on_logistic_regression_targets(gpu, name):
    """PIS / DDS on a Bayesian logistic-regression target with method='kl': the reference's LogisticRegression.score is autograd-made without a
    graph (distr/base.py:146-154), so back-propagation sees it as a constant of x -- the one-launch adjoint takes the scores of all rows from
    the HIP score kernel as an input (ADJ_EXT) and must give the step-by-step adjoint's gradients (torch VJPs of the module itself)."""
    c = gc.load(name)
    out = {}
    for native in (True, False):
        b = bc.build(c, gpu)
        loss = b["loss"]
        loss.method, loss.max_rnd, loss.native_adjoint = "kl", None, native
        loss.seed = c.meta["seed"]
        assert E.adjoint_ctrl_ok(loss.generative_ctrl)
        kw = {k: v for k, v in b["kwargs"].items() if k == "initial_log_prob"}
        value, _ = loss(b["ts"], b["x0"], *b["args"], **kw)
        value.backward()
        assert loss.last_adjoint_path == ("native" if native else "stepwise")
        out[native] = (float(value.detach()), {k: p.grad.clone() for k, p in loss.generative_ctrl.named_parameters() if p.grad is not None})
    assert out[True][0] == out[False][0] and out[True][1].keys() == out[False][1].keys()
    worst = max(float((out[True][1][k] - g).abs().max() / g.abs().max().clamp(min=1e-30)) for k, g in out[False][1].items())
    print(f"{name}: native (external score) vs stepwise adjoint, worst relative gradient difference {worst:.2e} over {len(out[False][1])} parameters")
    assert len(out[False][1]) >= 20 and worst < 2e-5
