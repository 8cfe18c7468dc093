"""Sinkhorn and MMD kernels against the reference's own results (tests/golden/gen_golden_metrics.py), through the C ABI.

Tolerance: |hip - ref64| / ref64 <= 4 F, where ref64 is the reference on the float64 cast of the stored inputs and F the largest
relative |ref32 - ref64| over all stored cases of that metric -- the reference's own float32 noise (metrics_summary.json).  The factor
4 allows for a summation order that differs from both reference runs.  The achieved errors are printed (profiles/metrics_parity.log)."""
import json
import os

import numpy as np
import pytest
import torch

from sde_sampler_lrds_amd import engine as E
from sde_sampler_lrds_amd.additions.ks import compute_sliced_ks
from sde_sampler_lrds_amd.additions.mmd import mmd_median
from sde_sampler_lrds_amd.eval.sinkhorn import Sinkhorn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUMMARY = json.load(open(os.path.join(GOLDEN, "metrics_summary.json")))
F_SINKHORN, F_MMD = SUMMARY["sinkhorn"]["F"], SUMMARY["mmd"]["F"]
SINKHORN_CASES = sorted(SUMMARY["sinkhorn"]["rel_ref32_vs_ref64"])
MMD_CASES = sorted(SUMMARY["mmd"]["rel_ref32_vs_ref64"])


def _case(name, dev):
    c = np.load(os.path.join(GOLDEN, f"metrics_{name}.npz"))
    t = lambda k: torch.from_numpy(c[k]).to(dev) if k in c.files else None
    return c, t("x"), t("y"), t("w_x"), t("w_y")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SINKHORN_CASES)
def test_sinkhorn_matches_reference(gpu, name):
    c, x, y, wx, wy = _case(name, gpu)
    kw = dict(p=int(c["p"]), eps=float(c["eps"]))
    ref64, it64 = float(c["sinkhorn_ref64"]), int(c["sinkhorn_iters64"])
    out = E.sinkhorn(x, y, wx, wy, **kw)
    out_re = E.sinkhorn(x, y, wx, wy, materialise=False, **kw)  # every pass recomputes the costs: same arithmetic, same result
    rel = abs(out["distance"].double().item() - ref64) / ref64
    print(f"sinkhorn {name}: n={x.shape[0]} m={y.shape[0]} d={x.shape[1]} hip {out['distance'].item():.8g} ref64 {ref64:.8g} "
          f"rel {rel:.2e} (ref32 rel {abs(float(c['sinkhorn_ref32']) - ref64) / ref64:.2e}; bound {4 * F_SINKHORN:.2e}) "
          f"iters {out['iters']} (ref64 {it64}, ref32 {int(c['sinkhorn_iters32'])}) max change {max(out['max_err_u'], out['max_err_v']):.2e}")
    assert out["materialised"] and not out_re["materialised"]
    assert rel <= 4 * F_SINKHORN
    assert abs(out["iters"] - it64) <= (1 if name == "d2_eps_large" else 0)
    for key in ("distance", "u", "v", "corr_x_to_y", "corr_y_to_x"):
        assert torch.equal(out[key], out_re[key]), key
    assert out["iters"] == out_re["iters"]
    assert out["u"].shape == (x.shape[0],) and out["v"].shape == (y.shape[0],)
    assert out["corr_x_to_y"].shape == (x.shape[0],) and int(out["corr_x_to_y"].max()) < y.shape[0]
    assert out["corr_y_to_x"].shape == (y.shape[0],) and int(out["corr_y_to_x"].max()) < x.shape[0]
    # the public class: same number, iterations recorded
    s = Sinkhorn(**kw)
    dist, c_xy, c_yx = s.compute(x, y, wx, wy)
    assert dist.item() == out["distance"].item() and s.n_iters_ == out["iters"] and torch.equal(c_xy, out["corr_x_to_y"])
    assert s(x, y, wx, wy).item() == dist.item()


@pytest.mark.gpu
def test_sinkhorn_correspondences_on_a_permuted_copy(gpu):
    c = np.load(os.path.join(GOLDEN, "metrics_perm.npz"))
    x, y = torch.from_numpy(c["x"]).to(gpu), torch.from_numpy(c["y"]).to(gpu)
    _, c_xy, c_yx = Sinkhorn().compute(x, y)
    wrong = int((c_xy.cpu() != torch.from_numpy(c["corr_x_to_y"])).sum()) + int((c_yx.cpu() != torch.from_numpy(c["corr_y_to_x"])).sum())
    print(f"sinkhorn permuted copy: {wrong} of {2 * x.shape[0]} correspondences differ from the permutation")
    assert c_xy.dtype == torch.int64 and wrong == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", MMD_CASES)
def test_mmd_median_matches_reference(gpu, name):
    c, x, y, _, _ = _case(name, gpu)
    ref64 = float(c["mmd_ref64"])
    mmd, bw = E.mmd_median(x, y)
    rel = abs(mmd.double().item() - ref64) / ref64
    # the bandwidth: exactly the lower median (torch.median) of the fp32 distances the kernel sees
    z = torch.cat([x, y]).double()
    d2 = ((z[:, None, :] - z[None, :, :]) ** 2).sum(-1)
    iu = torch.triu_indices(z.shape[0], z.shape[0], offset=1, device=gpu)
    med = torch.median(d2[iu[0], iu[1]].float())
    print(f"mmd {name}: n={x.shape[0]} d={x.shape[1]} hip {mmd.item():.8g} ref64 {ref64:.8g} rel {rel:.2e} "
          f"(ref32 rel {abs(float(c['mmd_ref32']) - ref64) / ref64:.2e}; bound {4 * F_MMD:.2e}) bandwidth_sq {bw.item():.8g} median {med.item():.8g}")
    assert rel <= 4 * F_MMD
    assert bw.item() == med.item()
    assert mmd_median(x, y).item() == mmd.item()


@pytest.mark.gpu
def test_reruns_are_bit_identical(gpu):
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(1500, 7, generator=g).to(gpu), (torch.randn(1100, 7, generator=g) * 1.2 + 0.3).to(gpu)
    wx, wy = torch.rand(1500, generator=g).to(gpu) + 0.1, torch.rand(1100, generator=g).to(gpu) + 0.1
    wx, wy = wx / wx.sum(), wy / wy.sum()
    runs = [E.sinkhorn(x, y, wx, wy, max_iters=20) for _ in range(3)]
    for r in runs[1:]:
        for key in ("distance", "u", "v", "corr_x_to_y", "corr_y_to_x"):
            assert torch.equal(r[key], runs[0][key]), key
        assert (r["iters"], r["max_err_u"], r["max_err_v"]) == (runs[0]["iters"], runs[0]["max_err_u"], runs[0]["max_err_v"])
    m = [torch.stack(E.mmd_median(x[:1100], y)) for _ in range(3)]
    assert torch.equal(m[0], m[1]) and torch.equal(m[0], m[2])


# ---- full size: a dense float64 restatement on the GPU -----------------------------------------------------------------------------
def _dense_cost(x, y, p, rows=64):
    out = torch.empty(x.shape[0], y.shape[0], dtype=x.dtype, device=x.device)
    for i in range(0, x.shape[0], rows):
        diff = x[i:i + rows, None, :] - y[None, :, :]
        out[i:i + rows] = diff.abs().sum(-1) if p == 1 else (diff ** 2).sum(-1) ** 0.5
    return out


def _dense_sinkhorn(x, y, p=2, eps=1e-3, max_iters=100, stop_thresh=1e-5):
    """eval/sinkhorn.py:113-177 on dense tensors of x's dtype, uniform weights."""
    n, m = x.shape[0], y.shape[0]
    M = _dense_cost(x, y, p)
    w_x, w_y = torch.ones(n).to(x) / n, torch.ones(m).to(x) / m * (n / m)
    log_a, log_b = torch.log(w_x), torch.log(w_y)
    u, v = torch.zeros_like(w_x), eps * torch.log(w_y)
    iters = 0
    for _ in range(max_iters):
        u_prev, v_prev = u, v
        u = eps * (log_a - ((-M + v[None, :]) / eps).logsumexp(dim=1))
        v = eps * (log_b - ((-M + u[:, None]) / eps).logsumexp(dim=0))
        iters += 1
        if (u_prev - u).abs().max() < stop_thresh and (v_prev - v).abs().max() < stop_thresh:
            break
    P = ((-M + u[:, None] + v[None, :]) / eps).exp()
    return (P * M).sum().item(), iters


def _dense_mmd(X, Y):
    """additions/mmd.py:30-59 on dense tensors of X's dtype."""
    n = X.shape[0]

    def same(A):
        aa = A @ A.t()
        ra = aa.diag().unsqueeze(0).expand_as(aa)
        return ra.t() + ra - 2.0 * aa, ra

    d_xx, rx = same(X)
    d_yy, ry = same(Y)
    d_xy = rx.t() + ry - 2.0 * (X @ Y.t())
    iu = torch.triu_indices(n, n, offset=1, device=X.device)
    bw = torch.median(torch.cat([d_xx[iu[0], iu[1]], d_yy[iu[0], iu[1]], d_xy.flatten()]))
    k = lambda d: torch.exp(-(d / bw) / 2)
    mmd2 = (k(d_xx).sum() - n) / (n * (n - 1)) + (k(d_yy).sum() - n) / (n * (n - 1)) - 2.0 * k(d_xy).mean()
    return torch.sqrt(torch.clamp(mmd2, min=1e-20)).item()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [2, 128])
def test_full_size_against_dense_float64(gpu, d):
    n = 8192
    g = torch.Generator().manual_seed(40 + d)
    x, y = torch.randn(n, d, generator=g).to(gpu), (torch.randn(n, d, generator=g) * 1.3 + 0.5).to(gpu)
    s64, it64 = _dense_sinkhorn(x.double(), y.double())
    s32, _ = _dense_sinkhorn(x, y)
    out = E.sinkhorn(x, y)
    bound = 4 * max(F_SINKHORN, abs(s32 - s64) / s64)
    rel = abs(out["distance"].double().item() - s64) / s64
    print(f"sinkhorn full size d={d}: hip {out['distance'].item():.8g} dense64 {s64:.8g} dense32 {s32:.8g} rel {rel:.2e} bound {bound:.2e} "
          f"iters {out['iters']} (dense64 {it64}) materialised {out['materialised']}")
    assert rel <= bound and out["iters"] == it64
    m64, m32 = _dense_mmd(x.double(), y.double()), _dense_mmd(x, y)
    mmd = E.mmd_median(x, y)[0].double().item()
    bound = 4 * max(F_MMD, abs(m32 - m64) / m64)
    rel = abs(mmd - m64) / m64
    print(f"mmd full size d={d}: hip {mmd:.8g} dense64 {m64:.8g} dense32 {m32:.8g} rel {rel:.2e} bound {bound:.2e}")
    assert rel <= bound


@pytest.mark.gpu
def test_unequal_sizes_and_errors(gpu):
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(700, 3, generator=g).to(gpu), torch.randn(450, 3, generator=g).to(gpu)
    wx, wy = torch.ones(700, device=gpu) / 700, torch.ones(450, device=gpu) / 450
    out = E.sinkhorn(x, y, wx, wy, max_iters=30)
    M = _dense_cost(x.double(), y.double(), 2)
    u, v = out["u"].double(), out["v"].double()
    P = ((-M + u[:, None] + v[None, :]) / 1e-3).exp()  # the transport plan of the returned scalings
    assert out["distance"].item() == pytest.approx((P * M).sum().item(), rel=2e-3)  # (u, v leave as fp32: 1e-7 / eps in the exponent)
    assert out["iters"] == 30
    with pytest.raises(ValueError):  # uniform weights of unequal sizes do not sum to the same value (w_y *= n / m upstream)
        Sinkhorn()(x, y)
    with pytest.raises(NotImplementedError):
        Sinkhorn(p=3)(x, x)
    with pytest.raises(E.L.EngineError):
        E.sinkhorn(x, y, p=3)
    with pytest.raises(E.L.EngineError):
        E.mmd_median(x, y)


@pytest.mark.gpu
def test_evaluate_with_sample_metrics(gpu):
    from sde_sampler_lrds_amd.additions.hacking import TrainableWrapper
    from sde_sampler_lrds_amd.experiments.benchmark_utils import make_model, make_target_details
    args = ("vp-ref", "default", "lv", "ei", "base_zero_init", "uniform", dict(sigma=1.0), make_target_details("many_modes", dim=2, n_modes=4),
            dict(train_steps=1, train_batch_size=64, eval_batch_size=1024))
    model = make_model(*args, n_steps=16)
    assert set(model.eval_sample_losses) == {"sinkhorn", "mmd", "ks"}
    assert make_model(*args, n_steps=16, compute_samples_based_metrics=False).eval_sample_losses is None
    torch.manual_seed(11)
    res = model.evaluate(log=True)
    torch.manual_seed(11)
    plain = model.evaluate()
    gt = model.target.sample((1024,))
    direct = {"error/sinkhorn": Sinkhorn()(res.samples, gt).item(), "error/mmd": mmd_median(res.samples, gt).item(),
              "error/ks": compute_sliced_ks(res.samples, gt).item(), "eval/emc": model.target.entropy(res.samples).item()}
    print("evaluate(log=True):", {k: res.metrics[k] for k in direct})
    for key, val in direct.items():
        assert res.metrics[key] == val, key
    # a plain evaluate() reports what it did before the sample metrics existed
    base = {"eval/elbo", "eval/lv_loss", "eval/sample_time", "eval/norm_effective_sample_size"}
    assert base <= set(plain.metrics) and set(plain.metrics) <= set(res.metrics)
    assert not any(k.startswith("error/") or k in ("eval/emc", "eval/avg_stddev", "eval/square") for k in plain.metrics)
    assert set(plain.metrics) == set(model.compute_results().metrics)
    wrapped = TrainableWrapper(model, verbose=False, sample_metrics=True).evaluate()
    assert "error/sinkhorn" in wrapped.metrics and "error/sinkhorn" not in TrainableWrapper(model, verbose=False).evaluate().metrics
