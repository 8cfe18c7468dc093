"""Torch statements of the CMCD KL gradient, shared by the CPU and GPU tests of the one-launch adjoint (sdeng_cmcd_kl_adjoint).

``whole_loop``       autograd through the reference's own loop (losses/oc.py:703-750 with train=True, rnd0 = 0): the ground truth.
``step_costs``       c_j = cost_j dt_j + db_j on given states, without a graph (what the host hands the kernel as ``cbar``).
``npoint_recursion`` the recursion over the N + 1 evaluation points (include/sdeng.h, sdeng_cmcd_kl_adjoint) with the states as constants;
                     the two Jacobian-transpose products of a point are taken by autograd on that point alone.
Any dtype: the modules decide."""
import torch


def whole_loop(ctrl, sde, neg_log_target, ts, x0, z, w):
    """-> (sum_b w_b rnd_b, [gradient per parameter of ctrl], states [N+1,B,d] detached, d loss / d x_N through the terminal alone)."""
    params = [p for p in ctrl.parameters() if p.requires_grad]
    g, N = sde.diff_coeff, ts.numel() - 1
    x, rnd, xs = x0, 0.0, [x0]
    for k in range(N):
        s, t = ts[k], ts[k + 1]
        dt = t - s
        db = dt.sqrt() * z[k]
        u_s, b_s = ctrl(s, x), sde.drift(s, x)
        y = x + (b_s + u_s * g) * dt + g * db
        cost = (b_s + sde.drift(t, y)) / g + u_s - ctrl(t, y)
        rnd = rnd + 0.5 * (cost ** 2).sum(-1, keepdim=True) * dt + (cost * db).sum(-1, keepdim=True)
        x = y
        xs.append(y)
    loss = (w * (rnd + neg_log_target(x).view(-1, 1))).sum()
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    xn = x.detach().requires_grad_(True)
    lam_n, = torch.autograd.grad((w * neg_log_target(xn).view(-1, 1)).sum(), xn)
    return loss.detach(), [torch.zeros_like(p) if gr is None else gr for p, gr in zip(params, grads)], torch.stack([v.detach() for v in xs]), lam_n


def step_costs(ctrl, sde, ts, xs, z):
    """cbar [N,B,d]: cost_j dt_j + db_j with cost_j = (b_j + b_{j+1})/g + u_j - u_{j+1} evaluated on the given states."""
    g, N = sde.diff_coeff, ts.numel() - 1
    with torch.no_grad():
        u = torch.stack([ctrl(ts[j], xs[j].clone()) for j in range(N + 1)])
    b = torch.stack([sde.drift(ts[j], xs[j].clone()).detach() for j in range(N + 1)])
    dt = (ts[1:] - ts[:-1]).view(N, 1, 1)
    cost = (b[:-1] + b[1:]) / g + u[:-1] - u[1:]
    return cost * dt + dt.sqrt() * z


def npoint_recursion(ctrl, sde, ts, xs, cbar, w, lam_n):
    """Lambda_{N+1} = lam_n; for j = N .. 0 (c_j = w cbar_j, c_{-1} = c_N = 0, dt_N = 0):
        ubar_j = g dt_j Lambda + c_j - c_{j-1} ;  v_j = dt_j Lambda + (c_j + c_{j-1})/g ;  Lambda += J_u(x_j)^T ubar_j + J_b(x_j)^T v_j
    -> (Lambda_0, [gradient per parameter])."""
    params = [p for p in ctrl.parameters() if p.requires_grad]
    grads = [torch.zeros_like(p) for p in params]
    g, N = sde.diff_coeff, ts.numel() - 1
    lam, zero = lam_n, torch.zeros_like(lam_n)
    for j in range(N, -1, -1):
        dt = ts[j + 1] - ts[j] if j < N else torch.zeros_like(ts[0])
        cj = w * cbar[j] if j < N else zero
        cm = w * cbar[j - 1] if j > 0 else zero
        ubar, v = g * dt * lam + cj - cm, dt * lam + (cj + cm) / g
        xj = xs[j].detach().clone().requires_grad_(True)
        got = torch.autograd.grad((ubar * ctrl(ts[j], xj)).sum() + (v * sde.drift(ts[j], xj)).sum(), [xj] + params, allow_unused=True)
        lam = lam + got[0]
        for acc, gk in zip(grads, got[1:]):
            if gk is not None:
                acc.add_(gk)
    return lam, grads
