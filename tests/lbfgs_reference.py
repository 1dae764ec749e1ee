"""References of the L-BFGS stage (hpv_lbfgs_step), written independently of the kernels and the driver (a plain helper module like
tests/cases.py):
  two_loop(S, Y, g)                  the two-loop recursion in numpy -- plain loops, math.fsum dot products;
  dense_bfgs_direction(S, Y, g)      the same direction from the dense BFGS inverse Hessian built pair by pair;
  torch_lbfgs(closure, theta0, ..)   torch.optim.LBFGS(line_search_fn="strong_wolfe") in fp64 on the CPU around a numpy closure,
                                     with every evaluation, the iteration count and the margins of the search's decisions recorded."""
import math

import numpy as np


def _dot(a, b):
    return math.fsum(float(x) * float(y) for x, y in zip(a, b))


def pair_scalars(S, Y):
    """(rho [n], h_diag): 1 / (y_i . s_i) per pair and (y . s) / (y . y) of the newest (last) one; h_diag 1.0 without pairs."""
    rho = np.array([1.0 / _dot(y, s) for s, y in zip(S, Y)])
    if len(S) == 0:
        return rho, 1.0
    return rho, _dot(Y[-1], S[-1]) / _dot(Y[-1], Y[-1])


def two_loop(S, Y, g, rho=None, h_diag=None):
    """d = -H g for the pairs S[i], Y[i] (oldest first).  rho, h_diag: as pair_scalars gives them unless handed in."""
    S, Y, g = np.asarray(S, dtype=np.float64), np.asarray(Y, dtype=np.float64), np.asarray(g, dtype=np.float64)
    n = len(S)
    if rho is None or h_diag is None:
        rho, h_diag = pair_scalars(S, Y)
    q = -g.copy()
    al = [0.0] * n
    for i in range(n - 1, -1, -1):
        al[i] = rho[i] * _dot(S[i], q)
        for j in range(q.size):
            q[j] -= al[i] * Y[i][j]
    r = q * h_diag
    for i in range(n):
        be = rho[i] * _dot(Y[i], r)
        for j in range(r.size):
            r[j] += (al[i] - be) * S[i][j]
    return r


def dense_bfgs_direction(S, Y, g):
    """-H g with H built densely: H_0 = h_diag I, H_{k+1} = (I - rho s y^T) H_k (I - rho y s^T) + rho s s^T."""
    S, Y, g = np.asarray(S, dtype=np.float64), np.asarray(Y, dtype=np.float64), np.asarray(g, dtype=np.float64)
    P = g.size
    _, h_diag = pair_scalars(S, Y)
    H = h_diag * np.eye(P)
    for s, y in zip(S, Y):
        rho = 1.0 / float(y @ s)
        V = np.eye(P) - rho * np.outer(s, y)
        H = V @ H @ V.T + rho * np.outer(s, s)
    return -H @ g


def torch_lbfgs(closure, theta0, max_iter, history=20, lr=1.0, tolerance_grad=1e-7, tolerance_change=1e-9, max_eval=None):
    """One `step` of torch.optim.LBFGS with the strong-Wolfe search on closure(theta) -> (loss, grad), numpy in and out.  Returns
    dict(theta, func_evals, n_iter, evals = [(theta, loss)] of every evaluation, losses = the loss after every iteration (from the
    starting point on), margin = the smallest relative distance of any decision of the line searches from its threshold: the
    sufficient-decrease test |f_new - (f + c1 t gtd)| / |f|, the curvature test ||gtd_new| - c2 |gtd|| / |gtd| and the sign test
    |gtd_new| / |gtd|)."""
    import torch
    import torch.optim.lbfgs as L
    p = torch.nn.Parameter(torch.tensor(np.asarray(theta0, dtype=np.float64).copy()))
    opt = torch.optim.LBFGS([p], lr=lr, max_iter=max_iter, max_eval=max_eval, tolerance_grad=tolerance_grad,
                            tolerance_change=tolerance_change, history_size=history, line_search_fn="strong_wolfe")
    evals, losses, margins = [], [], []

    def cl():
        th = p.detach().numpy().copy()
        loss, grad = closure(th)
        p.grad = torch.tensor(np.asarray(grad, dtype=np.float64).copy())
        evals.append((th, float(loss)))
        return torch.tensor(float(loss), dtype=torch.float64)

    inner = L._strong_wolfe

    def watched(obj_func, x, t, d, f, g, gtd, c1=1e-4, c2=0.9, tolerance_change=1e-9, max_ls=25):
        if not losses:
            losses.append(float(f))

        def obj(x_, t_, d_):
            f_new, g_new = obj_func(x_, t_, d_)
            gtd_new = float(g_new.dot(d_))
            margins.append(abs(f_new - (float(f) + c1 * float(t_) * float(gtd))) / max(abs(float(f)), 1e-300))
            margins.append(abs(abs(gtd_new) - c2 * abs(float(gtd))) / abs(float(gtd)))
            margins.append(abs(gtd_new) / abs(float(gtd)))
            return f_new, g_new
        out = inner(obj, x, t, d, f, g, gtd, c1, c2, tolerance_change, max_ls)
        losses.append(float(out[0]))
        return out

    L._strong_wolfe = watched
    try:
        opt.step(cl)
    finally:
        L._strong_wolfe = inner
    st = opt.state[p]
    return dict(theta=p.detach().numpy().copy(), func_evals=int(st["func_evals"]), n_iter=int(st["n_iter"]), evals=evals,
                losses=losses, margin=min(margins) if margins else float("inf"))
