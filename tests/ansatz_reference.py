"""Exact Dirichlet conditions by ansatz u = G + D N on the variable-coefficient classes (hpv_set_ansatz, k_ansatz_fwd / k_ansatz_adj,
VPINNLinear / VPINNNonlinear(hard_bc=...)) in fp64 on the CPU, and the case table of tests/test_gpu_ansatz.py (a plain helper module
like ident_reference.py, which it extends; no GPU needed).  tests/test_ansatz_host.py proves it.

    u = G + D N        u_x = G_x + D_x N + D N_x   (same for y)
    Nbar = D ubar + D_x uxbar + D_y uybar          N_xbar = D uxbar          N_ybar = D uybar

Two derivations of the same loss and gradient:

  reference           the library's route, in numpy: the network's channels N, N_x(, N_y) at each point set (nonlinear_reference._channels,
                      flux_reference._u_du), the map applied to them with the PLANES (G, G_x, .., D, D_x, ..) as given numbers, the existing
                      residual / loss code on the mapped channels as leaves (ident_reference._loss: linear_reference's loss with the
                      nonlinear planes and the directions in it; zero planes add exact zeros), the channel adjoints pulled back through the
                      transposed map in numpy, and a vector-Jacobian product of the network for d loss / d theta.
  reference_autograd  independent: G and D as closed-form torch functions of the points, u = G(X) + D(X) net(X) differentiated with
                      respect to X by autograd (the planes' derivative rows are never read), one graph from theta to the loss.

Inputs: the problems of linear_reference / nonlinear_reference / ident_reference (same seeds, same draws) on the shapes of CASES, plus
the fields of FIELDS.  `generic` keeps D off zero on the boundary and is not a polynomial, so that every term of the adjoint carries
weight; `vanishing` is zero on the boundary of [-1, 1]^dim (u == G there for every theta); `identity` is G = 0, D = 1.
"""
import numpy as np
import torch

import data_term_reference as dr
import flux_reference as fr
import ident_reference as ir
import linear_reference as lr
import nonlinear_reference as nr
import validation_reference as vr

N_FLUX, N_VAL = 3, 33


# ---- the fields: value as a torch function of the points (n, dim) -> (n,), and the planes analytically in numpy ------------------------
def _g_generic(X):
    return torch.sin(X[:, 0] + (2.0 * X[:, 1] if X.shape[1] == 2 else 0.3))


def _d_generic(X):
    d = 1.0 - X[:, 0] ** 2
    return (d * (1.0 - X[:, 1] ** 2) if X.shape[1] == 2 else d) + 0.3


def _d_vanishing(X):
    d = 1.0 - X[:, 0] ** 2
    return d * (1.0 - X[:, 1] ** 2) if X.shape[1] == 2 else d


FIELDS = {
    "generic": (_g_generic, _d_generic),
    "vanishing": (_g_generic, _d_vanishing),
    "identity": (lambda X: torch.zeros(X.shape[0], dtype=torch.float64), lambda X: torch.ones(X.shape[0], dtype=torch.float64)),
}


def planes(kind, P):
    """(2 * (1 + dim), n): the rows (G, G_x[, G_y], D, D_x[, D_y]) of hpv_set_ansatz at the points P (n, dim), differentiated by hand"""
    P = np.asarray(P, dtype=np.float64)
    n, dim = P.shape
    x = P[:, 0]
    y = P[:, 1] if dim == 2 else None
    if kind == "identity":
        return np.concatenate([np.zeros((1 + dim, n)), np.ones((1, n)), np.zeros((dim, n))], 0)
    a = x + (2.0 * y if dim == 2 else 0.3)
    G = [np.sin(a), np.cos(a)] + ([2.0 * np.cos(a)] if dim == 2 else [])
    off = 0.3 if kind == "generic" else 0.0
    if dim == 2:
        D = [(1.0 - x * x) * (1.0 - y * y) + off, -2.0 * x * (1.0 - y * y), -2.0 * y * (1.0 - x * x)]
    else:
        D = [(1.0 - x * x) + off, -2.0 * x]
    return np.stack(G + D, 0)


def apply_map(A, N):
    """the channels [u, u_x(, u_y)] of u = G + D N from the network's [N, N_x(, N_y)] (numpy, (n,) each); len(N) == 1: the value alone"""
    dim = A.shape[0] // 2 - 1
    G, D = A[:1 + dim], A[1 + dim:]
    return [G[0] + D[0] * N[0]] + [G[k] + D[k] * N[0] + D[0] * N[k] for k in range(1, len(N))]


def apply_adjoint(A, ub):
    """the adjoints [Nbar, N_xbar(, N_ybar)] from [ubar, uxbar(, uybar)]"""
    dim = A.shape[0] // 2 - 1
    D = A[1 + dim:]
    nb = D[0] * ub[0]
    for k in range(1, len(ub)):
        nb = nb + D[k] * ub[k]
    return [nb] + [D[0] * ub[k] for k in range(1, len(ub))]


# ---- the problems ------------------------------------------------------------------------------------------------------------------------
def problem(c, kind="generic"):
    """the problem dict of case `c` (variant c['variant']: 'lin', 'nl' with all four terms, 'id' with two trainable coefficients) plus
    val = (X, u, du), kind, and ans = dict(quad, data, flux, val): the planes at each point set; full = [theta | c0]"""
    v = c["variant"]
    dim = c["L"][0]
    if v == "id":
        p = ir.problem(dict(c, terms=(), dirs=[[0, 1], [4, 6]] if dim == 2 else [[0], [2, 5]]))
    else:
        p = nr.problem(dict(c, terms=nr.TERMS if v == "nl" else ()))
        p["dirs"], p["c0"], p["full"] = np.zeros((0, sum(ir.n_planes(dim)), p["planes"].shape[1])), np.zeros(0), p["theta"].copy()
    rng = np.random.default_rng(c["seed"] + 29)
    Xv = dr.points(p["prob"], N_VAL, c["seed"] + 3)
    p["val"] = (Xv, rng.standard_normal(N_VAL), rng.standard_normal((N_VAL, dim)))
    with_fields(p, kind)
    return p


def with_fields(p, kind):
    """(re)evaluate the planes of every point set of p for the fields `kind`; None removes the ansatz"""
    p["kind"] = kind
    if kind is None:
        p["ans"] = None
        return p
    b = p["boxes"][p["eb"]:p["ee"]]
    Pq = lr.quad_points(b, p["xr"][0], p["yr"][0] if p["dim"] == 2 else None)
    p["ans"] = dict(quad=planes(kind, Pq), data=None if p["data"] is None else planes(kind, p["data"][0]),
                    flux=None if p["flux"] is None else planes(kind, p["flux"]["X"]), val=planes(kind, p["val"][0]))
    return p


def _vjp(outs, theta, cots):
    """sum_k cots[k] . d outs[k] / d theta"""
    g, = torch.autograd.grad(outs, theta, grad_outputs=[torch.tensor(np.ascontiguousarray(c)) for c in cots], retain_graph=True)
    return g.numpy().copy()


def _base_planes(p, ct):
    base = torch.tensor(np.concatenate([p["planes"], p["nl"]], 0))
    return base + torch.einsum("m,mpq->pq", ct, torch.tensor(p["dirs"])) if ct.numel() else base


def reference(p, full=None):
    """(loss triple, gradient [d theta | d c], R) of var + data + flux at `full` by the library's route (module docstring)"""
    theta, c = ir.split(p, p["full"] if full is None else full)
    A = p["ans"]
    ident = lambda a, n: n      # noqa: E731  (no ansatz: the channels as they are)
    fwd, adj = (apply_map, apply_adjoint) if A is not None else (ident, ident)
    # variational term
    o, ch = nr._channels(p, theta)
    leaves = [torch.tensor(v, requires_grad=True) for v in fwd(A and A["quad"], [t.detach().numpy() for t in ch])]
    ct = torch.tensor(c, requires_grad=True)
    R, _, lossv, mask = ir._loss(p, leaves, _base_planes(p, ct))
    gr = torch.autograd.grad(lossv, leaves + ([ct] if c.size else []))
    g = _vjp(ch, o.theta, adj(A and A["quad"], [t.numpy() for t in gr[:len(leaves)]]))
    gc = gr[-1].numpy().copy() if c.size else np.zeros(0)
    Rn = R.detach().numpy().copy()
    Rn[~mask] = 0.0
    # boundary / data term: lbw * mean((u - u_d)^2)
    d = dict(wmsq=0.0, msq=0.0)
    if p["data"] is not None:
        X, ud = p["data"]
        od = vr.bare_oracle(p["prob"], p["layers"], theta)
        N = od.neural_net(torch.tensor(X)).reshape(-1)
        u = torch.tensor(fwd(A and A["data"], [N.detach().numpy()])[0], requires_grad=True)
        sq = torch.square(torch.tensor(ud).reshape(-1, 1) - u.reshape(-1, 1)).reshape(-1)      # (data_term_reference.data_part's expression)
        ub, = torch.autograd.grad(float(p["lbw"]) * torch.mean(sq), u)
        msq = float(np.mean(sq.detach().numpy()))
        d = dict(msq=msq, wmsq=float(p["lbw"]) * msq)
        g = g + _vjp([N], od.theta, adj(A and A["data"], [ub.numpy()]))
    # flux term: w_f * mean((a u + b . grad u - g)^2)
    f = dict(wmsf=0.0, msf=0.0)
    if p["flux"] is not None:
        fx = p["flux"]
        of = vr.bare_oracle(p["prob"], p["layers"], theta)
        N, dN = fr._u_du(of, fx["X"])
        chf = [N] + [dN[:, k] for k in range(p["dim"])]
        uu = [torch.tensor(v, requires_grad=True) for v in fwd(A and A["flux"], [t.detach().numpy() for t in chf])]
        r = torch.tensor(fx["a"]) * uu[0] + torch.sum(torch.tensor(fx["b"]) * torch.stack(uu[1:], 1), dim=1) - torch.tensor(fx["g"])
        sq = torch.square(r)                                                                    # (flux_reference.flux_part's expression)
        ubf = torch.autograd.grad(float(fr.W_F) * torch.mean(sq), uu)
        msf = float(np.mean(sq.detach().numpy()))
        f = dict(msf=msf, wmsf=float(fr.W_F) * msf)
        g = g + _vjp(chf, of.theta, adj(A and A["flux"], [t.numpy() for t in ubf]))
    return fr.triple(p["prob"], float(lossv.detach()), d, f), np.concatenate([g, gc]), Rn


def reference_autograd(p, full=None):
    """(loss triple, gradient) of the same loss, one torch graph, G and D as closed-form functions of the points (module docstring)"""
    theta, c = ir.split(p, p["full"] if full is None else full)
    gt, dt = FIELDS[p["kind"]]
    o = vr.bare_oracle(p["prob"], p["layers"], theta)
    dim = p["dim"]

    def u_du(X):
        Xt = torch.tensor(np.asarray(X, dtype=np.float64), requires_grad=True)
        u = gt(Xt) + dt(Xt) * o.neural_net(Xt).reshape(-1)
        du, = torch.autograd.grad(u.sum(), Xt, create_graph=True)
        return u, du
    b = p["boxes"][p["eb"]:p["ee"]]
    u, du = u_du(lr.quad_points(b, p["xr"][0], p["yr"][0] if dim == 2 else None))
    ct = torch.tensor(c, requires_grad=True)
    _, _, lossv, _ = ir._loss(p, [u] + [du[:, k] for k in range(dim)], _base_planes(p, ct))
    msq = msf = torch.zeros((), dtype=torch.float64)
    if p["data"] is not None:
        msq = torch.mean(torch.square(u_du(p["data"][0])[0] - torch.tensor(p["data"][1])))
    if p["flux"] is not None:
        fx = p["flux"]
        uf, duf = u_du(fx["X"])
        msf = torch.mean(torch.square(torch.tensor(fx["a"]) * uf + torch.sum(torch.tensor(fx["b"]) * duf, dim=1) - torch.tensor(fx["g"])))
    loss = lossv + p["lbw"] * msq + fr.W_F * msf
    gr = torch.autograd.grad(loss, [o.theta] + ([ct] if c.size else []))
    d = dict(msq=float(msq.detach()), wmsq=p["lbw"] * float(msq.detach()))
    f = dict(msf=float(msf.detach()), wmsf=fr.W_F * float(msf.detach()))
    return fr.triple(p["prob"], float(lossv.detach()), d, f), np.concatenate([t.numpy() for t in gr])


def predict(p, X, full=None, grad=False):
    """u = G + D N at the points X (n,); grad: also its gradient (n, dim)"""
    theta, _ = ir.split(p, p["full"] if full is None else full)
    N, dN = fr._u_du(vr.bare_oracle(p["prob"], p["layers"], theta), X)
    ch = [N.detach().numpy()] + [dN[:, k].detach().numpy() for k in range(p["dim"])]
    if p["ans"] is not None:
        ch = apply_map(planes(p["kind"], X), ch)
    return (ch[0], np.stack(ch[1:], 1)) if grad else ch[0]


def validation(p, full=None, with_du=True):
    """the six sums of hpv_validate on p's validation set"""
    X, u, du = p["val"]
    uh, duh = predict(p, X, full, grad=True)
    return vr.norms(uh, u, duh if with_du else None, du if with_du else None)


def adam_trajectory(p, steps, lr_=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """`steps` TF1-Adam updates (the rule and constants of oracle.vpinn_oracle.adam_step) over network and coefficients"""
    th = np.array(p["full"], dtype=np.float64)
    m, v = np.zeros_like(th), np.zeros_like(th)
    b1p, b2p = b1, b2
    for _ in range(steps):
        g = reference(p, th)[1]
        lr_t = lr_ * np.sqrt(1.0 - b2p) / (1.0 - b1p)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        th = th - lr_t * m / (np.sqrt(v) + eps)
        b1p, b2p = b1p * b1, b2p * b2
    return th


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
def _grid_boxes(gx, gy):
    gx, gy = np.asarray(gx, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    return [[gx[i], gx[i + 1], gy[j], gy[j + 1]] for i in range(gx.size - 1) for j in range(gy.size - 1)]


# rows: 21 points (less than one wave); 180 points, qx != qy (a transposed plane layout shows; ends inside a workgroup); 840 points
# (several workgroups of 256 with a ragged tail)
ROWS = {
    "1d-21": dict(L=[1, 8, 8, 1], boxes=lr.BOXES1, q=7, nt=4),
    "2d-180": dict(L=lr.S8, boxes=_grid_boxes([-1.0, -0.2, 0.3, 1.0], [-1.0, 0.1, 1.0]), q=(6, 5), nt=(4, 3)),
    "2d-840": dict(L=lr.S8, boxes=_grid_boxes([-1.0, -0.55, -0.1, 0.25, 0.7, 1.0], [-1.0, -0.4, 0.1, 0.6, 1.0]), q=(7, 6), nt=(5, 4)),
}
VARIANTS = ("lin", "nl", "id")
DATA_COUNTS = (1, 17)
CASES = {}
for _i, (_r, _row) in enumerate(ROWS.items()):
    for _j, _v in enumerate(VARIANTS):
        for _k, _nd in enumerate(DATA_COUNTS):
            _name = "%s-%s-d%d" % (_r, _v, _nd)
            CASES[_name] = lr._c(_name, _row["L"], _row["boxes"], _row["q"], _row["nt"], 9700 + 20 * _i + 4 * _j + _k, data=_nd, flux=N_FLUX, variant=_v)
