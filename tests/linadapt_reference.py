"""The element-wise strong form of the variable-coefficient classes (hpv_set_strong_form, hpv_linear_indicators, k_lin_indicators;
VPINNLinear / VPINNNonlinear(strong_form="elementwise")) in fp64 on the CPU, and the case table of tests/test_gpu_linadapt.py (a
plain helper module like linear_reference.py; no GPU needed).  tests/test_linadapt_host.py proves it.  Of hp_vpinns_amd only
quadrature.diff_matrix is imported here (it is under test on the host); the sibling reference modules bring rules and tables.

    r = kx u_xx + dkx u_x + ky u_yy + dky u_y + bx u_x + by u_y + s u + N(u, grad u) - f          (1-D: k u'' + dk u' + b u' + s u + N - f)
    dkx[e][j][i] = (sum_m Dx[i][m] kx[e][j][m]) / Jx[e]        dky[e][j][i] = (sum_m Dy[j][m] ky[e][m][i]) / Jy[e]
    N = a2 u^2 + a3 u^3 + ae exp(u) + u (gx u_x + gy u_y)

with every plane the EFFECTIVE one (base + sum_m c_m D_m where the case has trainable coefficients) and Dx, Dy = diff_matrix of the
rule's nodes.  The five columns per owned element (include/hpvpinn.h, hpv_element_indicators):
    0 loss_e = sumR2 / (nax nay)    1 eta2 = J sum_q w_x[i] w_y[j] r^2    2 sumR2 over the active block    3 topx (r == nax - 1)
    4 topy (k == nay - 1; 0 in 1-D)
R comes from linear_reference / nonlinear_reference / ident_reference .var_part as those modules compute it; u and its first and
second derivatives by torch autograd through the oracle's own `neural_net` (validation_reference.bare_oracle).

Inputs.  Every case is a generic point: generic_point.generic_theta (Xavier + 0.3 N(0, 1) on every weight and bias), boxes of unequal
width AND unequal aspect (Jx != Jy, different from box to box), and smooth NON-polynomial coefficient fields (`fields`): the sibling
modules' random planes are replaced by them, so that the derivative of the interpolant means something; F is seeded N(0, 1) scaled to
the size of the projections, f is a field of its own.
"""
import numpy as np
import torch

import generic_point as gp
import ident_reference as ir
import linear_reference as lr
import nonlinear_reference as nr
import validation_reference as vr

F_SCALE = 0.5      # |F| against the projections of these smooth fields (linear_reference's 0.03 belongs to its random planes)


def diff(x):
    from hp_vpinns_amd.quadrature import diff_matrix
    return diff_matrix(x)


# ---- smooth non-polynomial fields at points P (n, dim); y = 0 in 1-D ----------------------------------------------------------------
def fields(P):
    """dict(planes (K, n), nl (M, n), f (n,), dir_k (n,), dir_s (n,)) at the points P"""
    x = P[:, 0]
    y = P[:, 1] if P.shape[1] == 2 else np.zeros_like(x)
    kx = 1.2 + 0.5 * np.sin(1.7 * x + 0.9 * y + 0.3)
    ky = 0.9 + 0.4 * np.cos(1.3 * x - 2.1 * y)
    bx = 0.8 * np.exp(0.5 * x) - 0.3 * y
    by = -0.7 + 0.5 * np.sin(2.0 * y + x)
    s = 0.5 + 0.6 * np.cos(x * y + 0.4 * x)
    a2 = 0.7 + 0.3 * np.sin(3.0 * x - y)
    a3 = -0.8 + 0.3 * np.cos(2.0 * y + x)
    ae = 0.3 + 0.5 * np.exp(-x * x - y * y)
    gx = 0.9 + 0.4 * np.sin(x - y)
    gy = -0.6 + 0.3 * np.cos(2.0 * x + 0.5 * y)
    f = np.sin(2.3 * x + 0.7) * np.cosh(0.8 * y) + 0.4
    if P.shape[1] == 2:
        planes, nl = np.stack([kx, ky, bx, by, s]), np.stack([a2, a3, ae, gx, gy])
    else:
        planes, nl = np.stack([kx, bx, s]), np.stack([a2, a3, ae, gx])
    return dict(planes=planes, nl=nl, f=f, dir_k=0.6 + 0.3 * np.cos(2.0 * x + y), dir_s=0.9 + 0.7 * np.sin(1.5 * x - 0.5 * y))


def problem(c):
    """The problem dict of the sibling modules (ident_reference.problem: planes, nl, dirs, c0, full, F, ...) for case dict `c`, with
    the smooth fields in place of the random ones, f (n_owned * NQ,) and kind ('lin' | 'nl' | 'id')."""
    p = ir.problem(dict(c, dirs=c.get("dirs", []), terms=c.get("terms", ())))
    dim, eb, ee = p["dim"], p["eb"], p["ee"]
    P = lr.quad_points(p["boxes"][eb:ee], p["xr"][0], p["yr"][0] if dim == 2 else None)
    fl = fields(P)
    p["planes"] = fl["planes"]
    p["nl"] = np.where(p["nl"] != 0.0, fl["nl"], 0.0)
    K = p["planes"].shape[0]
    for m in range(p["dirs"].shape[0]):
        for r in range(p["dirs"].shape[1]):
            if np.any(p["dirs"][m, r] != 0.0):
                p["dirs"][m, r] = fl["dir_k"] if r < K - 1 else fl["dir_s"]
    p["f"] = fl["f"]
    p["F"] = F_SCALE * np.random.default_rng(c["seed"] + 29).standard_normal(p["F"].shape)
    p["kind"] = "id" if p["dirs"].shape[0] else ("nl" if p["terms"] else "lin")
    return p


def projected_residuals(p):
    """R (n_owned, nty, ntx) as the sibling module of the case's kind computes it"""
    if p["kind"] == "lin":
        return lr.var_part(p)["R"]
    if p["kind"] == "nl":
        return nr.var_part(p)["R"]
    return ir.var_part(p, grad=False)["R"]


def effective_planes(p):
    if p["kind"] == "id":
        return ir.effective(p, p["c0"])
    return p["planes"], p["nl"]


def channels(p, theta=None):
    """u, u_x, u_y, u_xx, u_yy at the owned quadrature points as [e][j][i] numpy (u_y, u_yy None in 1-D): torch autograd through the
    oracle's own neural_net"""
    o = vr.bare_oracle(p["prob"], p["layers"], p["theta"] if theta is None else theta)
    dim, b = p["dim"], p["boxes"][p["eb"]:p["ee"]]
    xi = p["xr"][0]
    yi = p["yr"][0] if dim == 2 else None
    X = torch.tensor(lr.quad_points(b, xi, yi), requires_grad=True)
    u = o.neural_net(X)
    du, = torch.autograd.grad(u.sum(), X, create_graph=True)
    shape = (b.shape[0], 1 if yi is None else yi.size, xi.size)
    out = [u.reshape(-1)]
    second = []
    for d in range(dim):
        d2, = torch.autograd.grad(du[:, d].sum(), X, retain_graph=True)
        out.append(du[:, d])
        second.append(d2[:, d])
    v = [t.detach().numpy().reshape(shape).copy() for t in out + second]
    return (v[0], v[1], None, v[2], None) if dim == 1 else (v[0], v[1], v[2], v[3], v[4])


def plane_derivatives(p, kx, ky=None, Dx=None, Dy=None):
    """(dkx, dky) [e][j][i] of planes given as [e][j][i]: the derivative of the element-wise interpolant at the element's own points"""
    b = p["boxes"][p["eb"]:p["ee"]]
    Dx = diff(p["xr"][0]) if Dx is None else Dx
    dkx = np.einsum("im,ejm->eji", Dx, kx) / ((b[:, 1] - b[:, 0]) / 2)[:, None, None]
    if ky is None:
        return dkx, None
    Dy = diff(p["yr"][0]) if Dy is None else Dy
    return dkx, np.einsum("jm,emi->eji", Dy, ky) / ((b[:, 3] - b[:, 2]) / 2)[:, None, None]


def strong_parts(p, f=None, theta=None, dk=None, Dx=None, Dy=None):
    """dict of the terms of r as [e][j][i]: 'diff' (kx u_xx + ky u_yy), 'dkx' (dkx u_x), 'dky' (dky u_y; absent in 1-D), 'low' (bx u_x
    + by u_y + s u), 'N' (absent without terms), 'f', and 'r' itself.  f: (n_owned * NQ,), default the case's, 0.0 for none;
    dk = (dkx, dky): the planes' derivatives given from outside (the analytic ones of the host test) instead of D k."""
    u, ux, uy, uxx, uyy = channels(p, theta)
    sh = u.shape
    pl, nl = effective_planes(p)
    pl, nl = [v.reshape(sh) for v in pl], [v.reshape(sh) for v in nl]
    f = p["f"] if f is None else f
    out = {"f": np.broadcast_to(np.asarray(f, dtype=np.float64).reshape(-1) if np.size(f) > 1 else np.float64(f), (u.size,)).reshape(sh).copy()}
    if p["dim"] == 2:
        kx, ky, bx, by, s = pl
        dkx, dky = plane_derivatives(p, kx, ky, Dx, Dy) if dk is None else dk
        out.update(diff=kx * uxx + ky * uyy, dkx=dkx * ux, dky=dky * uy, low=bx * ux + by * uy + s * u)
        ga = nl[3] * ux + nl[4] * uy
    else:
        k, bb, s = pl
        dkx = plane_derivatives(p, k, None, Dx)[0] if dk is None else dk[0]
        out.update(diff=k * uxx, dkx=dkx * ux, low=bb * ux + s * u)
        ga = nl[3] * ux
    r = out["diff"] + out["dkx"] + out.get("dky", 0.0) + out["low"]
    if p["kind"] != "lin" and any(np.any(v != 0.0) for v in nl):
        out["N"] = nl[0] * u ** 2 + nl[1] * u ** 3 + nl[2] * np.exp(u) + u * ga
        r = r + out["N"]
    out["r"] = r - out["f"]
    return out


def indicators(p, R, r):
    """(n_owned, 5) from R (n_owned, nty, ntx; inactive entries 0) and r [e][j][i]"""
    eb, ee = p["eb"], p["ee"]
    b = p["boxes"][eb:ee]
    ne, ntx, nty = ee - eb, p["ntx"], p["nty"]
    wx = p["xr"][1]
    wy = p["yr"][1] if p["dim"] == 2 else np.ones(1)
    J = np.prod((b[:, 1::2] - b[:, 0::2]) / 2, axis=1)
    nax = np.full(ne, ntx) if p["nax"] is None else np.asarray(p["nax"][eb:ee])
    nay = np.full(ne, nty) if p["nay"] is None else np.asarray(p["nay"][eb:ee])
    out = np.zeros((ne, 5))
    for e in range(ne):
        A = R[e, :nay[e], :nax[e]] ** 2
        out[e, 2] = A.sum()
        out[e, 0] = out[e, 2] / (nax[e] * nay[e])
        out[e, 1] = J[e] * np.einsum("j,i,ji->", wy, wx, r[e] ** 2)
        out[e, 3] = A[:, nax[e] - 1].sum()
        out[e, 4] = A[nay[e] - 1, :].sum() if p["dim"] == 2 else 0.0
    return out


def reference(p, f=None):
    """dict(ind (n_owned, 5), r [e][j][i], parts, R) of case `p`; f as in strong_parts"""
    R = projected_residuals(p)
    parts = strong_parts(p, f)
    return dict(ind=indicators(p, R, parts["r"]), r=parts["r"], parts=parts, R=R)


def lds_bytes(dim, qx, qy):
    """the LDS of one k_lin_indicators workgroup by the formula of include/hpvpinn.h (hpv_set_strong_form)"""
    return 8 * ((2 if dim == 2 else 1) * qy * (qx | 1) + qx * (qx | 1) + (qy * (qy | 1) if dim == 2 else 0) + 16)


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# boxes of unequal width and unequal aspect inside [-1, 1]^2: Jx / Jy runs from 0.36 to 2.6 over them
BOXES2 = [[-1.0, -0.2, -1.0, 0.1], [-0.2, 1.0, -1.0, -0.3], [-1.0, -0.4, 0.1, 1.0], [-0.4, 0.3, 0.1, 0.55], [0.3, 0.95, -0.3, 0.9],
          [-0.4, 0.3, 0.55, 1.0], [-0.2, 0.3, -0.3, 0.1]]
BOXES1 = [[-1.0, -0.35], [-0.35, 0.2], [0.2, 0.65], [0.65, 1.0]]
S8 = [2, 8, 8, 1]


def _c(name, L, boxes, q, nt, seed, **kw):
    return dict(name=name, L=L, boxes=boxes, q=q, nt=nt, seed=seed, **kw)


CASES = {
    # qx != qy: Dx and Dy are not interchangeable; NQ = 35 is below one wave
    "2d-7x5": _c("2d-7x5", S8, BOXES2[:5], (7, 5), (4, 3), 9501),
    # NQ = 272 > 256: the stride loop runs; per-element counts
    "2d-17x16-counts": _c("2d-17x16-counts", S8, BOXES2[:3], (17, 16), (6, 5), 9502, counts=([6, 4, 5], [3, 5, 2])),
    # qy = 1, topy = 0, one D
    "1d-33-counts": _c("1d-33-counts", [1, 8, 8, 1], BOXES1, 33, 7, 9503, counts=([7, 4, 6, 5], None)),
    # mask = exp + advection only: the quadratic and cubic planes are never read
    "nl-6x6-exp-adv": _c("nl-6x6-exp-adv", S8, BOXES2[:3], (6, 6), (4, 3), 9504, terms=("exp", "adv")),
    # two trainable coefficients at non-initial values: one direction in kx (its derivative enters dkx), one in sigma
    "id-6x5": _c("id-6x5", S8, BOXES2[:3], (6, 5), (4, 3), 9505, dirs=[[0], [4]]),
    # a direction on a NONLINEAR plane (a3) with no base term: the cubic term is active through the direction alone and its base is the
    # handle's zero planes; the other direction is in ky (its derivative enters dky)
    "id-6x5-cubic-dir": _c("id-6x5-cubic-dir", S8, BOXES2[:3], (6, 5), (4, 3), 9508, dirs=[[1], [6]]),
}
TWIN = _c("twin-7-boxes", S8, BOXES2, (7, 5), (4, 3), 9506)      # Poisson twin: kappa = 1, beta = sigma = 0 on seven boxes


def twin_problem():
    p = problem(TWIN)
    p["planes"] = np.repeat(np.array([1.0, 1.0, 0.0, 0.0, 0.0])[:, None], p["planes"].shape[1], axis=1)
    return p


# ---- the class case: VPINNLinear(strong_form="elementwise") on a graded 4-element boundary-layer mesh ------------------------------
CLASS_EPS = 0.2
CLASS = dict(layers=[1, 8, 8, 1], n_quad=9, n_test=3, seed=9507, grid=1.0 - (1.0 - np.arange(5) / 4.0) ** 2.0)


def class_kappa(P):
    return -CLASS_EPS * (1.0 + 0.5 * np.sin(2.0 * P[:, 0]))


def class_f(P):
    return 1.0 + 0.8 * np.sin(20.0 * P[:, 0])      # (oscillatory: the top test function of the small elements keeps a share of R)


def class_problem():
    """the problem dict of the model tests/test_gpu_linadapt.py builds from CLASS (kappa = class_kappa, beta = 1, sigma = 0, f = class_f)"""
    g = CLASS["grid"]
    boxes = np.stack([g[:-1], g[1:]], 1)
    xr = lr.rule(CLASS["n_quad"])
    P = lr.quad_points(boxes, xr[0])
    ne, nq = boxes.shape[0], xr[0].size
    planes = np.stack([class_kappa(P), np.ones(ne * nq), np.zeros(ne * nq)])
    f = class_f(P)
    p = dict(prob="p1", dim=1, layers=list(CLASS["layers"]), theta=gp.generic_theta(CLASS["layers"], CLASS["seed"]), boxes=boxes, eb=0, ee=ne,
             xr=xr, yr=None, ntx=CLASS["n_test"], nty=1, nax=None, nay=None, planes=planes, nl=np.zeros((4, ne * nq)), f=f,
             flux=None, data=None, lbw=10.0, act="sin", kind="lin", terms=(), dirs=np.zeros((0, 7, ne * nq)), c0=np.zeros(0))
    ax = nr._tables(p)[0][0].numpy()                                # [ntx][qx]  w phi: F as hpv_assemble_rhs defines it
    J = (boxes[:, 1] - boxes[:, 0]) / 2
    p["F"] = J[:, None, None] * np.einsum("ri,ei->er", ax, f.reshape(ne, nq))[:, None, :]
    return p
