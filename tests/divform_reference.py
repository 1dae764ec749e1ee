"""The strong residual in DIVERGENCE form (hpv_set_strong_form_div, k_div_indicators; VPINNLinear / VPINNNonlinear(strong_form=
"divergence")) in fp64 on the CPU (a plain helper module like linadapt_reference.py; no GPU needed).  tests/test_divform_host.py proves it.

Two problem formats, the forward passes and `terms` of their modules reused:

  * mapped_reference.problem (2-D: boxes, bilinear quadrilaterals, polar boxes; a full tensor K; an ansatz).  Everything is PHYSICAL,
    as in that module: with A the Jacobian of the element's map at a node, d = det A and adj(A) = d A^-1,

        r[j][i] = (1 / d) ( sum_m Dx[i][m] Fh1[j][m] + sum_m Dy[j][m] Fh2[m][i] ) + b . grad u + s u + N(u, grad u) - f        Fh = adj(A) K grad u

    -- the Piola transform of the flux, its nodal interpolant on the element's tensor rule, the divergence of that on the reference
    square, back to the physical element.  On a box A = diag(Jx, Jy) and this is (1/Jx) Dx (K grad u)_1 + (1/Jy) Dy (K grad u)_2.
    K_eff and the product's fold are never formed.  Column 1 is sum_q w_q d_q r_q^2, the quadrature of int r^2 dx.
  * linadapt_reference.problem (1-D and diagonal 2-D boxes):  r = (1/Jx) Dx (kx u_x) + (1/Jy) Dy (ky u_y) + bx u_x + by u_y + s u + N - f.

Columns 0, 2, 3, 4 come from R as the sibling modules compute it (linadapt_reference.indicators' meaning).
"""
import numpy as np

import linadapt_reference as la
import mapped_reference as mr
import validation_reference as vr

diff = la.diff


# ---- mapped_reference problems ------------------------------------------------------------------------------------------------------
def effective(p, full=None):
    """dict over mapped_reference.COEF_KEYS of the owned elements at the trainable scalars of `full`: base + sum_m c_m D_m"""
    full = mr.full0(p) if full is None else np.asarray(full, dtype=np.float64)
    c = full[full.size - len(p["dirs"]):]
    eb, ee = p["eb"], p["ee"]
    nq = p["X"].shape[1]
    shapes = dict(K=(2, 2), b=(2,), s=(), a2=(), a3=(), ae=(), g=(2,))
    out = {}
    for k, sh in shapes.items():
        v = np.array(p["coefs"][k][eb:ee]) if k in p["coefs"] else np.zeros((ee - eb, nq) + sh)
        for m, d in enumerate(p["dirs"]):
            if k in d:
                v = v + c[m] * d[k][eb:ee]
        out[k] = v
    return out


def channels(p, full=None):
    """u (n_owned, NQ) and grad u (n_owned, NQ, 2) at the owned points, through the ansatz where p has one (mapped_reference._u_du)"""
    full = mr.full0(p) if full is None else np.asarray(full, dtype=np.float64)
    o = vr.bare_oracle("p2", p["layers"], full[:full.size - len(p["dirs"])])
    X = p["X"][p["eb"]:p["ee"]]
    u, du = mr._u_du(o, p, X.reshape(-1, 2))
    return u.detach().numpy().reshape(X.shape[0], -1).copy(), du.detach().numpy().reshape(X.shape[0], -1, 2).copy()


def strong(p, f=0.0, full=None, u_du=None):
    """r [e][j][i], the physical strong residual in divergence form; f (n_owned, NQ) physical, or a constant; u_du: (u, grad u) given
    from outside in place of the network's"""
    u, du = channels(p, full) if u_du is None else u_du
    c = effective(p, full)
    A = p["A"][p["eb"]:p["ee"]]
    (xi, _), (yi, _) = p["xr"], p["yr"]
    qx, qy, ne = xi.size, yi.size, u.shape[0]
    det = A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
    adj = np.stack([np.stack([A[..., 1, 1], -A[..., 0, 1]], -1), np.stack([-A[..., 1, 0], A[..., 0, 0]], -1)], -2)
    Fh = np.einsum("eqab,eqbc,eqc->eqa", adj, c["K"], du).reshape(ne, qy, qx, 2)
    div = np.einsum("im,ejm->eji", diff(xi), Fh[..., 0]) + np.einsum("jm,emi->eji", diff(yi), Fh[..., 1])
    N = c["a2"] * u ** 2 + c["a3"] * u ** 3 + u * np.sum(c["g"] * du, axis=2)
    if np.any(c["ae"] != 0.0):
        N = N + c["ae"] * np.exp(u)
    low = np.sum(c["b"] * du, axis=2) + c["s"] * u + N
    f = np.broadcast_to(np.asarray(f, dtype=np.float64), u.shape)
    return div / det.reshape(ne, qy, qx) + (low - f).reshape(ne, qy, qx)


def indicators(p, r, t=None):
    """(n_owned, 5) from r [e][j][i] and mapped_reference.terms (R with inactive entries 0, loss_e in the case's norm)"""
    t = mr.terms(p) if t is None else t
    eb, ee = p["eb"], p["ee"]
    ne, ntx, nty = ee - eb, p["ntx"], p["nty"]
    A = p["A"][eb:ee]
    det = (A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]).reshape(r.shape)
    nax = np.full(ne, ntx) if p["nax"] is None else np.asarray(p["nax"][eb:ee])
    nay = np.full(ne, nty) if p["nay"] is None else np.asarray(p["nay"][eb:ee])
    out = np.zeros((ne, 5))
    for e in range(ne):
        B = t["R"][e, :nay[e], :nax[e]] ** 2
        out[e] = [t["loss_e"][e], np.einsum("j,i,ji->", p["yr"][1], p["xr"][1], det[e] * r[e] ** 2), B.sum(), B[:, nax[e] - 1].sum(), B[nay[e] - 1, :].sum()]
    return out


def reference(p, f=0.0, full=None):
    """dict(ind (n_owned, 5), r [e][j][i]) of a mapped_reference problem"""
    r = strong(p, f, full)
    return dict(ind=indicators(p, r, mr.terms(p, full)), r=r)


def device_f(p, f):
    """f as a device that runs unit elements must be handed it: times det A on mapped elements (p["boxes"] None), as it is on boxes"""
    A = p["A"][p["eb"]:p["ee"]]
    f = np.broadcast_to(np.asarray(f, dtype=np.float64), A.shape[:2])
    return (f if p["boxes"] is not None else f * (A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0])).reshape(-1).copy()


# ---- linadapt_reference problems (1-D, diagonal 2-D boxes) ------------------------------------------------------------------------------
def strong_lin(p, f=None):
    """r [e][j][i] of a linadapt_reference problem in divergence form; f as in linadapt_reference.strong_parts"""
    u, ux, uy, _, _ = la.channels(p)
    sh = u.shape
    pl, nl = la.effective_planes(p)
    pl, nl = [v.reshape(sh) for v in pl], [v.reshape(sh) for v in nl]
    b = p["boxes"][p["eb"]:p["ee"]]
    f = p["f"] if f is None else f
    f = np.broadcast_to(np.asarray(f, dtype=np.float64).reshape(-1) if np.size(f) > 1 else np.float64(f), (u.size,)).reshape(sh)
    Jx = ((b[:, 1] - b[:, 0]) / 2)[:, None, None]
    if p["dim"] == 2:
        kx, ky, bx, by, s = pl
        Jy = ((b[:, 3] - b[:, 2]) / 2)[:, None, None]
        r = np.einsum("im,ejm->eji", diff(p["xr"][0]), kx * ux) / Jx + np.einsum("jm,emi->eji", diff(p["yr"][0]), ky * uy) / Jy
        r = r + bx * ux + by * uy + s * u
        ga = nl[3] * ux + nl[4] * uy
    else:
        k, bb, s = pl
        r = np.einsum("im,ejm->eji", diff(p["xr"][0]), k * ux) / Jx + bb * ux + s * u
        ga = nl[3] * ux
    if p["kind"] != "lin" and any(np.any(v != 0.0) for v in nl):
        r = r + nl[0] * u ** 2 + nl[1] * u ** 3 + nl[2] * np.exp(u) + u * ga
    return r - f


def reference_lin(p, f=None):
    """dict(ind, r) of a linadapt_reference problem"""
    r = strong_lin(p, f)
    return dict(ind=la.indicators(p, la.projected_residuals(p), r), r=r)
