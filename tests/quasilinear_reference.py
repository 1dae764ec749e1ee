"""Quasilinear diffusion on the variable-coefficient class (hpv_set_quasilinear, the _q instantiations of k_project_nl, k_div_indicators,
VPINNNonlinear(diffusivity=)) in fp64 on the CPU (a plain helper module like mapped_reference.py, whose geometry and problem dict it
uses; no GPU needed).  tests/test_quasilinear_host.py proves it.

Everything is stated in PHYSICAL terms, as in mapped_reference: with A the Jacobian of the element map at a quadrature point, d = det A,
v_kr = phi_r(xi) phi_k(eta) and grad_x v = A^-T grad_ref v,

    R[e][k][r] = sum_q w_q d_q [ -(mu K grad u) . grad_x v_kr + (b . grad u + s u + N(u, grad u)) v_kr ] - F[e][k][r]
    mu = P(u) B(s)      P = m0 + m1 u + m2 u^2      B = (delta + s)^r      s = |grad u|^2
    N  = a2 u^2 + a3 u^3 + ae exp(u) + u (g . grad u)

A box is the map with A = diag(Jx, Jy); a 1-D element the 1 x 1 case (A = Jx, K, b and g with one component, one test function "1" in
y).  Nothing of the product's fold is imported: K_eff = adj(A) K is never formed here.  A factor that is switched off is left out of
the expression (q["use_u"], q["use_grad"]), exactly as the mask of the kernel leaves it out.

    loss_e = mean over the ACTIVE test functions of R^2,  or  R_e^T G_e^-1 R_e  with the Gram matrices p["gram"] (a list over the
             owned elements: dualnorm_reference.gram_element for the table norm on boxes, dualdense_reference.gram_dense for the dense
             norms -- the energy metric uses K alone, never mu K)
    loss triple = (lossv + lbw msq, msq, lossv)

  terms(p, theta)       R, loss_e, the triple and d loss / d theta by torch autograd through the oracle's own network
  channel_adjoints(p)   the same loss with the channels u, u_x(, u_y) as leaves: autograd's d lossv / d channel (what GBAR holds)
  strong(p, f)          the physical strong residual in divergence form, (1/d) div_ref(adj(A) mu K grad u) + .. - f, with the rule's
                        differentiation matrices (linadapt_reference.diff), and indicators(): the five columns of hpv_linear_indicators
"""
import numpy as np
import torch

import dualdense_reference as dd
import dualnorm_reference as dn
import generic_point as gp
import linadapt_reference as la
import linear_reference as lr
import mapped_reference as mr
import validation_reference as vr

LBW = lr.LBW


# ---- geometry of 1-D elements in mapped_reference's terms --------------------------------------------------------------------------------
def geom_1d(boxes, xi):
    b = np.asarray(boxes, dtype=np.float64)
    hx = (b[:, 1] - b[:, 0]) / 2
    X = (b[:, 0:1] + hx[:, None] * (xi[None, :] + 1))[:, :, None]
    return X, np.broadcast_to(hx[:, None, None, None], X.shape + (1,)).copy()


# ---- the problem dict: mapped_reference.problem's plus q ---------------------------------------------------------------------------------
def quasi_planes(rng, ne, nq, use_u=True, use_grad=True, r=-0.5, varying=True):
    """dict(m (ne, nq, 3), delta (ne, nq), r, use_u, use_grad): m0 in U(0.5, 1.5), m1, m2 signed U(0.5, 1.5) * 0.5, delta in U(0.5, 1.5);
    a factor that is off holds the values that make it 1 (m = (1, 0, 0); r = 0)"""
    m = np.zeros((ne, nq, 3))
    m[..., 0] = 1.0
    if use_u:
        m[..., 0] = rng.uniform(0.5, 1.5, (ne, nq)) if varying else 1.0
        m[..., 1:] = 0.5 * mr._signed(rng, (ne, nq, 2)) if varying else np.array([0.3, 1.0])
    delta = rng.uniform(0.5, 1.5, (ne, nq)) if varying else np.full((ne, nq), 1.0)
    return dict(m=m, delta=delta, r=float(r) if use_grad else 0.0, use_u=bool(use_u), use_grad=bool(use_grad))


def problem(dim, layers, seed, X, A, rules, nt, coefs, q, counts=None, data=0, ansatz=None, boxes=None, gram=None):
    """mapped_reference.problem with dim, the quasilinear planes q (quasi_planes) and the Gram matrices of the loss (None: mean(R^2))"""
    if dim == 2:
        p = mr.problem(layers, seed, X, A, rules[0], rules[1], nt, coefs, counts=counts, data=data, ansatz=ansatz, boxes=boxes)
    else:                                                 # (the same dict for 1-D elements: one point and the function "1" in y)
        rng = np.random.default_rng(seed + 7)
        ne = X.shape[0]
        nax = None if counts is None else np.asarray(counts, dtype=np.int32)
        p = dict(prob="p1", dim=1, layers=list(layers), theta=gp.generic_theta(layers, seed), c0=np.zeros(0), X=X, A=A, eb=0, ee=ne,
                 xr=rules[0], yr=(np.zeros(1), np.ones(1)), ntx=int(nt), nty=1, nax=nax, nay=None if nax is None else np.ones_like(nax),
                 coefs=coefs, dirs=[], F=mr.F_SCALE * rng.standard_normal((ne, 1, int(nt))), data=None, flux=None, ansatz=None, mass=None,
                 boxes=boxes, lbw=LBW, act="sin")
    p["q"], p["gram"] = q, gram
    return p


def _u_du(o, p, Xn):
    if p["dim"] == 2:
        return mr._u_du(o, p, Xn)
    Xt = torch.tensor(np.ascontiguousarray(Xn), requires_grad=True)
    N = o.neural_net(Xt).reshape(-1)
    dN, = torch.autograd.grad(N.sum(), Xt, create_graph=True)
    return N, dN


def mu_of(q, u, s, sl=slice(None)):
    """mu at torch channels u, s = |grad u|^2 (ne, nq); only the factors that are switched on are formed"""
    mu = torch.ones_like(u)
    if q["use_u"]:
        m = torch.tensor(q["m"][sl])
        mu = m[..., 0] + m[..., 1] * u + m[..., 2] * u ** 2
    if q["use_grad"]:
        mu = mu * (torch.tensor(q["delta"][sl]) + s) ** q["r"]
    return mu


def _loss(p, u, du, q=None, coefs=None):
    """from the channels u (ne, nq), du (ne, nq, dim) as torch tensors: dict(R, loss_e, lossv, mask)"""
    from hp_vpinns_amd.testfcn import tables_1d
    dim, eb, ee = p["dim"], p["eb"], p["ee"]
    ne, sl = ee - eb, slice(eb, ee)
    q = p["q"] if q is None else q
    coefs = p["coefs"] if coefs is None else coefs
    A = torch.tensor(p["A"][sl])
    (xi, wx), (yi, wy) = p["xr"], p["yr"]
    qx, qy, ntx, nty = xi.size, yi.size, p["ntx"], p["nty"]

    def field(key, shape):
        return torch.tensor(coefs[key][sl]) if key in coefs else torch.zeros((ne, qx * qy) + shape, dtype=torch.float64)
    K, b, s0 = field("K", (dim, dim)), field("b", (dim,)), field("s", ())
    a2, a3, ae, g = field("a2", ()), field("a3", ()), field("ae", ()), field("g", (dim,))
    det, Ainv = torch.linalg.det(A), torch.linalg.inv(A)
    tx = torch.tensor(tables_1d(ntx, xi)[:2])
    ty = torch.tensor(tables_1d(nty, yi)[:2]) if dim == 2 else torch.tensor([[[1.0]], [[0.0]]], dtype=torch.float64)
    w = torch.tensor(np.outer(wy, wx).reshape(-1))
    v = torch.einsum("kj,ri->krji", ty[0], tx[0]).reshape(nty, ntx, -1)
    gref = [torch.einsum("kj,ri->krji", ty[0], tx[1]).reshape(nty, ntx, -1)]
    if dim == 2:
        gref.append(torch.einsum("kj,ri->krji", ty[1], tx[0]).reshape(nty, ntx, -1))
    gxv = torch.einsum("eqba,bkrq->ekrqa", Ainv, torch.stack(gref, dim=0))
    mu = mu_of(q, u, torch.sum(du * du, dim=2), sl)
    flux = mu[..., None] * torch.einsum("eqab,eqb->eqa", K, du)
    N = a2 * u ** 2 + a3 * u ** 3 + u * torch.sum(g * du, dim=2)
    if "ae" in coefs:
        N = N + ae * torch.exp(u)
    low = torch.sum(b * du, dim=2) + s0 * u + N
    wd = w[None, :] * det
    U = -torch.einsum("eq,eqa,ekrqa->ekr", wd, flux, gxv) + torch.einsum("eq,eq,krq->ekr", wd, low, v)
    R = U - torch.tensor(np.ascontiguousarray(p["F"][sl]))
    nax = np.full(ne, ntx) if p["nax"] is None else np.asarray(p["nax"][sl])
    nay = np.full(ne, nty) if p["nay"] is None else np.asarray(p["nay"][sl])
    mask = (np.arange(ntx)[None, None, :] < nax[:, None, None]) & (np.arange(nty)[None, :, None] < nay[:, None, None])
    R = R * torch.tensor(mask.astype(np.float64))
    if p["gram"] is None:
        loss_e = torch.sum(R * R, dim=(1, 2)) / torch.tensor((nax * nay).astype(np.float64))
    else:
        le = []
        for e in range(ne):
            r = R[e][:nay[e], :nax[e]].reshape(-1)
            le.append(torch.dot(r, torch.linalg.solve(torch.tensor(p["gram"][e]), r)))
        loss_e = torch.stack(le)
    return dict(R=R, loss_e=loss_e, lossv=torch.sum(loss_e), mask=mask)


def _channels(p, theta):
    o = vr.bare_oracle(p["prob"], p["layers"], theta)
    X = p["X"][p["eb"]:p["ee"]]
    u, du = _u_du(o, p, X.reshape(-1, p["dim"]))
    return o, u.reshape(X.shape[0], -1), du.reshape(X.shape[0], -1, p["dim"])


def terms(p, theta=None, q=None, coefs=None):
    """dict(R, loss_e, lossv, msq, triple, grad) at theta"""
    theta = p["theta"] if theta is None else np.asarray(theta, dtype=np.float64)
    o, u, du = _channels(p, theta)
    r = _loss(p, u, du, q, coefs)
    msq = torch.zeros((), dtype=torch.float64)
    if p["data"] is not None:
        ud, _ = _u_du(o, p, p["data"][0])
        msq = torch.mean((ud - torch.tensor(p["data"][1])) ** 2)
    loss = r["lossv"] + p["lbw"] * msq
    g, = torch.autograd.grad(loss, o.theta)
    Rn = r["R"].detach().numpy().copy()
    Rn[~r["mask"]] = 0.0
    lossv, msq, loss = float(r["lossv"].detach()), float(msq.detach()), float(loss.detach())
    return dict(R=Rn, loss_e=r["loss_e"].detach().numpy().copy(), lossv=lossv, msq=msq, triple=np.array([loss, msq, lossv]), grad=g.numpy().copy())


def reference(p, theta=None, **kw):
    """(loss triple, gradient, R)"""
    t = terms(p, theta, **kw)
    return t["triple"], t["grad"], t["R"]


def channel_adjoints(p, u_du=None):
    """with the channels as leaves: dict(u, du, gbar_u (ne, nq), gbar_du (ne, nq, dim)) -- d lossv / d channel, what GBAR holds"""
    if u_du is None:
        _, u, du = _channels(p, p["theta"])
    else:
        u, du = (torch.tensor(np.ascontiguousarray(v)) for v in u_du)
    u, du = u.detach().clone().requires_grad_(True), du.detach().clone().requires_grad_(True)
    r = _loss(p, u, du)
    r["lossv"].backward()
    return dict(u=u.detach().numpy().copy(), du=du.detach().numpy().copy(), gbar_u=u.grad.numpy().copy(), gbar_du=du.grad.numpy().copy())


def adam_trajectory(p, steps, lr_=1e-3, theta=None, q=None, q2=None, b1=0.9, b2=0.999, eps=1e-8):
    """`steps` TF1-Adam updates of the reference's loss under q; with q2, `steps` more under q2 with the same optimizer"""
    th = np.array(p["theta"] if theta is None else theta, dtype=np.float64)
    m, v = np.zeros_like(th), np.zeros_like(th)
    b1p, b2p = b1, b2
    for k in range(steps if q2 is None else 2 * steps):
        g = reference(p, th, q=q if k < steps else q2)[1]
        lr_t = lr_ * np.sqrt(1.0 - b2p) / (1.0 - b1p)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        th = th - lr_t * m / (np.sqrt(v) + eps)
        b1p, b2p = b1p * b1, b2p * b2
    return th


# ---- the strong residual in divergence form ----------------------------------------------------------------------------------------------
def strong(p, f=0.0, theta=None, u_du=None):
    """r [e][j][i], physical: (1 / det A) [ d/dxi (adj(A) mu K grad u)_1 + d/deta (..)_2 ] + b . grad u + s u + N - f, the flux's nodal
    interpolant differentiated by the rule's matrices; u_du: numpy channels from outside in place of the network's"""
    dim, sl = p["dim"], slice(p["eb"], p["ee"])
    if u_du is None:
        _, u, du = _channels(p, p["theta"] if theta is None else theta)
        u, du = u.detach(), du.detach()
    else:
        u, du = (torch.tensor(np.ascontiguousarray(v)) for v in u_du)
    c, ne = p["coefs"], u.shape[0]
    A = p["A"][sl]
    (xi, _), (yi, _) = p["xr"], p["yr"]
    qx, qy = xi.size, yi.size
    mu = mu_of(p["q"], u, torch.sum(du * du, dim=2), sl).numpy()
    u, du = u.numpy(), du.numpy()
    z = lambda k, sh: c[k][sl] if k in c else np.zeros((ne, qx * qy) + sh)
    flux = mu[..., None] * np.einsum("eqab,eqb->eqa", c["K"][sl], du)
    if dim == 2:
        det = A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
        adj = np.stack([np.stack([A[..., 1, 1], -A[..., 0, 1]], -1), np.stack([-A[..., 1, 0], A[..., 0, 0]], -1)], -2)
        Fh = np.einsum("eqab,eqb->eqa", adj, flux).reshape(ne, qy, qx, 2)
        div = np.einsum("im,ejm->eji", la.diff(xi), Fh[..., 0]) + np.einsum("jm,emi->eji", la.diff(yi), Fh[..., 1])
    else:
        det = A[..., 0, 0]
        div = np.einsum("im,ejm->eji", la.diff(xi), flux.reshape(ne, 1, qx))
    N = z("a2", ()) * u ** 2 + z("a3", ()) * u ** 3 + u * np.sum(z("g", (dim,)) * du, axis=2)
    if "ae" in c:
        N = N + c["ae"][sl] * np.exp(u)
    low = np.sum(z("b", (dim,)) * du, axis=2) + z("s", ()) * u + N
    f = np.broadcast_to(np.asarray(f, dtype=np.float64), u.shape)
    return div / det.reshape(ne, qy, qx) + (low - f).reshape(ne, qy, qx)


def indicators(p, r, t=None):
    """(n_owned, 5): loss_e, int r^2, sum R^2, its top rows in x and in y (divform_reference.indicators on this module's terms)"""
    t = terms(p) if t is None else t
    sl = slice(p["eb"], p["ee"])
    ne, ntx, nty = p["ee"] - p["eb"], p["ntx"], p["nty"]
    det = np.linalg.det(p["A"][sl]).reshape(r.shape)
    nax = np.full(ne, ntx) if p["nax"] is None else np.asarray(p["nax"][sl])
    nay = np.full(ne, nty) if p["nay"] is None else np.asarray(p["nay"][sl])
    out = np.zeros((ne, 5))
    for e in range(ne):
        B = t["R"][e, :nay[e], :nax[e]] ** 2
        out[e] = [t["loss_e"][e], np.einsum("j,i,ji->", p["yr"][1], p["xr"][1], det[e] * r[e] ** 2), B.sum(), B[:, nax[e] - 1].sum(),
                  B[nay[e] - 1, :].sum() if p["dim"] == 2 else 0.0]
    return out


# ---- Gram matrices of the three norms ----------------------------------------------------------------------------------------------------
def _counts(p):
    ne = p["ee"] - p["eb"]
    nax = np.full(ne, p["ntx"]) if p["nax"] is None else np.asarray(p["nax"])[p["eb"]:p["ee"]]
    nay = np.full(ne, p["nty"]) if p["nay"] is None else np.asarray(p["nay"])[p["eb"]:p["ee"]]
    return [int(v) for v in nax], [int(v) for v in nay]


def gram_table(p, mass):
    """the table norm on boxes: dualnorm_reference.gram_element per owned element"""
    nax, nay = _counts(p)
    b = np.asarray(p["boxes"], dtype=np.float64)[p["eb"]:p["ee"]]
    return [dn.gram_element(2, nax[e], nay[e], (b[e, 1] - b[e, 0]) / 2, (b[e, 3] - b[e, 2]) / 2, mass) for e in range(len(nax))]


def gram_dense(p, geom, mass, S=None):
    """the dense norms: dualdense_reference.gram_dense with geom(x, y) -> (X, A) of all elements; S None the physical H^1 product, else
    a callable of the physical points (the energy metric: K alone, symmetrised -- never mu K)"""
    nax, nay = _counts(p)
    x, w = dd.rule(p["ntx"], p["nty"])
    X, A = geom(x, x)
    return [dd.gram_dense(nax[e], nay[e], X[p["eb"] + e], A[p["eb"] + e], S, mass, x, w) for e in range(len(nax))]


# ---- what a device that runs the library's elements must be handed --------------------------------------------------------------------------
def device_planes(p):
    """(4, n_owned * NQ): the rows (m0, m1, m2, delta) of hpv_set_quasilinear -- plain, NOT times det A -- and the exponent"""
    q, sl = p["q"], slice(p["eb"], p["ee"])
    return np.stack([q["m"][sl][..., 0].reshape(-1), q["m"][sl][..., 1].reshape(-1), q["m"][sl][..., 2].reshape(-1), q["delta"][sl].reshape(-1)], 0), q["r"]


# ---- the three driver problems, restated: exact solutions and the multiplier, for the host tests ------------------------------------------
def scherk(X):
    """u = log(cos x) - log(cos y) and its gradient: the minimal-surface equation div(grad u / sqrt(1 + |grad u|^2)) = 0"""
    x, y = X[..., 0], X[..., 1]
    return np.log(np.cos(x)) - np.log(np.cos(y)), np.stack([-np.tan(x), np.tan(y)], -1)


def from_model(m, theta=None):
    """The problem dict of a live hp_vpinns_amd.vpinn.VPINNNonlinear on one rank (boxes or a MappedMesh, residual_norm="l2"), its
    coefficients evaluated here at the physical quadrature points"""
    from hp_vpinns_amd.adapt import MappedMesh
    from hp_vpinns_amd.vpinn import _coef_field, _kappa_field
    mesh, dim = m._mesh, m.layers[0]
    xr = m._rule[0]
    yr = m._rule[1] if dim == 2 else (np.zeros(1), np.ones(1))
    ne = len(mesh)
    if isinstance(mesh, MappedMesh):
        P, A = mesh.geometry(xr[0], yr[0], 0, ne)
        X, A = P.reshape(ne, -1, 2), A.reshape(ne, -1, 2, 2)
    elif dim == 2:
        X, A = mr.geom_boxes(mesh.boxes, xr[0], yr[0])
    else:
        X, A = geom_1d(mesh.boxes, xr[0])
    nq, P = X.shape[1], X.reshape(-1, dim)
    k = _kappa_field(m._op["kappa"], P, dim)
    K = k.reshape(ne, nq, dim, dim) if k.ndim == 3 else np.einsum("nqa,ab->nqab", k.reshape(ne, nq, dim), np.eye(dim))
    coefs = dict(K=K, b=_coef_field(m._op["beta"], P, dim, "beta", True).reshape(ne, nq, dim),
                 s=_coef_field(m._op["sigma"], P, dim, "sigma", False).reshape(ne, nq))
    for key, name in (("a2", "quadratic"), ("a3", "cubic"), ("ae", "exponential")):
        v = _coef_field(m._nl[name], P, dim, name, False)
        if np.any(v != 0.0):
            coefs[key] = v.reshape(ne, nq)
    g = _coef_field(m._nl["advection"], P, dim, "advection", True)
    if np.any(g != 0.0):
        coefs["g"] = g.reshape(ne, nq, dim)
    d = m._diffusivity
    mm = np.stack([_coef_field(c, P, dim, "poly", False) for c in d["poly"]], 1).reshape(ne, nq, 3)
    delta = _coef_field(d["shift"], P, dim, "shift", False).reshape(ne, nq)
    q = dict(m=mm, delta=delta, r=float(d["power"]), use_u=bool(np.any(mm != np.array([1.0, 0.0, 0.0]))), use_grad=d["power"] != 0.0)
    nt = (int(mesh.nax.max()), int(mesh.nay.max())) if dim == 2 else int(mesh.nax.max())
    counts = (mesh.nax, mesh.nay) if dim == 2 else mesh.nax
    p = problem(dim, m.layers, 0, X, A, (xr, yr), nt, coefs, q, counts=counts, boxes=None if isinstance(mesh, MappedMesh) else mesh.boxes)
    p["theta"] = np.asarray(m.get_params() if theta is None else theta, dtype=np.float64)
    from hp_vpinns_amd.testfcn import tables_1d
    f = _coef_field(m._f, P, dim, "f", False).reshape(ne, nq)                        # F[e][k][r] = sum_q w d f v_kr
    ax = tables_1d(p["ntx"], xr[0])[0] * xr[1][None, :]
    by = tables_1d(p["nty"], yr[0])[0] * yr[1][None, :] if dim == 2 else np.ones((1, 1))
    p["F"] = np.einsum("kj,ri,eji->ekr", by, ax, (np.linalg.det(A) * f).reshape(ne, yr[0].size, xr[0].size))
    p["lbw"] = m.lossb_weight
    if m.X_u_train is not None:
        p["data"] = (m.X_u_train, m.utrain)
    return p
