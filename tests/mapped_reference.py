"""Mapped elements and the full diffusion tensor (hpv_set_element_points, hpv_set_operator_tensor, adapt.MappedMesh) in fp64 on the CPU
(a plain helper module like linear_reference.py; no GPU needed).  tests/test_mapped_host.py proves it.

The residual is built in PHYSICAL terms and nothing else: with A = d(x, y) / d(xi, eta) the Jacobian of the element map at a quadrature
point, d = det A, and v_kr(xi, eta) = phi_r(xi) phi_k(eta) the test functions on the reference square,

    grad_x v = A^-T grad_ref v
    R[e][k][r] = sum_q w_q d_q [ -(K grad u) . grad_x v_kr + (b . grad u + s u + N(u, grad u)) v_kr ] - F[e][k][r]
    N = a2 u^2 + a3 u^3 + ae exp(u) + u (g . grad u)

with K (2 x 2, not necessarily symmetric), b, s, a2, a3, ae, g the PHYSICAL coefficients at the physical points, u and grad u the
network's (through the ansatz u = G + D N where there is one), and with trainable scalars c_m every coefficient is base + sum_m c_m D_m.
An axis-parallel box is the map with A = diag(Jx, Jy): the tensor operator on boxes is the same code.  K_eff = adj(A) K is never
formed and nothing of the product's folding (vpinn.VPINNLinear._fold) or geometry (adapt.MappedMesh) is imported: the geometry
of boxes, bilinear quadrilaterals and polar boxes is restated here.

    lossv = sum_e mean over the ACTIVE test functions of R^2     (dual norm, boxes only: R_e^T G_e^-1 R_e, dualnorm_reference.gram_element)
    loss triple = (lossv + lbw msq + w_f msf, msq, lossv)        (flux_reference.triple for the 2-D class)
"""
import numpy as np
import torch

import flux_reference as fr
import generic_point as gp
import linear_reference as lr
import validation_reference as vr

LBW = lr.LBW
F_SCALE = lr.F_SCALE


# ---- geometry, restated: X (ne, NQ, 2) physical points and A (ne, NQ, 2, 2) = d x_a / d ref_b, q = j * qx + i ---------------------------
def _ref_nodes(xi, yi):
    S, T = np.meshgrid(xi, yi)                           # [j][i]: s = xi[i], t = yi[j]
    return S.reshape(-1), T.reshape(-1)


def geom_boxes(boxes, xi, yi):
    b = np.asarray(boxes, dtype=np.float64)
    s, t = _ref_nodes(xi, yi)
    hx, hy = (b[:, 1] - b[:, 0]) / 2, (b[:, 3] - b[:, 2]) / 2
    X = np.stack([b[:, 0:1] + hx[:, None] * (s[None, :] + 1), b[:, 2:3] + hy[:, None] * (t[None, :] + 1)], axis=2)
    A = np.zeros(X.shape + (2,))
    A[:, :, 0, 0], A[:, :, 1, 1] = hx[:, None], hy[:, None]
    return X, A


def geom_quads(corners, xi, yi):
    """bilinear maps of [-1, 1]^2; corners (ne, 4, 2) counter-clockwise from the image of (-1, -1)"""
    c = np.asarray(corners, dtype=np.float64)
    s, t = _ref_nodes(xi, yi)
    X = np.zeros((c.shape[0], s.size, 2))
    A = np.zeros((c.shape[0], s.size, 2, 2))
    for k, (sk, tk) in enumerate([(-1, -1), (1, -1), (1, 1), (-1, 1)]):
        X += ((1 + sk * s) * (1 + tk * t) / 4)[None, :, None] * c[:, None, k, :]
        A[:, :, :, 0] += (sk * (1 + tk * t) / 4)[None, :, None] * c[:, None, k, :]
        A[:, :, :, 1] += ((1 + sk * s) * tk / 4)[None, :, None] * c[:, None, k, :]
    return X, A


def geom_polar(rt_boxes, xi, yi):
    """x = r cos th, y = r sin th on boxes (r0, r1, th0, th1) of the (r, theta) plane"""
    P, B = geom_boxes(rt_boxes, xi, yi)
    r, th = P[:, :, 0], P[:, :, 1]
    X = np.stack([r * np.cos(th), r * np.sin(th)], axis=2)
    A = np.zeros(X.shape + (2,))
    A[:, :, 0, 0], A[:, :, 0, 1] = np.cos(th) * B[:, :, 0, 0], -r * np.sin(th) * B[:, :, 1, 1]
    A[:, :, 1, 0], A[:, :, 1, 1] = np.sin(th) * B[:, :, 0, 0], r * np.cos(th) * B[:, :, 1, 1]
    return X, A


def polar_map(P):
    """the global map of adapt.MappedMesh(map=) for geom_polar: (X (n, 2), A (n, 2, 2))"""
    r, t = P[:, 0], P[:, 1]
    return (np.stack([r * np.cos(t), r * np.sin(t)], 1),
            np.stack([np.stack([np.cos(t), -r * np.sin(t)], 1), np.stack([np.sin(t), r * np.cos(t)], 1)], 1))


# ---- the problem dict -----------------------------------------------------------------------------------------------------------------
COEF_KEYS = ("K", "b", "s", "a2", "a3", "ae", "g")      # shapes (ne, NQ, 2, 2), (ne, NQ, 2), (ne, NQ), .., (ne, NQ, 2)


def _signed(rng, shape):
    return rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)


def random_coefs(rng, ne, nq, terms=(), diagonal=False):
    """independent random fields with values in +-U(0.5, 1.5): K non-symmetric (diagonal: kxy = kyx = 0), b, s, and the nonlinear
    terms named in `terms` ("u2", "u3", "exp", "adv"); exp gets +-U(0.05, 0.15) so that it does not drown the rest"""
    c = dict(K=_signed(rng, (ne, nq, 2, 2)), b=_signed(rng, (ne, nq, 2)), s=_signed(rng, (ne, nq)))
    if diagonal:
        c["K"][:, :, 0, 1] = c["K"][:, :, 1, 0] = 0.0
    for key, name in (("a2", "u2"), ("a3", "u3"), ("ae", "exp")):
        if name in terms:
            c[key] = _signed(rng, (ne, nq)) * (0.1 if name == "exp" else 1.0)
    if "adv" in terms:
        c["g"] = _signed(rng, (ne, nq, 2))
    return c


def problem(layers, seed, X, A, rule_x, rule_y, nt, coefs, counts=None, dirs=(), c0=(), data=0, flux=0, ansatz=None, mass=None,
            boxes=None, shard=None):
    """X, A: the geometry of ALL elements; coefs / dirs: dicts over COEF_KEYS of all elements; shard (eb, ee): the owned slice.
    F (n_total, nty, ntx) is seeded F_SCALE * N(0, 1).  mass: the dual norm's (boxes must then be given)."""
    rng = np.random.default_rng(seed + 7)
    ne = X.shape[0]
    eb, ee = shard or (0, ne)
    ntx, nty = nt
    theta = gp.generic_theta(layers, seed)
    nax, nay = counts or (None, None)
    p = dict(prob="p2", dim=2, layers=list(layers), theta=theta, c0=np.asarray(c0, dtype=np.float64), X=X, A=A, eb=eb, ee=ee,
             xr=rule_x, yr=rule_y, ntx=ntx, nty=nty, nax=None if nax is None else np.asarray(nax, dtype=np.int32),
             nay=None if nay is None else np.asarray(nay, dtype=np.int32), coefs=coefs, dirs=list(dirs),
             F=F_SCALE * rng.standard_normal((ne, nty, ntx)), data=None, flux=None, ansatz=ansatz, mass=mass, boxes=boxes, lbw=LBW, act="tanh")
    lo, hi = X.reshape(-1, 2).min(0), X.reshape(-1, 2).max(0)
    if data:
        Xd = lo + (hi - lo) * rng.uniform(size=(data, 2))
        p["data"] = (Xd, rng.uniform(-1.0, 1.0, data))
    if flux:
        Xf = lo + (hi - lo) * rng.uniform(size=(flux, 2))
        p["flux"] = dict(X=Xf, a=_signed(rng, flux), b=_signed(rng, (flux, 2)), g=rng.uniform(-1.0, 1.0, flux))
    return p


def full0(p):
    return np.concatenate([p["theta"], p["c0"]])


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def _u_du(o, p, Xn):
    """u (n,), grad u (n, 2) at the points Xn through the ansatz u = G + D N where p has one"""
    if p.get("u_fn") is not None:                         # (a given function in the network's place: the patch test)
        return p["u_fn"](torch.tensor(np.ascontiguousarray(Xn)))
    Xt = torch.tensor(np.ascontiguousarray(Xn), requires_grad=True)
    N = o.neural_net(Xt).reshape(-1)
    dN, = torch.autograd.grad(N.sum(), Xt, create_graph=True)
    if p["ansatz"] is None:
        return N, dN
    def field(c):                                        # (n, 3): a callable's value and gradient, or a constant
        return np.asarray(c(Xn), dtype=np.float64) if callable(c) else np.concatenate([np.full((Xn.shape[0], 1), float(c)), np.zeros((Xn.shape[0], 2))], 1)
    G, D = (torch.tensor(field(p["ansatz"][k])) for k in ("g", "d"))
    return G[:, 0] + D[:, 0] * N, G[:, 1:] + D[:, 1:] * N[:, None] + D[:, 0:1] * dN


def terms(p, full=None, coefs=None, X=None, A=None):
    """dict(R, loss_e, lossv, msq, msf, triple, grad) at `full` = [theta | c]; coefs / X / A override p's (all elements)"""
    from hp_vpinns_amd.testfcn import tables_1d
    full = full0(p) if full is None else np.asarray(full, dtype=np.float64)
    P = full.size - len(p["dirs"])
    o = vr.bare_oracle("p2", p["layers"], full[:P])
    c = torch.tensor(full[P:], requires_grad=True)
    eb, ee = p["eb"], p["ee"]
    ne = ee - eb
    X = (p["X"] if X is None else X)[eb:ee]
    A = torch.tensor((p["A"] if A is None else A)[eb:ee])
    coefs = p["coefs"] if coefs is None else coefs
    (xi, wx), (yi, wy) = p["xr"], p["yr"]
    qx, qy, ntx, nty = xi.size, yi.size, p["ntx"], p["nty"]
    u, du = _u_du(o, p, X.reshape(-1, 2))
    u, du = u.reshape(ne, -1), du.reshape(ne, -1, 2)

    def field(key, shape):
        v = torch.tensor(coefs[key][eb:ee]) if key in coefs else torch.zeros((ne, qx * qy) + shape, dtype=torch.float64)
        for m, d in enumerate(p["dirs"]):
            if key in d:
                v = v + c[m] * torch.tensor(d[key][eb:ee])
        return v
    K, b, s = field("K", (2, 2)), field("b", (2,)), field("s", ())
    a2, a3, ae, g = field("a2", ()), field("a3", ()), field("ae", ()), field("g", (2,))
    det = A[:, :, 0, 0] * A[:, :, 1, 1] - A[:, :, 0, 1] * A[:, :, 1, 0]
    Ainv = torch.linalg.inv(A)
    tx, ty = torch.tensor(tables_1d(ntx, xi)[:2]), torch.tensor(tables_1d(nty, yi)[:2])       # [2][n][q]: phi, phi' (no weights)
    w = torch.tensor(np.outer(wy, wx).reshape(-1))
    v = torch.einsum("kj,ri->krji", ty[0], tx[0]).reshape(nty, ntx, -1)                           # v_kr at q = j * qx + i
    gref = torch.stack([torch.einsum("kj,ri->krji", ty[0], tx[1]).reshape(nty, ntx, -1),
                        torch.einsum("kj,ri->krji", ty[1], tx[0]).reshape(nty, ntx, -1)], dim=0)  # [b][k][r][q]
    gxv = torch.einsum("eqba,bkrq->ekrqa", Ainv, gref)                                             # grad_x v = A^-T grad_ref v
    flux = torch.einsum("eqab,eqb->eqa", K, du)                                                   # K grad u
    N = a2 * u ** 2 + a3 * u ** 3 + ae * torch.exp(u) + u * torch.sum(g * du, dim=2)
    low = torch.sum(b * du, dim=2) + s * u + N
    wd = w[None, :] * det
    U = -torch.einsum("eq,eqa,ekrqa->ekr", wd, flux, gxv) + torch.einsum("eq,eq,krq->ekr", wd, low, v)
    R = U - torch.tensor(np.ascontiguousarray(p["F"][eb:ee]))
    nax = np.full(ne, ntx) if p["nax"] is None else p["nax"][eb:ee]
    nay = np.full(ne, nty) if p["nay"] is None else p["nay"][eb:ee]
    mask = (np.arange(ntx)[None, None, :] < nax[:, None, None]) & (np.arange(nty)[None, :, None] < nay[:, None, None])
    R = R * torch.tensor(mask.astype(np.float64))
    if p["mass"] is None:
        loss_e = torch.sum(R * R, dim=(1, 2)) / torch.tensor((nax * nay).astype(np.float64))
    else:
        import dualnorm_reference as dn
        bx = p["boxes"][eb:ee]
        le = []
        for e in range(ne):
            r = R[e][:nay[e], :nax[e]].reshape(-1)
            G = torch.tensor(dn.gram_element(2, int(nax[e]), int(nay[e]), (bx[e, 1] - bx[e, 0]) / 2, (bx[e, 3] - bx[e, 2]) / 2, p["mass"]))
            le.append(torch.dot(r, torch.linalg.solve(G, r)))
        loss_e = torch.stack(le)
    lossv = torch.sum(loss_e)
    msq = msf = torch.zeros((), dtype=torch.float64)
    if p["data"] is not None:
        ud, _ = _u_du(o, p, p["data"][0])
        msq = torch.mean((ud - torch.tensor(p["data"][1])) ** 2)
    if p["flux"] is not None:
        f = p["flux"]
        uf, duf = _u_du(o, p, f["X"])
        msf = torch.mean((torch.tensor(f["a"]) * uf + torch.sum(torch.tensor(f["b"]) * duf, dim=1) - torch.tensor(f["g"])) ** 2)
    loss = lossv + p["lbw"] * msq + fr.W_F * msf
    if p.get("u_fn") is not None:                         # (nothing depends on the parameters)
        gt, gc = torch.zeros_like(o.theta), None
    else:
        gt, gc = torch.autograd.grad(loss, [o.theta, c], allow_unused=True)
    gc = np.zeros(0) if gc is None else gc.numpy()
    lossv, msq, msf, loss = (t.detach() for t in (lossv, msq, msf, loss))
    Rn = R.detach().numpy().copy()
    Rn[~mask] = 0.0
    return dict(R=Rn, loss_e=loss_e.detach().numpy().copy(), lossv=float(lossv), msq=float(msq), msf=float(msf),
                triple=np.array([float(loss), float(msq), float(lossv)]), grad=np.concatenate([gt.numpy(), gc]))


def reference(p, full=None, **kw):
    """(loss triple, gradient [d theta | d c], R)"""
    t = terms(p, full, **kw)
    return t["triple"], t["grad"], t["R"]


def adam_trajectory(p, steps, lr_=1e-3, full=None, b1=0.9, b2=0.999, eps=1e-8):
    """`steps` TF1-Adam updates (the rule and constants of oracle.vpinn_oracle.adam_step) of the reference's loss; returns [theta | c]"""
    th = np.array(full0(p) if full is None else full, dtype=np.float64)
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


# ---- the fold, in numpy: what a device that runs UNIT elements must be handed (tests/test_mapped_host.py, tests/test_gpu_mapped.py) -------
def fold(A, c):
    """dict over COEF_KEYS: K_eff = adj(A) K, everything else times det A -- stated here a second time, for the tests' device inputs
    and for the host test that the box formula on the folded planes IS the physical reference"""
    det = A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
    M = np.stack([np.stack([A[..., 1, 1], -A[..., 0, 1]], -1), np.stack([-A[..., 1, 0], A[..., 0, 0]], -1)], -2)
    out = {}
    for k, v in c.items():
        out[k] = M @ v if k == "K" else v * (det[..., None] if v.ndim == det.ndim + 1 else det)
    return out


def unit_geometry(X):
    """the geometry of unit elements at the points X: A = I"""
    A = np.zeros(X.shape + (2,))
    A[..., 0, 0] = A[..., 1, 1] = 1.0
    return A


def operator_planes(c, eb, ee, tensor=True):
    """(7 | 5, n_owned * NQ): the rows of hpv_set_operator_tensor (hpv_set_operator for a diagonal K)"""
    K, b, s = (c[k][eb:ee] for k in ("K", "b", "s"))
    kr = [K[..., 0, 0], K[..., 0, 1], K[..., 1, 0], K[..., 1, 1]] if tensor else [K[..., 0, 0], K[..., 1, 1]]
    return np.stack([r.reshape(-1) for r in kr + [b[..., 0], b[..., 1], s]], 0)


def nonlinear_planes(c, eb, ee):
    """(5, n_owned * NQ): the rows (a2, a3, ae, gx, gy) of hpv_set_nonlinear, zeros where a term is absent"""
    n = c["s"][eb:ee].size
    z = np.zeros(n)
    g = c["g"][eb:ee] if "g" in c else np.zeros(c["s"][eb:ee].shape + (2,))
    return np.stack([c[k][eb:ee].reshape(-1) if k in c else z for k in ("a2", "a3", "ae")] + [g[..., 0].reshape(-1), g[..., 1].reshape(-1)], 0)


def direction_planes(d, like, eb, ee, tensor=True):
    """(7 + 5 | 5 + 5, n_owned * NQ) of one direction dict (absent keys are zero)"""
    z = {k: np.zeros_like(like[k]) for k in ("K", "b", "s")}
    z.update(d)
    return np.concatenate([operator_planes(z, eb, ee, tensor), nonlinear_planes(z, eb, ee)], 0)
