"""The variable-coefficient linear problems (hpv_set_operator, VPINNLinear) in fp64 on the CPU, and the case table of
tests/test_gpu_linear.py (a plain helper module like flux_reference.py; no GPU needed).  tests/test_linear_host.py proves it.

    L u = d/dx(kx u_x) + d/dy(ky u_y) + bx u_x + by u_y + s u = f                 1-D: (k u')' + b u' + s u = f
    R[e][k][r] = -(J/Jx) sum_q w kx u_x phi_r' phi_k - (J/Jy) sum_q w ky u_y phi_r phi_k' + J sum_q w (bx u_x + by u_y + s u) phi_r phi_k - F
    lossv = sum_e mean over the ACTIVE test functions of R^2,      loss = lossb_weight * lossb + lossf + lossv

  var_part    R, lossv and d lossv / d theta by torch autograd through the oracle's own `neural_net` (validation_reference.bare_oracle:
              sin network for the 1-D cases, tanh for the 2-D ones); u_x, u_y by torch.autograd.grad with respect to the points.
              Tables and rules come from hp_vpinns_amd.testfcn / quadrature.
  the rest    data_term_reference.data_part and flux_reference.flux_part, unchanged.

Inputs.  Elements: a list of boxes of unequal size inside the domain of data_term_reference; the handle owns a slice of it.  Every
coefficient plane is an independent random field with values in +-U(0.5, 1.5) (one value per quadrature point, no smoothness: the
projection does not care); F is seeded F_SCALE * N(0, 1); the parameters are generic_point.generic_theta.

Conditions on the reference alone (`conditions`), asserted before a device number is looked at:
  (a) every network block of the gradient is at least generic_point.BLOCK_FLOOR of its norm;
  (b) zeroing any one coefficient plane moves the loss by more than flux_reference.COLUMN_MOVE of it: a kernel that reads the wrong
      plane or the wrong channel cannot pass;
  (c) reading the points of an element as [qx][qy] instead of [qy][qx], or the residuals as [ntx][nty] instead of [nty][ntx], in the
      reference's own indexing moves the loss by more than the same share (2-D).
"""
import numpy as np
import torch

import data_term_reference as dr
import flux_reference as fr
import generic_point as gp
import validation_reference as vr

LBW = 3.0
F_SCALE = 0.03      # |F| of the order of the projections themselves (small elements, |w phi| < 1): at N(0, 1) the loss would be F's alone and (b) moot


def rule(q, pad=0):
    """the q-point Gauss-Lobatto rule, `pad` zero-weight points appended at the last node (the padding of vpinn._pad_rule)"""
    from hp_vpinns_amd import GaussLobattoJacobiWeights
    x, w = GaussLobattoJacobiWeights(q, 0, 0)
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return np.concatenate([x, np.full(pad, x[-1])]), np.concatenate([w, np.zeros(pad)])


def _signed(rng, shape):
    return rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)


def quad_points(boxes, xi, yi=None):
    """(n * NQ, dim), element-major, q = j * qx + i: the library's layout and its own expression of the affine map"""
    b = np.asarray(boxes, dtype=np.float64)
    X = b[:, 0:1] + (b[:, 1:2] - b[:, 0:1]) / 2 * (xi[None, :] + 1)
    if yi is None:
        return X.reshape(-1, 1)
    Y = b[:, 2:3] + (b[:, 3:4] - b[:, 2:3]) / 2 * (yi[None, :] + 1)
    n, qx, qy = b.shape[0], xi.size, yi.size
    return np.stack([np.broadcast_to(X[:, None, :], (n, qy, qx)).reshape(-1), np.broadcast_to(Y[:, :, None], (n, qy, qx)).reshape(-1)], 1)


def problem(c):
    """Everything of case dict `c` (see CASES) as arrays: dict(prob, dim, layers, theta, boxes (all), eb, ee, xr = (xi, wx), yr, ntx, nty,
    nax, nay (all elements, or None), planes (K, n_owned * NQ), F (n_total, nty, ntx), data = (X, u) | None, flux | None)"""
    rng = np.random.default_rng(c["seed"])
    dim = c["L"][0]
    prob = "p1" if dim == 1 else "p2"
    boxes = np.asarray(c["boxes"], dtype=np.float64)
    eb, ee = c.get("shard", (0, boxes.shape[0]))
    qx, qy = c["q"] if dim == 2 else (c["q"], 1)
    px, py = c.get("pad", (0, 0))
    xr = rule(qx - px, px)
    yr = rule(qy - py, py) if dim == 2 else None
    ntx, nty = c["nt"] if dim == 2 else (c["nt"], 1)
    theta = gp.generic_theta(c["L"], c["seed"])
    K = 3 if dim == 1 else 5
    planes = _signed(rng, (K, (ee - eb) * qx * qy))
    F = F_SCALE * rng.standard_normal((boxes.shape[0], nty, ntx))
    nax, nay = c.get("counts", (None, None))
    p = dict(prob=prob, dim=dim, layers=list(c["L"]), theta=theta, boxes=boxes, eb=eb, ee=ee, xr=xr, yr=yr, ntx=ntx, nty=nty,
             nax=None if nax is None else np.asarray(nax, dtype=np.int32), nay=None if nay is None else np.asarray(nay, dtype=np.int32),
             planes=planes, F=F, data=None, flux=None, lbw=LBW, act=c.get("act", "sin" if dim == 1 else "tanh"))
    if c.get("data"):
        X = dr.points(prob, c["data"], c["seed"] + 1)
        p["data"] = (X, dr.targets(prob, c["L"], theta, X, c["seed"] + 1).reshape(-1))
    if c.get("flux"):
        p["flux"] = fr.flux_data(prob, c["L"], theta, c["flux"], c["seed"] + 2)
    return p


def var_part(p, theta=None, planes=None, swap=None):
    """dict(R (n_owned, nty, ntx), loss_e, lossv, grad) of the variational term; swap 'q' / 'nt': the WRONG indexing of condition (c)"""
    from hp_vpinns_amd.testfcn import tables_1d
    theta = p["theta"] if theta is None else theta
    planes = p["planes"] if planes is None else planes
    o = vr.bare_oracle(p["prob"], p["layers"], theta)
    dim, eb, ee = p["dim"], p["eb"], p["ee"]
    b = p["boxes"][eb:ee]
    ne = ee - eb
    (xi, wx) = p["xr"]
    qx, ntx, nty = xi.size, p["ntx"], p["nty"]
    tx = torch.tensor(tables_1d(ntx, xi)[:2] * wx[None, None, :])                 # [2][ntx][qx]  w phi, w phi'
    if dim == 2:
        yi, wy = p["yr"]
        qy = yi.size
        ty = torch.tensor(tables_1d(nty, yi)[:2] * wy[None, None, :])
    else:
        yi, qy = None, 1
        ty = torch.ones((2, 1, 1), dtype=torch.float64)
    X = torch.tensor(quad_points(b, xi, yi), requires_grad=True)
    u = o.neural_net(X)
    du, = torch.autograd.grad(u.sum(), X, create_graph=True)

    def el(v):                                                    # (n_owned * NQ,) -> [e][j][i]
        if swap == "q":
            return v.reshape(ne, qx, qy).transpose(1, 2)
        return v.reshape(ne, qy, qx)
    pl = [el(torch.tensor(np.ascontiguousarray(r))) for r in planes]
    u, ux = el(u.reshape(-1)), el(du[:, 0])
    Jx = torch.tensor((b[:, 1] - b[:, 0]) / 2)
    if dim == 2:
        uy = el(du[:, 1])
        kx, ky, bx, by, s = pl
        Jy = torch.tensor((b[:, 3] - b[:, 2]) / 2)
        J = Jx * Jy
    else:
        k, bb, s = pl
        J = Jx

    def proj(G, dx, dy):                                           # [e][k][r] = sum_ji ty[dy][k][j] tx[dx][r][i] G[e][j][i]
        return torch.einsum("kj,ri,eji->ekr", ty[dy], tx[dx], G)
    if dim == 2:
        U = (-(J / Jx))[:, None, None] * proj(kx * ux, 1, 0) - (J / Jy)[:, None, None] * proj(ky * uy, 0, 1) \
            + J[:, None, None] * proj(bx * ux + by * uy + s * u, 0, 0)
    else:
        U = (-(J / Jx))[:, None, None] * proj(k * ux, 1, 0) + J[:, None, None] * proj(bb * ux + s * u, 0, 0)
    F = p["F"][eb:ee]
    if swap == "nt":
        F = F.reshape(ne, ntx, nty).transpose(0, 2, 1)
    R = U - torch.tensor(np.ascontiguousarray(F))
    nax = np.full(ne, ntx) if p["nax"] is None else p["nax"][eb:ee]
    nay = np.full(ne, nty) if p["nay"] is None else p["nay"][eb:ee]
    mask = (np.arange(ntx)[None, None, :] < nax[:, None, None]) & (np.arange(nty)[None, :, None] < nay[:, None, None])
    R = R * torch.tensor(mask.astype(np.float64))
    loss_e = torch.sum(R * R, dim=(1, 2)) / torch.tensor((nax * nay).astype(np.float64))
    lossv = torch.sum(loss_e)
    g, = torch.autograd.grad(lossv, o.theta)
    Rn = R.detach().numpy().copy()
    Rn[~mask] = 0.0                                                # (exact zeros, no -0.0)
    return dict(R=Rn, loss_e=loss_e.detach().numpy().copy(), lossv=float(lossv.detach()), grad=g.numpy().copy())


def reference(p, theta=None, planes=None):
    """(loss triple, gradient, R) of var + data + flux at `theta`"""
    theta = p["theta"] if theta is None else theta
    v = var_part(p, theta, planes)
    d = dict(wmsq=0.0, msq=0.0, grad=0.0) if p["data"] is None else dr.data_part(p["prob"], p["layers"], theta, p["data"][0], p["data"][1], p["lbw"])
    f = fr.flux_part(p["prob"], p["layers"], theta, p["flux"])
    return fr.triple(p["prob"], v["lossv"], d, f), v["grad"] + d["grad"] + f["grad"], v["R"]


def conditions(p, swaps=("q", "nt")):
    """(a) - (c) of the module docstring; returns the figures for the log.  swaps: the halves of (c) that are asked for -- exchanging
    two extents of which one is 1 is the same indexing, so a caller with such a shape leaves that half out"""
    v = var_part(p)
    _, g, _ = reference(p)
    total = np.linalg.norm(g)
    share = {k: float(np.linalg.norm(g[lo:hi]) / total) for k, lo, hi in gp.blocks(p["layers"], 0)}
    assert min(share.values()) >= gp.BLOCK_FLOOR, ("(a)", share)
    moves = []
    for i in range(p["planes"].shape[0]):
        z = p["planes"].copy()
        z[i] = 0.0
        moves.append(abs(var_part(p, planes=z)["lossv"] - v["lossv"]) / v["lossv"])
    assert min(moves) > fr.COLUMN_MOVE, ("(b)", moves)
    sw = []
    if p["dim"] == 2 and swaps:
        sw = [abs(var_part(p, swap=w)["lossv"] - v["lossv"]) / v["lossv"] for w in swaps]
        assert min(sw) > fr.COLUMN_MOVE, ("(c)", sw)
    return dict(block_share=min(share.values()), plane=min(moves), swap=min(sw) if sw else None)


def adam_trajectory(p, steps, lr=1e-3, theta=None, planes=None, b1=0.9, b2=0.999, eps=1e-8):
    """`steps` TF1-Adam updates (the rule and constants of oracle.vpinn_oracle.adam_step) of the reference's loss; returns the parameters"""
    th = np.array(p["theta"] if theta is None else theta, dtype=np.float64)
    m, v = np.zeros_like(th), np.zeros_like(th)
    b1p, b2p = b1, b2
    for _ in range(steps):
        g = reference(p, th, planes)[1]
        lr_t = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        th = th - lr_t * m / (np.sqrt(v) + eps)
        b1p, b2p = b1p * b1, b2p * b2
    return th


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# four boxes of unequal size inside [-1, 1]^2 (an L-shape plus one refined corner); the shard cases own the last three
BOXES2 = [[-1.0, -0.2, -1.0, 0.1], [-0.2, 1.0, -1.0, -0.3], [-1.0, -0.4, 0.1, 1.0], [-0.4, 0.3, 0.1, 0.55]]
BOXES1 = [[-1.0, -0.35], [-0.35, 0.5], [0.5, 1.0]]
S8, W24 = [2, 8, 8, 1], [2, 24, 24, 1]


def _c(name, L, boxes, q, nt, seed, **kw):
    return dict(name=name, L=L, boxes=boxes, q=q, nt=nt, seed=seed, **kw)


CASES = {
    "2d-h8": _c("2d-h8", S8, BOXES2[:3], (6, 5), (4, 3), 9101),
    "2d-h8-shard-data": _c("2d-h8-shard-data", S8, BOXES2, (6, 5), (4, 3), 9102, shard=(1, 4), data=19),
    "2d-h8-flux": _c("2d-h8-flux", S8, BOXES2[:3], (6, 5), (4, 3), 9103, data=19, flux=17),
    "2d-h8-counts": _c("2d-h8-counts", S8, BOXES2[:3], (6, 5), (4, 3), 9104, data=19, counts=([4, 2, 3], [1, 3, 2])),
    "2d-h24": _c("2d-h24", W24, BOXES2[:3], (6, 5), (4, 3), 9105, data=19),
    "2d-h24-counts-flux": _c("2d-h24-counts-flux", W24, BOXES2, (6, 5), (4, 3), 9106, shard=(1, 4), data=19, flux=17, counts=([3, 4, 2, 3], [2, 1, 3, 3])),
    "1d-sin": _c("1d-sin", [1, 8, 8, 1], BOXES1, 7, 4, 9107, data=2, counts=([4, 2, 3], None)),
    # the largest 2-D shape the drivers use, and a 20-point rule padded to 21 x 21 with zero-weight points (seeds: the first from 9108 on
    # whose random planes keep (b) with a margin of two -- 2000 independent signs per plane average out)
    "lds-20x20": _c("lds-20x20", S8, BOXES2[3:], (20, 20), (10, 10), 9110, data=19),
    "lds-21x21-padded": _c("lds-21x21-padded", S8, BOXES2[3:], (21, 21), (10, 10), 9111, data=19, pad=(1, 1)),
}
SMALL = [k for k in CASES if not k.startswith("lds")]


# ---- the three existing problems as special cases (tests/test_linear_host.py on the CPU, tests/test_gpu_linear.py on the device) ---
def from_setup(prob, s, L, theta, lbw, V=0.6):
    """The problem dict of a driver's setup() dict `s` (as generic_point warps it) restated in this class: Poisson-2D var_form 1 is
    k = 1, b = s = 0; AdvDiff var_form 1 at the epsilon of `theta` is kx = -eps, ky = 0, bx = V, by = 1 (network blocks only: theta
    loses its last entry); Poisson-1D var_form 2 is k = -1."""
    from hp_vpinns_amd.vpinn import _tensor_rule
    theta = np.asarray(theta, dtype=np.float64)
    if prob == "p1":
        g = np.asarray(s["grid"], dtype=np.float64)
        boxes = np.stack([g[:-1], g[1:]], 1)
        xr, yr = (np.asarray(s["X_quad_train"], dtype=np.float64)[:, 0].copy(), np.asarray(s["W_quad_train"], dtype=np.float64)[:, 0].copy()), None
        F = np.asarray(s["F_ext_total"], dtype=np.float64)
        F = F.reshape(F.shape[0], 1, -1)
        vals, data = [-1.0, 0.0, 0.0], (s["X_u_train"], s["u_train"])
    else:
        gx, gy = np.asarray(s["grid_x"], dtype=np.float64), np.asarray(s["grid_y" if prob == "p2" else "grid_t"], dtype=np.float64)
        ex, ey = np.repeat(np.arange(gx.size - 1), gy.size - 1), np.tile(np.arange(gy.size - 1), gx.size - 1)
        boxes = np.stack([gx[ex], gx[ex + 1], gy[ey], gy[ey + 1]], 1)
        Xq, Wq = (s["XY_quad_train"], s["WXY_quad_train"]) if prob == "p2" else (s["XT_quad_train"], s["WXT_quad_train"])
        xi, wx, yi, wy = _tensor_rule(Xq, Wq)
        xr, yr = (xi, wx), (yi, wy)
        ntx, nty = (int(np.max(v)) for v in s["N_testfcn_total"])
        if prob == "p2":
            F = np.asarray(s["F_ext_total"], dtype=np.float64).reshape(boxes.shape[0], nty, ntx)
            vals, data = [1.0, 1.0, 0.0, 0.0, 0.0], (s["X_u_train"], s["u_train"])
        else:
            F = np.zeros((boxes.shape[0], nty, ntx))
            vals, data = [-float(theta[-1]), 0.0, V, 1.0, 0.0], (s["XT_u_train"], s["u_train"])
            theta = theta[:-1].copy()
    ne, nq = boxes.shape[0], xr[0].size * (1 if yr is None else yr[0].size)
    planes = np.repeat(np.asarray(vals)[:, None], ne * nq, axis=1)
    return dict(prob="p1" if prob == "p1" else "p2", dim=boxes.shape[1] // 2, layers=list(L), theta=theta, boxes=boxes, eb=0, ee=ne, xr=xr, yr=yr,
                ntx=F.shape[2], nty=F.shape[1], nax=None, nay=None, planes=planes, F=F, flux=None, lbw=float(lbw),
                data=(np.asarray(data[0], dtype=np.float64), np.asarray(data[1], dtype=np.float64).reshape(-1)), act="sin" if prob == "p1" else "tanh")


SPECIAL = {      # generic-point cases of the three existing problems, in the keys tests/test_gpu_generic_point.py builds them from
    "p2": dict(name="lin-p2", prob="p2", vf=1, q=5, nt=3, nex=2, ney=2, L=[2, 8, 8, 1], seed=9201, lbw=3, F="random"),
    "adv": dict(name="lin-adv", prob="adv", vf=1, q=5, nt=3, nex=2, ney=2, L=[2, 8, 8, 1], seed=9202, lbw=3),
    "p1": dict(name="lin-p1", prob="p1", vf=2, q=7, nt=4, nex=3, ney=1, L=[1, 8, 8, 1], seed=9203, lbw=3),
}


def from_model(m, theta=None):
    """The problem dict of a live hp_vpinns_amd.vpinn.VPINNLinear (one rank): its mesh, rule, counts and data, its coefficients and f
    evaluated here at the quadrature points, F by numpy as hpv_assemble_rhs defines it, and `theta` (default: the parameters it holds now)."""
    from hp_vpinns_amd.testfcn import tables_1d
    from hp_vpinns_amd.vpinn import _coef_field
    mesh, dim = m._mesh, m.layers[0]
    xr, yr = m._rule[0], (m._rule[1] if dim == 2 else None)
    ntx, nty = int(mesh.nax.max()), int(mesh.nay.max())
    P = quad_points(mesh.boxes, xr[0], None if yr is None else yr[0])
    k, b = _coef_field(m._op["kappa"], P, dim, "kappa", True), _coef_field(m._op["beta"], P, dim, "beta", True)
    s, f = _coef_field(m._op["sigma"], P, dim, "sigma", False), _coef_field(m._f, P, dim, "f", False)
    ne, qx, qy = len(mesh), xr[0].size, 1 if yr is None else yr[0].size
    ax = tables_1d(ntx, xr[0])[0] * xr[1][None, :]
    by = np.ones((1, 1)) if yr is None else tables_1d(nty, yr[0])[0] * yr[1][None, :]
    J = np.prod((mesh.boxes[:, 1::2] - mesh.boxes[:, 0::2]) / 2, axis=1)
    F = J[:, None, None] * np.einsum("kj,ri,eji->ekr", by, ax, f.reshape(ne, qy, qx))
    ragged = bool(np.any(mesh.nax != ntx) or np.any(mesh.nay != nty))
    return dict(prob="p1" if dim == 1 else "p2", dim=dim, layers=list(m.layers), theta=m.get_params() if theta is None else np.asarray(theta, dtype=np.float64), boxes=mesh.boxes.copy(), eb=0, ee=ne,
                xr=xr, yr=yr, ntx=ntx, nty=nty, nax=mesh.nax.copy() if ragged else None, nay=mesh.nay.copy() if ragged and dim == 2 else None,
                planes=np.concatenate([k.T, b.T, s[None, :]], axis=0), F=F, flux=None, lbw=float(m.lossb_weight),
                data=None if m.X_u_train is None else (m.X_u_train, m.utrain), act="sin" if dim == 1 else "tanh")
