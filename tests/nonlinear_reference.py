"""The nonlinear terms on the variable-coefficient class (hpv_set_nonlinear, k_project_nl, VPINNNonlinear) in fp64 on the CPU, and the
case table of tests/test_gpu_nonlinear.py (a plain helper module like linear_reference.py, which it extends; no GPU needed).
tests/test_nonlinear_host.py proves it.

    L u + N(x; u, grad u) = f        N = a2 u^2 + a3 u^3 + ae exp(u) + u (gx u_x + gy u_y)         1-D: ... + g u u_x
    R[e][k][r] = linear_reference's  +  J sum_q w N phi_r phi_k              (N joins the (0, 0) integrand; nothing else changes)

  var_part    R, lossv and d lossv / d theta by torch autograd through the oracle's own `neural_net` (validation_reference.bare_oracle),
              exactly as linear_reference.var_part does it, with N added to the integrand that is projected against phi_r phi_k.
  channel_adjoints   the same loss from the channels u, u_x, (u_y) as leaves: autograd's d lossv / d channel and d lossv / d G_t.
  the rest    data_term_reference.data_part and flux_reference.flux_part, unchanged.

Inputs: linear_reference.problem's (same seeds, same draws) plus the planes `nl` (M, n_owned * NQ), M = 4 (a2, a3, ae, g) in 1-D and
5 (a2, a3, ae, gx, gy) in 2-D, each present one an independent field with values in +-U(0.5, 1.5) from a generator of its own
(seed + 7); a case may list the terms present (`terms`, of "u2", "u3", "exp", "adv"), the others are zero planes.

Conditions on the reference alone (`conditions`), asserted before a device number is looked at: linear_reference's (a) - (c), stated
on THIS reference (the loss with N in it), and
  (d) zeroing any one present nonlinear plane moves lossv by more than flux_reference.COLUMN_MOVE of it: a kernel that skips a term,
      reads the wrong plane for it or multiplies the wrong channel cannot pass.
Seeds: the first from the case's starting one (9301, 9311, ... per row) that keeps (a) - (c) and, with a margin of two, (d) -- as
linear_reference documents for lds-20x20.
"""
import numpy as np
import torch

import data_term_reference as dr
import flux_reference as fr
import generic_point as gp
import linear_reference as lr
import validation_reference as vr

TERMS = ("u2", "u3", "exp", "adv")


def term_rows(dim):
    """the rows of `nl` each term owns"""
    return {"u2": [0], "u3": [1], "exp": [2], "adv": [3] if dim == 1 else [3, 4]}


def problem(c):
    """linear_reference.problem(c) plus nl (M, n_owned * NQ) and terms (the present ones, in TERMS' order)"""
    p = lr.problem(c)
    rng = np.random.default_rng(c["seed"] + 7)
    M = 4 if p["dim"] == 1 else 5
    nl = lr._signed(rng, (M, p["planes"].shape[1]))
    terms = tuple(t for t in TERMS if t in c.get("terms", TERMS))
    rows = term_rows(p["dim"])
    for t in TERMS:
        if t not in terms:
            nl[rows[t]] = 0.0
    p["nl"], p["terms"] = nl, terms
    return p


def _tables(p):
    from hp_vpinns_amd.testfcn import tables_1d
    xi, wx = p["xr"]
    tx = torch.tensor(tables_1d(p["ntx"], xi)[:2] * wx[None, None, :])                 # [2][ntx][qx]  w phi, w phi'
    if p["dim"] == 2:
        yi, wy = p["yr"]
        return tx, torch.tensor(tables_1d(p["nty"], yi)[:2] * wy[None, None, :])
    return tx, torch.ones((2, 1, 1), dtype=torch.float64)


def _loss_from_channels(p, ch, planes, nl, swap=None):
    """ch = [u, u_x(, u_y)] as (n_owned * NQ,) tensors -> dict(R (masked), loss_e, lossv, mask, G = [G0, G1(, G2)] as [e][j][i])"""
    dim, eb, ee = p["dim"], p["eb"], p["ee"]
    b = p["boxes"][eb:ee]
    ne = ee - eb
    qx, ntx, nty = p["xr"][0].size, p["ntx"], p["nty"]
    qy = p["yr"][0].size if dim == 2 else 1
    tx, ty = _tables(p)

    def el(v):                                                    # (n_owned * NQ,) -> [e][j][i]
        if swap == "q":
            return v.reshape(ne, qx, qy).transpose(1, 2)
        return v.reshape(ne, qy, qx)
    pl = [el(torch.tensor(np.ascontiguousarray(r))) for r in planes]
    a2, a3, ae = (el(torch.tensor(np.ascontiguousarray(r))) for r in nl[:3])
    g = [el(torch.tensor(np.ascontiguousarray(r))) for r in nl[3:]]
    u, ux = el(ch[0]), el(ch[1])
    Jx = torch.tensor((b[:, 1] - b[:, 0]) / 2)
    N = a2 * u ** 2 + a3 * u ** 3 + ae * torch.exp(u) + u * g[0] * ux
    if dim == 2:
        uy = el(ch[2])
        N = N + u * g[1] * uy
        kx, ky, bx, by, s = pl
        Jy = torch.tensor((b[:, 3] - b[:, 2]) / 2)
        J = Jx * Jy
        G = [bx * ux + by * uy + s * u + N, kx * ux, ky * uy]
    else:
        k, bb, s = pl
        J = Jx
        G = [bb * ux + s * u + N, k * ux]

    def proj(Gt, dx, dy):                                          # [e][k][r] = sum_ji ty[dy][k][j] tx[dx][r][i] G[e][j][i]
        return torch.einsum("kj,ri,eji->ekr", ty[dy], tx[dx], Gt)
    if dim == 2:                                                   # (the order of linear_reference.var_part: equal bits at N = 0)
        U = (-(J / Jx))[:, None, None] * proj(G[1], 1, 0) - (J / Jy)[:, None, None] * proj(G[2], 0, 1) + J[:, None, None] * proj(G[0], 0, 0)
    else:
        U = (-(J / Jx))[:, None, None] * proj(G[1], 1, 0) + J[:, None, None] * proj(G[0], 0, 0)
    F = p["F"][eb:ee]
    if swap == "nt":
        F = F.reshape(ne, ntx, nty).transpose(0, 2, 1)
    R = U - torch.tensor(np.ascontiguousarray(F))
    nax = np.full(ne, ntx) if p["nax"] is None else p["nax"][eb:ee]
    nay = np.full(ne, nty) if p["nay"] is None else p["nay"][eb:ee]
    mask = (np.arange(ntx)[None, None, :] < nax[:, None, None]) & (np.arange(nty)[None, :, None] < nay[:, None, None])
    R = R * torch.tensor(mask.astype(np.float64))
    loss_e = torch.sum(R * R, dim=(1, 2)) / torch.tensor((nax * nay).astype(np.float64))
    return dict(R=R, loss_e=loss_e, lossv=torch.sum(loss_e), mask=mask, G=G)


def _channels(p, theta):
    o = vr.bare_oracle(p["prob"], p["layers"], theta)
    b = p["boxes"][p["eb"]:p["ee"]]
    X = torch.tensor(lr.quad_points(b, p["xr"][0], p["yr"][0] if p["dim"] == 2 else None), requires_grad=True)
    u = o.neural_net(X)
    du, = torch.autograd.grad(u.sum(), X, create_graph=True)
    return o, [u.reshape(-1)] + [du[:, d] for d in range(p["dim"])]


def var_part(p, theta=None, planes=None, nl=None, swap=None):
    """dict(R (n_owned, nty, ntx), loss_e, lossv, grad) of the variational term; swap 'q' / 'nt': the WRONG indexing of condition (c)"""
    theta = p["theta"] if theta is None else theta
    o, ch = _channels(p, theta)
    r = _loss_from_channels(p, ch, p["planes"] if planes is None else planes, p["nl"] if nl is None else nl, swap)
    g, = torch.autograd.grad(r["lossv"], o.theta)
    Rn = r["R"].detach().numpy().copy()
    Rn[~r["mask"]] = 0.0                                           # (exact zeros, no -0.0)
    return dict(R=Rn, loss_e=r["loss_e"].detach().numpy().copy(), lossv=float(r["lossv"].detach()), grad=g.numpy().copy())


def channel_adjoints(p):
    """At p's parameters, with the channels as leaves: dict(ch = [u, u_x(, u_y)], gbar = autograd's d lossv / d channel, g = d lossv / d G_t),
    all numpy (n_owned * NQ,) in the library's point order"""
    _, ch = _channels(p, p["theta"])
    ch = [c.detach().clone().requires_grad_(True) for c in ch]
    r = _loss_from_channels(p, ch, p["planes"], p["nl"])
    for G in r["G"]:
        G.retain_grad()
    r["lossv"].backward()
    return dict(ch=[c.detach().numpy().copy() for c in ch], gbar=[c.grad.numpy().copy() for c in ch],
                g=[G.grad.reshape(-1).numpy().copy() for G in r["G"]])


def reference(p, theta=None, planes=None, nl=None):
    """(loss triple, gradient, R) of var + data + flux at `theta`"""
    theta = p["theta"] if theta is None else theta
    v = var_part(p, theta, planes, nl)
    d = dict(wmsq=0.0, msq=0.0, grad=0.0) if p["data"] is None else dr.data_part(p["prob"], p["layers"], theta, p["data"][0], p["data"][1], p["lbw"])
    f = fr.flux_part(p["prob"], p["layers"], theta, p["flux"])
    return fr.triple(p["prob"], v["lossv"], d, f), v["grad"] + d["grad"] + f["grad"], v["R"]


def conditions(p, margin=1.0, swaps=("q", "nt")):
    """(a) - (d) of the module docstring; returns the figures for the log.  margin: the factor (d) is kept by (the seed search uses 2);
    swaps: the halves of (c) that are asked for, as in linear_reference.conditions"""
    v = var_part(p)
    _, g, _ = reference(p)
    total = np.linalg.norm(g)
    share = {k: float(np.linalg.norm(g[lo:hi]) / total) for k, lo, hi in gp.blocks(p["layers"], 0)}
    assert min(share.values()) >= gp.BLOCK_FLOOR, ("(a)", share)

    def move(**kw):
        return abs(var_part(p, **kw)["lossv"] - v["lossv"]) / v["lossv"]
    moves = []
    for i in range(p["planes"].shape[0]):
        z = p["planes"].copy()
        z[i] = 0.0
        moves.append(move(planes=z))
    assert min(moves) > fr.COLUMN_MOVE, ("(b)", moves)
    sw = []
    if p["dim"] == 2 and swaps:
        sw = [move(swap=w) for w in swaps]
        assert min(sw) > fr.COLUMN_MOVE, ("(c)", sw)
    nlm = {}
    rows = term_rows(p["dim"])
    for t in p["terms"]:
        for i in rows[t]:
            z = p["nl"].copy()
            z[i] = 0.0
            nlm["%s[%d]" % (t, i)] = move(nl=z)
    assert nlm and min(nlm.values()) > margin * fr.COLUMN_MOVE, ("(d)", nlm)
    return dict(block_share=min(share.values()), plane=min(moves), swap=min(sw) if sw else None, nl=min(nlm.values()))


def adam_trajectory(p, steps, lr_=1e-3, theta=None, planes=None, nl=None, nl2=None, b1=0.9, b2=0.999, eps=1e-8):
    """`steps` TF1-Adam updates (the rule and constants of oracle.vpinn_oracle.adam_step) of the reference's loss under `nl`; with nl2,
    `steps` more under nl2 with the same optimizer (one rule over both calls); returns the parameters"""
    th = np.array(p["theta"] if theta is None else theta, dtype=np.float64)
    m, v = np.zeros_like(th), np.zeros_like(th)
    b1p, b2p = b1, b2
    for k in range(steps if nl2 is None else 2 * steps):
        g = reference(p, th, planes, nl if k < steps else nl2)[1]
        lr_t = lr_ * np.sqrt(1.0 - b2p) / (1.0 - b1p)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        th = th - lr_t * m / (np.sqrt(v) + eps)
        b1p, b2p = b1p * b1, b2p * b2
    return th


# ---- the case table: the smallest shapes at which the kernel can still go wrong ---------------------------------------------------------
_c, S8, W24, B2, B1 = lr._c, lr.S8, lr.W24, lr.BOXES2, lr.BOXES1

CASES = {
    "2d-h8": _c("2d-h8", S8, B2[:3], (6, 5), (4, 3), 9301),
    "2d-h8-shard-data": _c("2d-h8-shard-data", S8, B2, (6, 5), (4, 3), 9311, shard=(1, 4), data=19),        # the element offset into planes and F
    "2d-h8-counts-flux": _c("2d-h8-counts-flux", S8, B2[:3], (6, 5), (4, 3), 9322, data=19, flux=17, counts=([4, 2, 3], [1, 3, 2])),
    "2d-h24": _c("2d-h24", W24, B2[:3], (6, 5), (4, 3), 9331, data=19),                                   # the MFMA wide kernels around it
    "1d-sin": _c("1d-sin", [1, 8, 8, 1], B1, 7, 4, 9342, data=2, counts=([4, 2, 3], None)),
    # one term alone: each branch of the mask
    "only-u2": _c("only-u2", S8, B2[:3], (6, 5), (4, 3), 9351, terms=("u2",)),
    "only-u3": _c("only-u3", S8, B2[:3], (6, 5), (4, 3), 9361, terms=("u3",)),
    "only-exp": _c("only-exp", S8, B2[:3], (6, 5), (4, 3), 9371, terms=("exp",)),
    "only-adv": _c("only-adv", S8, B2[:3], (6, 5), (4, 3), 9382, terms=("adv",)),
    # the LDS maximum and the padding invariant: a 20-point rule padded to 21 x 21 with zero-weight points, 10 x 10 functions, one box
    # (the first seed from 9391 on that keeps (b) and, with a margin of two, (d): 2000 independent signs per plane average out)
    "lds-21x21-padded": _c("lds-21x21-padded", S8, B2[3:], (21, 21), (10, 10), 9403, data=19, pad=(1, 1)),
}
SMALL = [k for k in CASES if not k.startswith("lds")]


def from_model(m, theta=None):
    """The problem dict of a live hp_vpinns_amd.vpinn.VPINNNonlinear (one rank): linear_reference.from_model's plus its nonlinear
    coefficients evaluated here at the quadrature points"""
    from hp_vpinns_amd.vpinn import _coef_field
    p = lr.from_model(m, theta)
    mesh, dim = m._mesh, m.layers[0]
    P = lr.quad_points(mesh.boxes, p["xr"][0], None if p["yr"] is None else p["yr"][0])
    a = [_coef_field(m._nl[k], P, dim, k, False) for k in ("quadratic", "cubic", "exponential")]
    g = _coef_field(m._nl["advection"], P, dim, "advection", True)
    p["nl"] = np.concatenate([np.stack(a, 0), g.T], axis=0)
    rows = term_rows(dim)
    p["terms"] = tuple(t for t in TERMS if np.any(p["nl"][rows[t]] != 0.0))
    return p
