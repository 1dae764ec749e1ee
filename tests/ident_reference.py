"""Coefficient identification on the variable-coefficient class (hpv_create_ex, hpv_set_trainable, k_project_id, VPINNLinear /
VPINNNonlinear(trainable=...)) in fp64 on the CPU, and the case table of tests/test_gpu_ident.py (a plain helper module like
nonlinear_reference.py, which it extends; no GPU needed).  tests/test_ident_host.py proves it.

    plane_p = base_p + sum_m c_m D_m,p        p over (k, b, s | kx, ky, bx, by, s) then (a2, a3, ae, g | a2, a3, ae, gx, gy)
    R, lossv: nonlinear_reference's on these planes;  the parameter vector is [theta | c_0 .. c_{nc-1}]

  var_part    the loss of nonlinear_reference._loss_from_channels restated on torch planes, with the coefficients c as torch LEAVES:
              d lossv / d theta and d lossv / d c by autograd.
  the rest    data_term_reference.data_part and flux_reference.flux_part, unchanged: they add nothing to the coefficients' gradient.

Inputs: nonlinear_reference.problem's (same seeds, same draws) plus `dirs` (nc, K + M, n_owned * NQ) -- each (m, p) plane a case lists
an independent field with values in +-U(0.5, 1.5) from a generator of its own (seed + 13), all others zero -- and the coefficients'
values `c0` (nc,), +-U(0.3, 0.9); `full` = [theta | c0].

Conditions on the reference alone (`conditions`), asserted before a device number is looked at: nonlinear_reference's (a) - (c) on
THIS reference (the network blocks of the gradient, the base planes, the indexing) and
  (e) exchanging any two directions moves the vector d lossv / d c by more than flux_reference.COLUMN_MOVE of its norm: a kernel that
      reads direction m' for coefficient m, or lands a sum in the wrong slot, cannot pass;
  (f) zeroing any one non-zero (m, p) plane moves lossv by more than that share: a kernel that skips a plane or adds it to the wrong
      coefficient plane cannot pass.
Seeds: the first from the case's starting one that keeps all of them (searched here, on the CPU).
"""
import itertools

import numpy as np
import torch

import data_term_reference as dr
import flux_reference as fr
import generic_point as gp
import linear_reference as lr
import nonlinear_reference as nr


def n_planes(dim):
    return (3, 4) if dim == 1 else (5, 5)


def problem(c):
    """nonlinear_reference.problem(c) plus dirs (nc, K + M, n_owned * NQ), c0 (nc,), full = [theta | c0]; c['dirs'] lists, per
    coefficient, the planes its direction touches"""
    p = nr.problem(c)
    K, M = n_planes(p["dim"])
    rng = np.random.default_rng(c["seed"] + 13)
    nq = p["planes"].shape[1]
    dirs = np.zeros((len(c["dirs"]), K + M, nq))
    for m, rows in enumerate(c["dirs"]):
        for r in rows:
            dirs[m, r] = lr._signed(rng, nq)
    p["dirs"] = dirs
    p["c0"] = rng.uniform(0.3, 0.9, dirs.shape[0]) * rng.choice([-1.0, 1.0], dirs.shape[0])
    p["full"] = np.concatenate([p["theta"], p["c0"]])
    return p


def split(p, full):
    full = np.asarray(full, dtype=np.float64)
    n = p["theta"].size
    return full[:n], full[n:]


def effective(p, c, dirs=None):
    """(planes, nl) as numpy with c_m D_m baked in (the baked-in equivalence test hands them to a handle without coefficients)"""
    K, _ = n_planes(p["dim"])
    eff = np.concatenate([p["planes"], p["nl"]], 0) + np.einsum("m,mpq->pq", np.asarray(c, dtype=np.float64), p["dirs"] if dirs is None else dirs)
    return eff[:K], eff[K:]


def _loss(p, ch, pl):
    """nonlinear_reference._loss_from_channels on torch planes pl (K + M, n_owned * NQ) -> (R masked, loss_e, lossv, mask)"""
    dim, eb, ee = p["dim"], p["eb"], p["ee"]
    b = p["boxes"][eb:ee]
    ne = ee - eb
    qx, ntx, nty = p["xr"][0].size, p["ntx"], p["nty"]
    qy = p["yr"][0].size if dim == 2 else 1
    tx, ty = nr._tables(p)
    K, _ = n_planes(dim)

    def el(v):
        return v.reshape(ne, qy, qx)
    P = [el(r) for r in pl]
    a2, a3, ae = P[K:K + 3]
    g = P[K + 3:]
    u, ux = el(ch[0]), el(ch[1])
    Jx = torch.tensor((b[:, 1] - b[:, 0]) / 2)
    N = a2 * u ** 2 + a3 * u ** 3 + ae * torch.exp(u) + u * g[0] * ux
    if dim == 2:
        uy = el(ch[2])
        N = N + u * g[1] * uy
        kx, ky, bx, by, s = P[:K]
        Jy = torch.tensor((b[:, 3] - b[:, 2]) / 2)
        J = Jx * Jy
        G = [bx * ux + by * uy + s * u + N, kx * ux, ky * uy]
    else:
        k, bb, s = P[:K]
        J = Jx
        G = [bb * ux + s * u + N, k * ux]

    def proj(Gt, dx, dy):
        return torch.einsum("kj,ri,eji->ekr", ty[dy], tx[dx], Gt)
    if dim == 2:
        U = (-(J / Jx))[:, None, None] * proj(G[1], 1, 0) - (J / Jy)[:, None, None] * proj(G[2], 0, 1) + J[:, None, None] * proj(G[0], 0, 0)
    else:
        U = (-(J / Jx))[:, None, None] * proj(G[1], 1, 0) + J[:, None, None] * proj(G[0], 0, 0)
    R = U - torch.tensor(np.ascontiguousarray(p["F"][eb:ee]))
    nax = np.full(ne, ntx) if p["nax"] is None else p["nax"][eb:ee]
    nay = np.full(ne, nty) if p["nay"] is None else p["nay"][eb:ee]
    mask = (np.arange(ntx)[None, None, :] < nax[:, None, None]) & (np.arange(nty)[None, :, None] < nay[:, None, None])
    R = R * torch.tensor(mask.astype(np.float64))
    loss_e = torch.sum(R * R, dim=(1, 2)) / torch.tensor((nax * nay).astype(np.float64))
    return R, loss_e, torch.sum(loss_e), mask


def var_part(p, full=None, dirs=None, planes=None, nl=None, grad=True):
    """dict(R, lossv, grad = [d theta | d c]) of the variational term at full = [theta | c]"""
    theta, c = split(p, p["full"] if full is None else full)
    o, ch = nr._channels(p, theta)
    ct = torch.tensor(c, requires_grad=True)
    base = torch.tensor(np.concatenate([p["planes"] if planes is None else planes, p["nl"] if nl is None else nl], 0))
    D = torch.tensor(p["dirs"] if dirs is None else dirs)
    pl = base + torch.einsum("m,mpq->pq", ct, D)
    R, _, lossv, mask = _loss(p, ch, pl)
    Rn = R.detach().numpy().copy()
    Rn[~mask] = 0.0
    out = dict(R=Rn, lossv=float(lossv.detach()))
    if grad:
        gt, gc = torch.autograd.grad(lossv, [o.theta, ct])
        out["grad"] = np.concatenate([gt.numpy(), gc.numpy()])
    return out


def reference(p, full=None, dirs=None):
    """(loss triple, gradient [d theta | d c], R) of var + data + flux at `full`"""
    full = p["full"] if full is None else np.asarray(full, dtype=np.float64)
    theta, c = split(p, full)
    v = var_part(p, full, dirs)
    d = dict(wmsq=0.0, msq=0.0, grad=0.0) if p["data"] is None else dr.data_part(p["prob"], p["layers"], theta, p["data"][0], p["data"][1], p["lbw"])
    f = fr.flux_part(p["prob"], p["layers"], theta, p["flux"])
    g = v["grad"].copy()
    g[:theta.size] += d["grad"] + f["grad"]
    return fr.triple(p["prob"], v["lossv"], d, f), g, v["R"]


def conditions(p):
    """(a) - (c), (e), (f) of the module docstring; returns the figures for the log"""
    K, _ = n_planes(p["dim"])
    v = var_part(p)
    _, g, _ = reference(p)
    nth = p["theta"].size
    total = np.linalg.norm(g[:nth])
    share = {k: float(np.linalg.norm(g[lo:hi]) / total) for k, lo, hi in gp.blocks(p["layers"], 0)}
    assert min(share.values()) >= gp.BLOCK_FLOOR, ("(a)", share)

    def move(**kw):
        return abs(var_part(p, grad=False, **kw)["lossv"] - v["lossv"]) / v["lossv"]
    base = []
    for i in range(K):
        z = p["planes"].copy()
        z[i] = 0.0
        base.append(move(planes=z))
    assert min(base) > fr.COLUMN_MOVE, ("(b)", base)
    gc = v["grad"][nth:]
    ex = {}
    for i, j in itertools.combinations(range(gc.size), 2):
        d = p["dirs"].copy()
        d[[i, j]] = d[[j, i]]
        ex[(i, j)] = float(np.linalg.norm(var_part(p, dirs=d)["grad"][nth:] - gc) / np.linalg.norm(gc))
    assert not ex or min(ex.values()) > fr.COLUMN_MOVE, ("(e)", ex)
    zp = {}
    for m, r in zip(*np.nonzero(np.any(p["dirs"] != 0.0, axis=2))):
        d = p["dirs"].copy()
        d[m, r] = 0.0
        zp[(int(m), int(r))] = move(dirs=d)
    assert zp and min(zp.values()) > fr.COLUMN_MOVE, ("(f)", zp)
    return dict(block_share=min(share.values()), base=min(base), exchange=min(ex.values()) if ex else None, plane=min(zp.values()))


def adam_trajectory(p, steps, lr_=1e-3, full=None, b1=0.9, b2=0.999, eps=1e-8):
    """`steps` TF1-Adam updates (the rule and constants of oracle.vpinn_oracle.adam_step) over network AND coefficients; returns
    (full after the last update, m, v)"""
    th = np.array(p["full"] if full is None else full, dtype=np.float64)
    m, v = np.zeros_like(th), np.zeros_like(th)
    b1p, b2p = b1, b2
    for _ in range(steps):
        g = reference(p, th)[1]
        lr_t = lr_ * np.sqrt(1.0 - b2p) / (1.0 - b1p)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        th = th - lr_t * m / (np.sqrt(v) + eps)
        b1p, b2p = b1p * b1, b2p * b2
    return th, m, v


# ---- the case table: linear_reference.CASES' small shapes with coefficients on them ---------------------------------------------------
# 2-D planes: kx 0, ky 1, bx 2, by 3, s 4 | a2 5, a3 6, ae 7, gx 8, gy 9;   1-D: k 0, b 1, s 2 | a2 3, a3 4, ae 5, g 6
_c, S8, W24, B2, B1 = lr._c, lr.S8, lr.W24, lr.BOXES2, lr.BOXES1

CASES = {
    # two coefficients; the first is an anisotropic conductivity, the second touches the operator and a nonlinear plane
    "2d-h8": _c("2d-h8", S8, B2[:3], (6, 5), (4, 3), 9501, dirs=[[0, 1], [4, 6]]),
    # n_coef = 1, every plane at once, on a shard with data: the element offset into the directions
    "2d-h8-shard-data-nc1": _c("2d-h8-shard-data-nc1", S8, B2, (6, 5), (4, 3), 9512, shard=(1, 4), data=19, dirs=[list(range(10))]),      # (9511 misses (f) on ky)
    # two coefficients SHARING a plane (kx), one direction with all but one plane zero; per-element counts, data + flux
    "2d-h8-counts-flux-shared": _c("2d-h8-counts-flux-shared", S8, B2[:3], (6, 5), (4, 3), 9521, data=19, flux=17,
                                   counts=([4, 2, 3], [1, 3, 2]), dirs=[[0], [0, 3]]),
    # n_coef = 8 around the wide layer kernels, shard + counts + flux
    "2d-h24-nc8": _c("2d-h24-nc8", W24, B2, (6, 5), (4, 3), 9531, shard=(1, 4), data=19, flux=17, counts=([3, 4, 2, 3], [2, 1, 3, 3]),
                     dirs=[[0], [1], [2, 3], [4], [5], [6], [7], [8, 9]]),
    "1d-sin": _c("1d-sin", [1, 8, 8, 1], B1, 7, 4, 9541, data=2, counts=([4, 2, 3], None), dirs=[[0], [2, 5]]),
    # directions on nonlinear planes over a ZERO base: the handle never hears of hpv_set_nonlinear, the terms are active all the same
    "2d-nl-over-zero-base": _c("2d-nl-over-zero-base", S8, B2[:3], (6, 5), (4, 3), 9551, terms=(), dirs=[[5], [7], [8, 9]]),
    "1d-nl-over-zero-base": _c("1d-nl-over-zero-base", [1, 8, 8, 1], B1, 7, 4, 9561, data=2, terms=(), dirs=[[4], [6]]),
    # one element of 17 x 17 points: NQ = 289 > 256, some threads own two points
    "2d-17x17": _c("2d-17x17", S8, B2[3:], (17, 17), (4, 3), 9571, data=19, dirs=[[0, 1], [7]]),
    # the padding invariant: a 20-point rule padded to 21 x 21 with zero-weight points, 10 x 10 functions
    "lds-21x21-padded": _c("lds-21x21-padded", S8, B2[3:], (21, 21), (10, 10), 9581, data=19, pad=(1, 1), dirs=[[0, 1], [6]]),
}
SMALL = [k for k in CASES if not k.startswith("lds")]


def from_model(m, full=None):
    """The problem dict of a live VPINNLinear / VPINNNonlinear with trainable coefficients (one rank): nonlinear_reference.from_model's
    (linear_reference.from_model's with a zero nonlinear term) plus its directions evaluated here at the quadrature points"""
    full = m.get_params() if full is None else np.asarray(full, dtype=np.float64)
    nc = len(m._trainable)
    theta = full[:full.size - nc]
    if hasattr(m, "_nl"):
        p = nr.from_model(m, theta)
    else:
        p = lr.from_model(m, theta)
        p["nl"], p["terms"] = np.zeros((n_planes(p["dim"])[1], p["planes"].shape[1])), ()
    mesh, dim = m._mesh, m.layers[0]
    P = lr.quad_points(mesh.boxes, p["xr"][0], None if p["yr"] is None else p["yr"][0])
    p["dirs"] = np.stack([m._direction(t, P, dim) for t in m._trainable], 0)
    p["c0"], p["full"] = full[full.size - nc:].copy(), full.copy()
    return p


def host_model(s, LR=1e-3, seed=1234):
    """The model drivers/identify.run(s) would create, WITHOUT a device: the class's own constructor (mesh, rule, fields, trainable
    list, initial parameters) with everything that touches the library left out.  from_model(host_model(s)) is the CPU reference's
    problem for the driver's setting."""
    from hp_vpinns_amd.init import xavier_init
    from hp_vpinns_amd.vpinn import VPINNLinear, VPINNNonlinear

    class Host(VPINNNonlinear if s["nonlinear"] else VPINNLinear):
        def _create(self, layers, var_form, LR, lossb_weight, V, init_params, seed, backend, device):
            self.layers = [int(v) for v in layers]
            self.rank, self.world = 0, 1
            self._params = xavier_init(self.layers, seed, extra=[t["init"] for t in self._trainable])

        def _populate_mesh(self, mesh, f):
            pass

        def _hand_data(self):
            pass

        def _finish(self):
            pass

        def get_params(self):
            return self._params.copy()

        def __del__(self):
            pass
    return Host(s["layers"], LR=LR, seed=seed, **s["model"])
