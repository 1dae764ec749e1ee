"""The dual-norm residual loss through DENSE Gram matrices (hpv_set_residual_gram, csrc/hpv_dual_dense.h, quadrature.gram_factors,
VPINNLinear(residual_norm=dict(kind="dual", metric="physical" | "energy"))) in fp64 on the CPU, and the case tables of
tests/test_gpu_dualdense.py (a plain helper module like dualnorm_reference.py; no GPU needed).  tests/test_dualdense_host.py proves it.

    loss_e = R_e^T G_e^{-1} R_e        G_e[(k,r),(k',r')] = int_e  grad v_kr . S grad v_k'r'  +  mass v_kr v_k'r'   dx

on the element's ACTIVE test functions v_kr = phi_r(xi) phi_k(eta), S the identity (the physical H^1 product) or a symmetric positive
definite field (the energy product of div(K grad u), S = sym(K)); the element any smooth image of the reference square.

  reference   G_e assembled here with plain loops over hp_vpinns_amd.testfcn's functions, in PHYSICAL terms (grad_x v = A^-T grad_ref v,
              dx = det A dxi deta) on a Gauss-Legendre rule of GRAM_MARGIN + max(ntx, nty) points -- nothing of quadrature.gram_factors,
              no Cholesky factor; loss_e by a dense torch solve.  Everything up to R is dualnorm_reference.reference (boxes, 1-D and
              2-D: ansatz_reference / ident_reference) or mapped_reference.terms (quadrilaterals) unchanged: both form their Gram
              matrix through dualnorm_reference.gram_element, which `_dense` replaces for the duration of a call.
  product     quadrature.gram_factors: W_e applied to R in numpy (`factor_route`).
"""
import contextlib

import numpy as np
import torch

import dualnorm_reference as dn
import linear_reference as lr
import linop_sweep as ls
import mapped_reference as mr

GRAM_MARGIN = 3                  # dualnorm_reference.gram_quadrature's: n + 3 points
ESTIMATOR_TOL = 1e-13            # one decade above the measured 1.5e-15 (sheared quadrilateral, physical) / 4.0e-15 (box, 2 x 2 SPD K(x), energy), rounded up to a power of ten


def rule(ntx, nty):
    return np.polynomial.legendre.leggauss(max(ntx, nty) + GRAM_MARGIN)


# ---- the weight tensors of the tests: symmetric positive definite fields of the physical point ---------------------------------------
def S_energy(P):
    """(n, 2, 2) at points (n, 2): eigenvalues inside [0.5, 2.3]"""
    x, y = P[:, 0], P[:, 1]
    o = 0.3 * np.cos(x - y)
    return np.stack([np.stack([1.5 + 0.5 * np.sin(2.0 * x + y), o], 1), np.stack([o, 1.2 + 0.4 * np.cos(y)], 1)], 1)


def S_energy_1d(P):
    return 1.5 + 0.5 * np.sin(3.0 * P[:, 0])


# ---- G_e by loops -------------------------------------------------------------------------------------------------------------------
def gram_dense(nax, nay, X, A, S, mass, x, w):
    """G_e on the active block, index k * nax + r.  X (ng * ng, 2), A (ng * ng, 2, 2) at the rule's points (g = j * ng + i); S a callable
    of the physical points or None (identity)"""
    from hp_vpinns_amd.testfcn import Test_fcn, dTest_fcn
    ng = x.size
    px, dpx, py, dpy = Test_fcn(nax, x), dTest_fcn(nax, x)[0], Test_fcn(nay, x), dTest_fcn(nay, x)[0]
    Sg = np.tile(np.eye(2), (ng * ng, 1, 1)) if S is None else S(X)
    n = nax * nay
    G = np.zeros((n, n))
    for j in range(ng):
        for i in range(ng):
            g = j * ng + i
            a = A[g]
            det = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
            ait = np.linalg.inv(a).T
            val = np.array([px[r, i] * py[k, j] for k in range(nay) for r in range(nax)])
            gref = np.array([[dpx[r, i] * py[k, j], px[r, i] * dpy[k, j]] for k in range(nay) for r in range(nax)])      # (n, 2)
            gx = gref @ ait.T                                                                                            # grad_x v = A^-T grad_ref v
            s = 0.5 * (Sg[g] + Sg[g].T)
            G += w[j] * w[i] * det * (gx @ s @ gx.T + mass * np.outer(val, val))
    return G


def gram_dense_1d(nax, X, Jx, S, mass, x, w):
    from hp_vpinns_amd.testfcn import Test_fcn, dTest_fcn
    px, dpx = Test_fcn(nax, x), dTest_fcn(nax, x)[0]
    s = np.ones(x.size) if S is None else S(X)
    G = np.zeros((nax, nax))
    for i in range(x.size):
        G += w[i] * Jx * (s[i] * np.outer(dpx[:, i], dpx[:, i]) / Jx ** 2 + mass * np.outer(px[:, i], px[:, i]))
    return G


def _counts(p):
    ne = p["ee"] - p["eb"]
    nax = np.full(ne, p["ntx"]) if p["nax"] is None else np.asarray(p["nax"])[p["eb"]:p["ee"]]
    nay = np.full(ne, p["nty"]) if p["nay"] is None else np.asarray(p["nay"])[p["eb"]:p["ee"]]
    return [int(v) for v in nax], [int(v) for v in nay]


def grams(p, S, geom=None):
    """[G_e] of the owned elements of problem dict p (dualnorm_reference's on boxes, mapped_reference's with geom = a function
    (xi, yi) -> (X, A) of ALL elements)"""
    nax, nay = _counts(p)
    x, w = rule(p["ntx"], p["nty"])
    eb, ee = p["eb"], p["ee"]
    if p["dim"] == 1:
        b = np.asarray(p["boxes"], dtype=np.float64)[eb:ee]
        return [gram_dense_1d(nax[e], (b[e, 0] + (b[e, 1] - b[e, 0]) / 2 * (x + 1))[:, None], (b[e, 1] - b[e, 0]) / 2, S, p["mass"], x, w)
                for e in range(ee - eb)]
    X, A = mr.geom_boxes(p["boxes"], x, x) if geom is None else geom(x, x)
    return [gram_dense(nax[e], nay[e], X[eb + e], A[eb + e], S, p["mass"], x, w) for e in range(ee - eb)]


@contextlib.contextmanager
def _dense(Gs, p):
    """dualnorm_reference.gram_element answers with the dense G_e of the owned elements, in their order (both references ask once per
    owned element and loss evaluation, in element order)"""
    orig, n = dn.gram_element, [0]
    nax, nay = _counts(p)

    def gram_element(dim, na, nb, Jx, Jy, mass):
        e = n[0] % len(Gs)
        n[0] += 1
        assert (na, nb if dim == 2 else 1) == (nax[e], nay[e] if dim == 2 else 1) and Gs[e].shape[0] == na * (nb if dim == 2 else 1)
        return Gs[e]
    dn.gram_element = gram_element
    try:
        yield
    finally:
        dn.gram_element = orig


def loss_e(Gs, p, R):
    """(loss_e, Rbar = d loss_e / d R) of numpy residuals R (n_owned, nty, ntx) by the dense solve"""
    nax, nay = _counts(p)
    le, Rb = [], np.zeros_like(R)
    for e, G in enumerate(Gs):
        r = R[e][:nay[e], :nax[e]].reshape(-1)
        v = np.linalg.solve(G, r)
        le.append(float(r @ v))
        Rb[e][:nay[e], :nax[e]] = 2.0 * v.reshape(nay[e], nax[e])
    return np.array(le), Rb


def factor_route(W, R):
    """the same through the product's factors W (n_owned, NR, NR): loss_e = |W_e R_e|^2, Rbar = 2 W_e^T W_e R_e"""
    y = np.einsum("eij,ej->ei", W, R.reshape(R.shape[0], -1))
    return np.sum(y * y, axis=1), 2.0 * np.einsum("eij,ei->ej", W, y).reshape(R.shape)


# ---- boxes: the machinery of dualnorm_reference / linop_sweep ----------------------------------------------------------------------
B2 = np.asarray(lr.BOXES2[:3])
ROWS = {
    "1d-33": dict(L=ls.L1, boxes=lr.BOXES1[:2], q=36, nt=33, data=1, flux=0),                       # NR odd, fewer columns than lanes; the rows end on wave 0
    "2d-70": dict(L=lr.S8, boxes=B2[:2], q=(12, 9), nt=(10, 7), data=1, flux=0),                    # more rows than lanes; NR no multiple of 4
    "2d-1x1": dict(L=lr.S8, boxes=B2[:2], q=(3, 3), nt=(1, 1), data=0, flux=0),                     # one row
    "counts": dict(L=lr.S8, boxes=B2, q=(6, 5), nt=(4, 3), data=1, flux=3, counts=([4, 1, 3], [3, 2, 1])),      # inactive rows inside the triangle
    "shard": dict(L=lr.S8, boxes=B2, q=(6, 5), nt=(4, 3), data=1, flux=0, counts=([4, 1, 3], [3, 2, 1]), shard=(1, 3)),      # the offset into W
    "append": dict(L=lr.S8, boxes=B2[:2], q=(3, 2), nt=(5, 4), data=1, flux=0),                     # NR = 20 > 3 * 2 * 3: y is appended behind red
    "aspect": dict(L=lr.S8, boxes=dn.BOXES_ASPECT, q=(6, 5), nt=(4, 3), data=0, flux=0, counts=([4, 1, 3, 4], [3, 3, 1, 2])),      # Jx / Jy = 24
}
# (name, row, variant, ansatz, mass, metric)
TABLE = [
    ("1d-33-lin", "1d-33", "lin", None, 0.0, "energy"), ("2d-70-lin", "2d-70", "lin", None, 3.0, "energy"),
    ("2d-1x1-lin", "2d-1x1", "lin", None, 0.0, "physical"), ("counts-lin", "counts", "lin", None, 0.0, "energy"),
    ("counts-nl", "counts", "nl", None, 3.0, "energy"), ("counts-id", "counts", "id", None, 0.0, "energy"),
    ("counts-lin-ansatz", "counts", "lin", "generic", 3.0, "energy"), ("shard-lin", "shard", "lin", None, 0.0, "energy"),
    ("append-lin", "append", "lin", None, 3.0, "energy"), ("aspect-lin", "aspect", "lin", None, 3.0, "physical"),
]


def cases():
    out = []
    for i, (name, row, variant, ansatz, mass, metric) in enumerate(TABLE):
        c = ls._case(name, ROWS[row], variant, ansatz, 14001 + 50 * i)
        c["row"], c["mass"], c["metric"] = row, mass, metric
        out.append(c)
    return out


def problem(c):
    p = ls.problem(c)
    p["mass"] = float(c["mass"])
    p["metric"] = c["metric"]
    return p


def S_of(p):
    return None if p["metric"] == "physical" else S_energy_1d if p["dim"] == 1 else S_energy


def box_factors(p):
    """quadrature.gram_factors of the owned boxes of p: what a caller of hpv_set_residual_gram hands over"""
    from hp_vpinns_amd.quadrature import gram_factors, gram_rule
    eb, ee = p["eb"], p["ee"]
    b = np.asarray(p["boxes"], dtype=np.float64)[eb:ee]
    x = gram_rule(p["ntx"], p["nty"])[0]
    ng, ne = x.size, ee - eb
    nax, nay = _counts(p)
    S = S_of(p)
    if p["dim"] == 1:
        J = (b[:, 1] - b[:, 0]) / 2
        P = (b[:, 0:1] + J[:, None] * (x[None, :] + 1)).reshape(-1, 1)
        return gram_factors(1, p["ntx"], 1, nax, 1, np.repeat(J[:, None], ng, 1), None if S is None else S(P).reshape(ne, ng), p["mass"], first=eb)
    X, A = mr.geom_boxes(b, x, x)
    return gram_factors(2, p["ntx"], p["nty"], nax, nay, A, None if S is None else S(X.reshape(-1, 2)).reshape(ne, ng * ng, 2, 2), p["mass"], first=eb)


def reference(p, full=None):
    """(loss triple, gradient, R) of a box problem under the dense dual norm"""
    with _dense(grams(p, S_of(p)), p):
        return dn.reference(p, full)


def reference_autograd(p, full=None):
    with _dense(grams(p, S_of(p)), p):
        return dn.reference_autograd(p, full)


def adam_trajectory(p, steps):
    with _dense(grams(p, S_of(p)), p):
        return dn.adam_trajectory(p, steps)


# ---- quadrilaterals: mapped_reference ------------------------------------------------------------------------------------------------
def quad_geom(corners):
    return lambda xi, yi: mr.geom_quads(corners, xi, yi)


def mapped_terms(p, corners, S=None, full=None):
    """mapped_reference.terms of problem dict p (mass set, boxes a placeholder) under the dense Gram matrices of the quadrilaterals"""
    q = dict(p, boxes=np.zeros((p["X"].shape[0], 4)))
    with _dense(grams(q, S, quad_geom(corners)), q):
        return mr.terms(q, full)


def mapped_adam(p, corners, steps):
    q = dict(p, boxes=np.zeros((p["X"].shape[0], 4)))
    with _dense(grams(q, None, quad_geom(corners)), q):
        return mr.adam_trajectory(q, steps)


def rotated_rectangle(box, angle):
    """corners (4, 2) of the box (x0, x1, y0, y1) rotated by `angle` about the origin, counter-clockwise from the image of (-1, -1)"""
    x0, x1, y0, y1 = box
    c = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
    rot = np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]])
    return c @ rot.T
