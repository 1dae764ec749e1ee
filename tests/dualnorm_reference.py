"""The dual-norm (Riesz) residual loss of the variable-coefficient classes (hpv_set_residual_norm, csrc/hpv_dual_norm.h,
VPINNLinear / VPINNNonlinear(residual_norm="dual")) in fp64 on the CPU, and the case table of tests/test_gpu_dualnorm.py (a plain
helper module like linop_sweep.py; no GPU needed).  tests/test_dualnorm_host.py proves it.

    loss_e = R_e^T G_e^{-1} R_e        G_e = (Jy/Jx) M_y (x) K_x + (Jx/Jy) K_y (x) M_x + mass Jx Jy M_y (x) M_x      (1-D: K_x / Jx + mass Jx M_x)

on the element's ACTIVE test functions, K = int phi' phi', M = int phi phi on the reference interval.

  reference   the loss, R and the gradient by a DENSE solve of the Kronecker-assembled G_e, whose K and M are assembled here by
              Gauss-Legendre quadrature of hp_vpinns_amd.testfcn's functions (`gram_quadrature`: no closed form, no eigen-solve).
              Everything up to R -- channels, planes, nonlinear terms, directions, ansatz, data and flux terms -- is
              ansatz_reference.reference / ident_reference._loss (the superset of linear_reference.var_part) unchanged: only the
              step R -> loss_e is replaced (`_dual`), so torch differentiates through the solve.
  table route the library's: quadrature.gram_stacks (closed forms, symmetric eigen-solve), G_e^{-1} = (S_y (x) S_x) diag(1/d)
              (S_y (x) S_x)^T applied to R in numpy (`table_route`), compared with the dense solve on R of every case.

Conditions on the reference alone (`conditions`), before a device number is looked at: linop_sweep.conditions of the case (the l2
problem's (a) - (c) and the two derivations within AGREE); max d / min d < COND_D on every element (no case loses more than half its
digits in d); table route against dense solve, loss_e and Rbar, within linop_sweep.AGREE; the two derivations of the DUAL loss and
gradient (ansatz_reference.reference and .reference_autograd under `_dual`) within AGREE; the network gradient against central
differences of the reference loss along N_FD random directions within FD_TOL.
"""
import contextlib

import numpy as np
import torch

import ansatz_reference as ar
import generic_point as gp
import ident_reference as ir
import linear_reference as lr
import linop_sweep as ls

COND_D = 1e8
N_FD = 3
FD_H = float(np.finfo(np.float64).eps ** (1.0 / 3.0))          # the step that balances truncation h^2 against rounding eps / h
FD_TOL = 1e4 * float(np.finfo(np.float64).eps ** (2.0 / 3.0))  # ~3.7e-7: that balance with four decades for the derivatives' constants (as vpinn._check_ansatz_field)


# ---- Gram matrices, assembled independently ---------------------------------------------------------------------------------------------
def gram_quadrature(n):
    """(K, M) of the first n test functions by Gauss-Legendre quadrature (n + 3 points: exact to degree 2 n + 5 >= 2 n + 2)"""
    from hp_vpinns_amd.testfcn import Test_fcn, dTest_fcn
    x, w = np.polynomial.legendre.leggauss(n + 3)
    phi, dphi = Test_fcn(n, x), dTest_fcn(n, x)[0]
    return (dphi * w[None, :]) @ dphi.T, (phi * w[None, :]) @ phi.T


def gram_element(dim, nax, nay, Jx, Jy, mass):
    """G_e on the active block, index k * nax + r (the order of R[k][r])"""
    Kx, Mx = gram_quadrature(nax)
    if dim == 1:
        return Kx / Jx + mass * Jx * Mx
    Ky, My = gram_quadrature(nay)
    return (Jy / Jx) * np.kron(My, Kx) + (Jx / Jy) * np.kron(Ky, Mx) + mass * Jx * Jy * np.kron(My, Mx)


def _elements(p):
    """[(nax, nay, Jx, Jy)] of the owned elements"""
    eb, ee = p["eb"], p["ee"]
    b = p["boxes"][eb:ee]
    ne = ee - eb
    nax = np.full(ne, p["ntx"]) if p["nax"] is None else p["nax"][eb:ee]
    nay = np.full(ne, p["nty"]) if p["nay"] is None else p["nay"][eb:ee]
    Jx = (b[:, 1] - b[:, 0]) / 2
    Jy = (b[:, 3] - b[:, 2]) / 2 if p["dim"] == 2 else np.ones(ne)
    return [(int(nax[e]), int(nay[e]), float(Jx[e]), float(Jy[e])) for e in range(ne)]


def _loss_dual(orig, p, ch, pl, mass):
    """ident_reference._loss with loss_e = R_e^T G_e^{-1} R_e by a dense solve"""
    R, _, _, mask = orig(p, ch, pl)
    le = []
    for e, (nax, nay, Jx, Jy) in enumerate(_elements(p)):
        r = R[e][:nay, :nax].reshape(-1)
        G = torch.tensor(gram_element(p["dim"], nax, nay, Jx, Jy, mass))
        le.append(torch.dot(r, torch.linalg.solve(G, r)))
    loss_e = torch.stack(le)
    return R, loss_e, torch.sum(loss_e), mask


@contextlib.contextmanager
def _dual(mass):
    """ident_reference._loss replaced by _loss_dual for the references that call it (ansatz_reference.reference, .reference_autograd)"""
    orig = ir._loss
    ir._loss = lambda p, ch, pl: _loss_dual(orig, p, ch, pl, mass)
    try:
        yield
    finally:
        ir._loss = orig


def reference(p, full=None):
    """(loss triple, gradient [d theta | d c], R) under the dual norm with p['mass']"""
    with _dual(p["mass"]):
        return ar.reference(p, full)


def reference_autograd(p, full=None):
    with _dual(p["mass"]):
        return ar.reference_autograd(p if p["kind"] is not None else dict(p, kind="identity"), full)


def adam_trajectory(p, steps):
    with _dual(p["mass"]):
        return ar.adam_trajectory(p, steps)


def dense_route(p, R):
    """(loss_e (n_owned,), Rbar (n_owned, nty, ntx) = d loss_e / d R) of the numpy residuals R by the dense solve"""
    le, Rb = [], np.zeros_like(R)
    for e, (nax, nay, Jx, Jy) in enumerate(_elements(p)):
        r = R[e][:nay, :nax].reshape(-1)
        w = np.linalg.solve(gram_element(p["dim"], nax, nay, Jx, Jy, p["mass"]), r)
        le.append(float(r @ w))
        Rb[e][:nay, :nax] = 2.0 * w.reshape(nay, nax)
    return np.array(le), Rb


def d_table(p, e_info, stacks=None):
    """d[a][b] of one element (nax, nay, Jx, Jy) from quadrature.gram_stacks"""
    from hp_vpinns_amd.quadrature import gram_stacks
    nax, nay, Jx, Jy = e_info
    lx = (stacks[0] if stacks else gram_stacks(p["ntx"]))[1][nax - 1, :nax]
    if p["dim"] == 1:
        return (lx / Jx + p["mass"] * Jx)[None, :]
    ly = (stacks[1] if stacks else gram_stacks(p["nty"]))[1][nay - 1, :nay]
    return (Jy / Jx) * lx[None, :] + (Jx / Jy) * ly[:, None] + p["mass"] * Jx * Jy


def table_route(p, R):
    """the same by the library's route: the eigen tables of quadrature.gram_stacks, four small products per element"""
    from hp_vpinns_amd.quadrature import gram_stacks
    st = (gram_stacks(p["ntx"]), gram_stacks(p["nty"]) if p["dim"] == 2 else None)
    le, Rb = [], np.zeros_like(R)
    for e, info in enumerate(_elements(p)):
        nax, nay, Jx, Jy = info
        Sx = st[0][0][nax - 1, :nax, :nax]
        Sy = st[1][0][nay - 1, :nay, :nay] if p["dim"] == 2 else np.ones((1, 1))
        Rh = Sy.T @ (R[e][:nay, :nax] @ Sx)
        w = Rh / d_table(p, info, st)
        le.append(float(np.sum(Rh * w)))
        Rb[e][:nay, :nax] = Sy @ (2.0 * w) @ Sx.T
    return np.array(le), Rb


def lds_bytes(qx, qy, ntx, nty):
    """hpv_dual_lds_bytes (csrc/kernels_linop.hip, hpv_dual_norm.h), restated: the layout of linop_sweep.lds_bytes, with the scratch
    Sx [ntx][ntx|1]  Sy [nty][nty|1]  lam_x [ntx]  lam_y [nty]  A [nty][ntx|1]  appended where G [3][qy][qx|1] cannot hold it.
    Returns (bytes, aliased)"""
    scratch = ntx * (ntx | 1) + nty * (nty | 1) + ntx + nty + nty * (ntx | 1)
    aliased = scratch <= 3 * qy * (qx | 1)
    return ls.lds_bytes(qx, qy, ntx, nty) + (0 if aliased else 8 * scratch), aliased


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
# the counts row on boxes of unequal aspect ratio: the second has Jx / Jy = 24
BOXES_ASPECT = [[-1.0, -0.2, -1.0, 0.1], [-0.2, 1.0, -1.0, -0.95], [-1.0, -0.4, 0.1, 1.0], [-0.4, 0.3, 0.1, 0.55]]
ROWS = dict(ls.ROWS)
ROWS["counts"] = dict(ls.ROWS["counts"], boxes=BOXES_ASPECT)
# two rows beyond the issue's: shapes whose scratch does not fit the G region and is appended behind `red` (many functions on few points)
ROWS["1d-append"] = dict(L=ls.L1, boxes=lr.BOXES1, q=12, nt=10, data=1, flux=0)
ROWS["2d-append"] = dict(L=lr.S8, boxes=lr.BOXES2[:2], q=(12, 3), nt=(10, 1), data=0, flux=3)
REFUSED_1D = (62, 1, 60, 1)      # hpv_set_tables admits it (63 984 B); with the scratch appended it is past 64 KiB: the setter refuses
ESTIMATOR_TOL = 1e-13            # one decade above the measured 4.6e-15 (2-D) / 2.6e-15 (1-D), rounded up to a power of ten
# (name, row, variant, ansatz, mass): every row as lin; nr272 and counts also as nl and id; counts under the generic ansatz; both masses on >= 2 rows
TABLE = [
    ("min-lin", "min", "lin", None, 0.0), ("nty1-lin", "nty1", "lin", None, 3.0),
    ("nr272-lin", "nr272", "lin", None, 0.0), ("nr272-nl", "nr272", "nl", None, 3.0), ("nr272-id", "nr272", "id", None, 0.0),
    ("tall-lin", "tall", "lin", None, 3.0), ("wide-lin", "wide", "lin", None, 0.0),
    ("counts-lin", "counts", "lin", None, 0.0), ("counts-nl", "counts", "nl", None, 3.0), ("counts-id", "counts", "id", None, 3.0),
    ("counts-lin-ansatz", "counts", "lin", "generic", 0.0),
    ("padx-lin", "padx", "lin", None, 3.0), ("ldsmax-lin", "ldsmax", "lin", None, 0.0),
    ("1d-min-lin", "1d-min", "lin", None, 3.0), ("1d-272-lin", "1d-272", "lin", None, 0.0),
    ("1d-append-lin", "1d-append", "lin", None, 3.0), ("2d-append-lin", "2d-append", "lin", None, 0.0),
]
# the first seed from each case's base (9901 + 50 * position, the rule of linop_sweep.fixed_cases) that keeps `conditions`
SEEDS = {
    "min-lin": 12001, "nty1-lin": 12051, "nr272-lin": 12103, "nr272-nl": 12152, "nr272-id": 12204, "tall-lin": 12251, "wide-lin": 12302,
    "counts-lin": 12351, "counts-nl": 12402, "counts-id": 12451, "counts-lin-ansatz": 12501, "padx-lin": 12551, "ldsmax-lin": 12601,
    "1d-min-lin": 12651, "1d-272-lin": 12701, "1d-append-lin": 12751, "2d-append-lin": 12802,
}


def cases(seeds=None):
    seeds = SEEDS if seeds is None else seeds
    out = []
    for i, (name, row, variant, ansatz, mass) in enumerate(TABLE):
        c = ls._case(name, ROWS[row], variant, ansatz, seeds.get(name, 12001 + 50 * i))
        c["row"], c["mass"] = row, mass
        out.append(c)
    return out


def problem(c):
    p = ls.problem(c)
    p["mass"] = float(c["mass"])
    return p


def _rel0(a, b):
    return float(np.max(np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))))


def conditions(c, p=None):
    """dict(ok, why, fig) of case c: the module docstring's conditions on the reference alone"""
    p = problem(c) if p is None else p
    fig = {}
    try:
        base = ls.conditions(c, p)
        assert base["ok"], ("the l2 problem", base["why"])
        ratios = [float(d.max() / d.min()) for d in (d_table(p, info) for info in _elements(p))]
        fig["d_ratio"] = max(ratios)
        assert max(ratios) < COND_D, ("max d / min d", ratios)
        ref = reference(p)
        (le_d, rb_d), (le_t, rb_t) = dense_route(p, ref[2]), table_route(p, ref[2])
        fig["routes"] = (_rel0(le_t, le_d), float(np.linalg.norm(rb_t - rb_d) / np.linalg.norm(rb_d)))
        assert max(fig["routes"]) < ls.AGREE, ("table route against dense solve", fig["routes"])
        l3b, gb = reference_autograd(p)
        fig["agree"] = (_rel0(np.asarray(ref[0]), np.asarray(l3b)), float(gp.block_rel(ref[1], gb, p["layers"], p["c0"].size)))
        assert max(fig["agree"]) < ls.AGREE, ("the two derivations under the dual norm", fig["agree"])
        rng = np.random.default_rng(c["seed"] + 41)
        fd = []
        for _ in range(N_FD):
            v = rng.standard_normal(p["full"].size)
            v /= np.linalg.norm(v)
            lp, lm = reference(p, p["full"] + FD_H * v)[0][0], reference(p, p["full"] - FD_H * v)[0][0]
            fd.append(abs((lp - lm) / (2 * FD_H) - ref[1] @ v) / np.linalg.norm(ref[1]))
        fig["fd"] = float(max(fd))
        assert fig["fd"] < FD_TOL, ("central differences", fd)
    except AssertionError as e:
        return dict(ok=False, why=str(e)[:300], fig=fig)
    return dict(ok=True, why="", fig=fig)


# ---- the estimator identity: kappa = 1, beta = sigma = 0, channels from a polynomial ---------------------------------------------------
def _poly(coef, X):
    """(value, gradient (n, dim), Laplacian) of sum_ab coef[a][b] x^a y^b (1-D: coef (n,)) at the points X (n, dim)"""
    P = np.polynomial.polynomial
    if X.shape[1] == 1:
        x = X[:, 0]
        return P.polyval(x, coef), P.polyval(x, P.polyder(coef))[:, None], P.polyval(x, P.polyder(coef, 2))
    x, y = X[:, 0], X[:, 1]
    cx, cy = P.polyder(coef, 1, axis=0), P.polyder(coef, 1, axis=1)
    lap = P.polyval2d(x, y, P.polyder(coef, 2, axis=0)) + P.polyval2d(x, y, P.polyder(coef, 2, axis=1))
    return P.polyval2d(x, y, coef), np.stack([P.polyval2d(x, y, cx), P.polyval2d(x, y, cy)], 1), lap


def estimator_problem(dim, boxes, q, nt, seed, deg=4):
    """Poisson (kappa = 1) on `boxes` with F from the polynomial u and channels from the polynomial pt, both of degree `deg` per
    direction: deg + nt + 1 <= 2 q - 3, so the q-point Lobatto rule integrates every projection exactly"""
    assert deg + nt + 1 <= 2 * q - 3
    from hp_vpinns_amd.testfcn import tables_1d
    rng = np.random.default_rng(seed)
    shape = (deg + 1,) * dim
    cu, cp = rng.standard_normal(shape), rng.standard_normal(shape)
    boxes = np.asarray(boxes, dtype=np.float64)
    xr = lr.rule(q)
    yr = lr.rule(q) if dim == 2 else None
    ne, nty = boxes.shape[0], nt if dim == 2 else 1
    X = lr.quad_points(boxes, xr[0], yr[0] if dim == 2 else None)
    f = _poly(cu, X)[2]                                             # div(grad u) = f
    ax = tables_1d(nt, xr[0])[0] * xr[1][None, :]
    by = tables_1d(nt, yr[0])[0] * yr[1][None, :] if dim == 2 else np.ones((1, 1))
    J = np.prod((boxes[:, 1::2] - boxes[:, 0::2]) / 2, axis=1)
    F = J[:, None, None] * np.einsum("kj,ri,eji->ekr", by, ax, f.reshape(ne, q if dim == 2 else 1, q))
    K, M = ir.n_planes(dim)
    planes = np.zeros((K + M, X.shape[0]))
    planes[:dim] = 1.0                                              # k | kx, ky
    p = dict(prob="p1" if dim == 1 else "p2", dim=dim, boxes=boxes, eb=0, ee=ne, xr=xr, yr=yr, ntx=nt, nty=nty, nax=None, nay=None, F=F,
             mass=0.0)
    return p, planes, cu, cp, X


def estimator_loss(p, planes, cp, X):
    """sum_e loss_e of the dual norm with the channels of the polynomial pt"""
    v, g, _ = _poly(cp, X)
    ch = [torch.tensor(v)] + [torch.tensor(np.ascontiguousarray(g[:, k])) for k in range(p["dim"])]
    with _dual(0.0):
        return float(ir._loss(p, ch, torch.tensor(planes))[2])


def projected_error_energy(p, cu, cp, n_gauss=12):
    """|P_h(pt - u)|^2 in the H^1 seminorm, P_h the orthogonal projection onto each element's bubble space: b_i = (grad(pt - u),
    grad phi_i) by Gauss-Legendre quadrature on the element, b^T G_e^{-1} b by a dense solve -- no Lobatto rule, no test tables"""
    from hp_vpinns_amd.testfcn import Test_fcn, dTest_fcn
    x, w = np.polynomial.legendre.leggauss(n_gauss)
    dim, nt = p["dim"], p["ntx"]
    phi, dphi = Test_fcn(nt, x), dTest_fcn(nt, x)[0]
    total = 0.0
    for e, (nax, nay, Jx, Jy) in enumerate(_elements(p)):
        box = p["boxes"][e:e + 1]
        X = lr.quad_points(box, x, x if dim == 2 else None)
        ge = _poly(cp, X)[1] - _poly(cu, X)[1]
        if dim == 1:
            b = (dphi * w[None, :]) @ ge[:, 0]                     # int e' phi' dx = int e_x (phi' / Jx) Jx dxi
        else:
            ex, ey = ge[:, 0].reshape(n_gauss, n_gauss), ge[:, 1].reshape(n_gauss, n_gauss)      # [j][i]
            b = Jy * np.einsum("kj,ri,ji->kr", phi * w[None, :], dphi * w[None, :], ex) + Jx * np.einsum("kj,ri,ji->kr", dphi * w[None, :], phi * w[None, :], ey)
            b = b.reshape(-1)
        total += float(b @ np.linalg.solve(gram_element(dim, nax, nay, Jx, Jy, 0.0), b))
    return total
