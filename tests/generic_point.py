"""Generic points of the input space for the parity tests (a plain helper module like cases.py; no GPU needed).

Almost every parity case of the suite sits at one special point: uniform grids (every element has the same J, Jx, Jy: a wrong
element index reads the right number), Xavier initial parameters with all biases zero (an odd tanh network on a symmetric domain),
V = 1 (the weights of u_x and u_t cannot be told apart), lossb_weight = 10, the default Adam constants.  The builders here move a
`setup()` dict of the drivers away from all of them:

  warp            non-uniform grids -- no two elements share a coefficient;
  generic_theta   Xavier + 0.3 N(0,1) on EVERY weight and bias;
  block_rel       the gradient error per parameter block (W_l, b_l, epsilon), not one global norm: at such a point the block norms of
                  the default network span two orders of magnitude, and d/d epsilon is 1e-3 of the total;
  warp_poisson2d / warp_advdiff / warp_poisson1d   the setup dict on warped grids with F recomputed (numpy, the expression of the
                  driver's own loop) or seeded random, and the positional argument tuples of the classes.
"""
import numpy as np

BLOCK_FLOOR = 1e-4      # every oracle block norm must be at least this fraction of the oracle gradient norm (else: ill-posed case)


def warp(grid, rng):
    """The grid with its end points kept and the cell widths drawn from U(0.5, 1.5), rescaled to the span: neighbouring Jacobians
    differ by up to 3x."""
    grid = np.asarray(grid, dtype=np.float64)
    n = grid.size - 1
    if n < 2:
        return grid.copy()
    w = rng.uniform(0.5, 1.5, n)
    w *= (grid[-1] - grid[0]) / w.sum()
    out = grid[0] + np.concatenate([[0.0], np.cumsum(w)])
    out[-1] = grid[-1]
    assert np.all(np.diff(out) > 0) and len(set(np.round(np.diff(out), 12))) == n
    return out


def generic_theta(layers, seed, extra=(), scale=0.3):
    """xavier_init plus `scale` N(0,1) on every weight and every bias; the trailing extras (epsilon) as given.  (0.3 on a 64-wide
    tanh layer saturates it: tests/shape_matrix.py passes a smaller scale at the wider layers.)"""
    from hp_vpinns_amd.init import n_params, xavier_init
    layers = [int(v) for v in layers]
    th = xavier_init(layers, seed, extra=extra)
    n = n_params(layers)
    th[:n] += scale * np.random.default_rng(seed + 100003).standard_normal(n)
    return th


def blocks(layers, n_extra=0):
    """[(name, lo, hi)] of the packed parameter vector: W_l, b_l per layer, then `eps`."""
    out, o = [], 0
    for l in range(len(layers) - 1):
        i, j = int(layers[l]), int(layers[l + 1])
        out.append(("W%d" % l, o, o + i * j)); o += i * j
        out.append(("b%d" % l, o, o + j)); o += j
    if n_extra:
        out.append(("eps", o, o + n_extra))
    return out


def block_errors(g, g_ref, layers, n_extra=0):
    """{name: relative 2-norm error of that block}; asserts that no block is negligible in the reference gradient (such a case is
    ill-posed: it would compare round-off)."""
    g, g_ref = np.asarray(g, dtype=np.float64).ravel(), np.asarray(g_ref, dtype=np.float64).ravel()
    bl = blocks(layers, n_extra)
    assert g.size == g_ref.size == bl[-1][2], (g.size, g_ref.size, bl[-1][2])
    total = np.linalg.norm(g_ref)
    out = {}
    for name, lo, hi in bl:
        nb = np.linalg.norm(g_ref[lo:hi])
        assert nb >= BLOCK_FLOOR * total, "ill-posed case: block %s has norm %.3e of a gradient of norm %.3e" % (name, nb, total)
        out[name] = float(np.linalg.norm(g[lo:hi] - g_ref[lo:hi]) / nb)
    return out


def block_rel(g, g_ref, layers, n_extra=0):
    """The largest per-block relative 2-norm error (see block_errors)."""
    return max(block_errors(g, g_ref, layers, n_extra).values())


def worst_block(g, g_ref, layers, n_extra=0):
    e = block_errors(g, g_ref, layers, n_extra)
    k = max(e, key=e.get)
    return k, e[k]


# ---- right-hand sides --------------------------------------------------------------------------------------------------------
def poisson2d_F(grid_x, grid_y, ntx, nty, q):
    """F_ext_total of the Poisson-2D driver on any tensor grid, vectorised: F[ex, ey][k][r] = Jx Jy sum_ji w_j phi_k(xi_j) f(x_i, y_j)
    w_i phi_r(xi_i) -- the expression of the driver's element loop."""
    from hp_vpinns_amd import GaussLobattoJacobiWeights, Test_fcn
    from hp_vpinns_amd.drivers.poisson2d import f_ext
    gx, gy = np.asarray(grid_x, dtype=np.float64), np.asarray(grid_y, dtype=np.float64)
    X, W = GaussLobattoJacobiWeights(q, 0, 0)
    ax, by = Test_fcn(ntx, X) * W, Test_fcn(nty, X) * W
    jx, jy = (gx[1:] - gx[:-1]) / 2, (gy[1:] - gy[:-1]) / 2
    xq = gx[:-1, None] + jx[:, None] * (X[None, :] + 1)             # [ex][i]
    yq = gy[:-1, None] + jy[:, None] * (X[None, :] + 1)             # [ey][j]
    fq = f_ext(xq[:, None, None, :], yq[None, :, :, None])          # [ex][ey][j][i]
    return (jx[:, None] * jy[None, :])[:, :, None, None] * np.einsum("kj,abji,ri->abkr", by, fq, ax)


def random_F(shape, seed):
    """A seeded right-hand side without any symmetry, of the size of the driver's own (|F| ~ 1)."""
    return np.random.default_rng(seed).standard_normal(shape)


# ---- builders ----------------------------------------------------------------------------------------------------------------
def warp_poisson2d(s, seed, F="recomputed"):
    """A poisson2d.setup() dict (uniform test-function counts) on warped grids; F: 'recomputed' | 'random'."""
    rng = np.random.default_rng(seed)
    s = dict(s)
    s["grid_x"], s["grid_y"] = warp(s["grid_x"], rng), warp(s["grid_y"], rng)
    ntx, nty = max(s["N_testfcn_total"][0]), max(s["N_testfcn_total"][1])
    q = int(round(np.sqrt(s["XY_quad_train"].shape[0])))
    Fd = poisson2d_F(s["grid_x"], s["grid_y"], ntx, nty, q) if F == "recomputed" else random_F((len(s["grid_x"]) - 1, len(s["grid_y"]) - 1, nty, ntx), seed + 1)
    nax, nay = s["N_testfcn_total"]
    if len(set(nax)) > 1 or len(set(nay)) > 1:     # per-element counts: what the reference class indexes with [ex, ey]
        bl = np.empty(Fd.shape[:2], dtype=object)
        for ex in range(Fd.shape[0]):
            for ey in range(Fd.shape[1]):
                bl[ex, ey] = Fd[ex, ey][:nay[ey], :nax[ex]].copy()
        Fd = bl
    s["F_ext_total"] = Fd
    return s


def warp_advdiff(s, seed, both=True):
    """An advdiff.setup() dict on a warped grid_x (and grid_t when `both`)."""
    rng = np.random.default_rng(seed)
    s = dict(s)
    s["grid_x"] = warp(s["grid_x"], rng)
    if both:
        s["grid_t"] = warp(s["grid_t"], rng)
    return s


def warp_poisson1d(s, seed, grid=None):
    """A poisson1d.setup() dict (equal counts) on a warped grid (or on `grid`), F recomputed with the driver's expression."""
    from hp_vpinns_amd import Test_fcn
    from hp_vpinns_amd.drivers.poisson1d import f_ext
    rng = np.random.default_rng(seed)
    s = dict(s)
    g = warp(s["grid"], rng) if grid is None else np.asarray(grid, dtype=np.float64)
    x, w = s["X_quad_train"][:, 0], s["W_quad_train"][:, 0]
    nt = np.asarray(s["F_ext_total"]).shape[1]
    t = Test_fcn(nt, x)
    J = (g[1:] - g[:-1]) / 2
    xq = g[:-1, None] + J[:, None] * (x[None, :] + 1)
    s["grid"] = g
    s["F_ext_total"] = (J[:, None] * ((w * f_ext(xq)) @ t.T))[:, :, None]
    return s


def data_subset(X, u, n, seed=0):
    """n of the data points (seeded choice, n <= len): the data tiles' tail cases."""
    idx = np.sort(np.random.default_rng(seed).choice(len(X), n, replace=False))
    return np.ascontiguousarray(X[idx]), np.ascontiguousarray(np.asarray(u)[idx])


def p2_tuple(s, layers):
    """positional arguments of VPINN2D / OracleVPINN2D"""
    return (s["X_u_train"], s["u_train"], s["X_f_train"], s["f_train"], s["XY_quad_train"], s["WXY_quad_train"], None,
            s["F_ext_total"], s["grid_x"], s["grid_y"], s["N_testfcn_total"], s["X_u_train"], s["u_train"], list(layers))


def p3_tuple(s, layers):
    """positional arguments of VPINNAdvDiff / OracleVPINNAdvDiff"""
    return (s["XT_u_train"], s["u_train"], s["XT_f_train"], s["XT_quad_train"], s["WXT_quad_train"], s["T_quad"], s["WT_quad"],
            s["grid_x"], s["grid_t"], s["N_testfcn_total"], s["XT_u_train"], s["u_train"], list(layers), None, None)


def p1_tuple(s, layers):
    """positional arguments of VPINN1D / OracleVPINN1D"""
    return (s["X_u_train"], s["u_train"], s["X_quad_train"], s["W_quad_train"], s["F_ext_total"], s["grid"], s["X_test"],
            s["u_test"], list(layers), s["X_f_train"], s["f_train"])
