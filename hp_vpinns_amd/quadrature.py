"""Jacobi polynomials and Gauss-Lobatto-Jacobi quadrature rules (host side, numpy only).

Mirrors the public surface of the reference quadrature module
(`Utilities/GaussJacobiQuadRule_V3.py:24-61`): `Jacobi`, `DJacobi`,
`GaussJacobiWeights`, `GaussLobattoJacobiWeights` -- same names, argument order and
return conventions -- but everything is evaluated with the stable three-term
recurrence (never expanded monomial coefficients) and the nodes come from a Newton
iteration on the recurrence instead of scipy's eigenvalue solver, so this file has no
scipy dependency.  Pinned against the reference by `tests/golden/quadrature.npz`.
"""
import math

import numpy as np


def Jacobi(n, a, b, x):
    """P_n^{(a,b)}(x) by the three-term recurrence.  (reference: Q:24-26)

    `x` may be any array-like; the result has the shape of `np.array(x)`.
    n < 0 returns zeros (the reference never asks for it; the test-function code
    guards those terms the same way the reference does, P1:164-183).
    """
    x = np.array(x, dtype=np.float64)
    if n < 0:
        return np.zeros_like(x)
    p0 = np.ones_like(x)
    if n == 0:
        return p0
    p1 = 0.5 * ((a - b) + (a + b + 2.0) * x)
    if n == 1:
        return p1
    for k in range(1, n):
        # 2(k+1)(k+a+b+1)(2k+a+b) P_{k+1} =
        #   (2k+a+b+1)[(2k+a+b+2)(2k+a+b) x + a^2-b^2] P_k - 2(k+a)(k+b)(2k+a+b+2) P_{k-1}
        c = 2.0 * k + a + b
        a1 = 2.0 * (k + 1.0) * (k + a + b + 1.0) * c
        a2 = (c + 1.0) * (a * a - b * b)
        a3 = c * (c + 1.0) * (c + 2.0)
        a4 = 2.0 * (k + a) * (k + b) * (c + 2.0)
        p2 = ((a2 + a3 * x) * p1 - a4 * p0) / a1
        p0, p1 = p1, p2
    return p1


def DJacobi(n, a, b, x, k: int):
    """k-th derivative of P_n^{(a,b)}.  (reference: Q:30-33)"""
    x = np.array(x, dtype=np.float64)
    if k > n:
        return np.zeros_like(x)
    ctemp = math.gamma(a + b + n + 1 + k) / (2 ** k) / math.gamma(a + b + n + 1)
    return ctemp * Jacobi(n - k, a + k, b + k, x)


def _jacobi_roots(n, a, b):
    """Roots of P_n^{(a,b)} by Newton with polynomial deflation-free updates.

    Uses the classical simultaneous (Aberth-like) correction so that every root
    converges to a distinct zero; initial guesses are Chebyshev points.
    """
    if n <= 0:
        return np.zeros(0)
    k = np.arange(n, dtype=np.float64)
    x = -np.cos((2.0 * k + 1.0) * math.pi / (2.0 * n))
    for _ in range(100):
        p = Jacobi(n, a, b, x)
        dp = DJacobi(n, a, b, x, 1)
        diff = x[:, None] - x[None, :]
        np.fill_diagonal(diff, 1.0)
        s = (1.0 / diff).sum(axis=1) - 1.0  # remove the diagonal's 1/1
        dx = p / (dp - s * p)
        x = x - dx
        if np.max(np.abs(dx)) < 1e-16:
            break
    # two plain Newton polish steps (quadratic, removes the Aberth coupling error)
    for _ in range(2):
        x = x - Jacobi(n, a, b, x) / DJacobi(n, a, b, x, 1)
    x = np.sort(x)
    if a == b:  # symmetric weight: enforce exact symmetry like an eigen-solver would not
        x = 0.5 * (x - x[::-1])
    return x


def GaussJacobiWeights(Q: int, a, b):
    """Gauss-Jacobi nodes and weights.  (reference: Q:38-40; imported but never called)"""
    X = _jacobi_roots(Q, a, b)
    # w_i = Gamma(a+Q+1)Gamma(b+Q+1)/(Gamma(a+b+Q+1) Q!) * 2^{a+b+1} / ((1-x^2) P'_Q(x)^2)
    lg = (math.lgamma(a + Q + 1) + math.lgamma(b + Q + 1)
          - math.lgamma(a + b + Q + 1) - math.lgamma(Q + 1))
    c = math.exp(lg) * 2.0 ** (a + b + 1)
    W = c / ((1.0 - X * X) * DJacobi(Q, a, b, X, 1) ** 2)
    return [X, W]


def GaussLobattoJacobiWeights(Q: int, a, b):
    """Gauss-Lobatto-Jacobi nodes (endpoints included) and weights.  (reference: Q:46-61)

    Interior nodes are the roots of P_{Q-2}^{(a+1,b+1)}; the Legendre case (a=b=0, the
    only one the drivers use: P1:260, P2:355, P3:395) has weights 2/((Q-1) Q P_{Q-1}(x)^2).
    """
    X = _jacobi_roots(Q - 2, a + 1, b + 1)
    if a == 0 and b == 0:
        W = 2 / ((Q - 1) * (Q) * (Jacobi(Q - 1, 0, 0, X) ** 2))
        Wl = 2 / ((Q - 1) * (Q) * (Jacobi(Q - 1, 0, 0, -1) ** 2))
        Wr = 2 / ((Q - 1) * (Q) * (Jacobi(Q - 1, 0, 0, 1) ** 2))
    else:
        g = math.gamma
        c = 2 ** (a + b + 1) * g(a + Q) * g(b + Q) / ((Q - 1) * g(Q) * g(a + b + Q + 1))
        W = c / (Jacobi(Q - 1, a, b, X) ** 2)
        Wl = (b + 1) * c / (Jacobi(Q - 1, a, b, -1) ** 2)
        Wr = (a + 1) * c / (Jacobi(Q - 1, a, b, 1) ** 2)
    W = np.append(W, Wr)
    W = np.append(Wl, W)
    X = np.append(X, 1)
    X = np.append(-1, X)
    return [X, W]


def diff_matrix(x):
    """Differentiation matrix of the distinct nodes `x`: (D v)[i] = p'(x_i) for the polynomial p of degree < len(x) with
    p(x_m) = v[m].  Barycentric form -- D[i][m] = (lam_m / lam_i) / (x_i - x_m) off the diagonal, lam_i = 1 / prod_{m != i}
    (x_i - x_m) -- with the diagonal as the negative sum of the row's other entries, which makes the derivative of a constant
    exactly zero.  Raises ValueError on repeated nodes (e.g. a zero-weight padded rule): their interpolant does not exist."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    if n < 1:
        raise ValueError("diff_matrix needs at least one node")
    dx = x[:, None] - x[None, :]
    np.fill_diagonal(dx, 1.0)
    if np.any(dx == 0.0):
        raise ValueError("diff_matrix needs distinct nodes (a padded rule repeats some)")
    lam = 1.0 / np.prod(dx, axis=1)
    D = (lam[None, :] / lam[:, None]) / dx
    np.fill_diagonal(D, 0.0)
    np.fill_diagonal(D, -D.sum(axis=1))
    return D


# ---- the Gram matrices of the test functions phi_n = P_{n+1} - P_{n-1}, n = 1 .. N, on the reference interval ------------------------
def gram_1d(n):
    """(K, M) of the first n test functions, exact closed forms: the stiffness K = int phi_i' phi_j' = diag(2 (2 i + 1)) (because
    phi_i' = (2 i + 1) P_i) and the mass M = int phi_i phi_j with M_ii = 2 / (2 i + 3) + 2 / (2 i - 1), M_i,i+2 = -2 / (2 i + 3)
    (indices 1-based)."""
    n = int(n)
    if n < 1:
        raise ValueError("gram_1d needs at least one test function")
    i = np.arange(1, n + 1, dtype=np.float64)
    K = np.diag(2.0 * (2.0 * i + 1.0))
    M = np.diag(2.0 / (2.0 * i + 3.0) + 2.0 / (2.0 * i - 1.0))
    for j in range(n - 2):
        M[j, j + 2] = M[j + 2, j] = -2.0 / (2.0 * i[j] + 3.0)
    return K, M


def gram_eig(n):
    """(S, lam) of the generalised problem K S = M S diag(lam) with S^T M S = I (so S^T K S = diag(lam)), lam ascending: a symmetric
    eigen-solve of K^{-1/2} M K^{-1/2} = V diag(mu) V^T (K is diagonal), lam = 1 / mu, S = K^{-1/2} V diag(mu^{-1/2})."""
    K, M = gram_1d(n)
    k = 1.0 / np.sqrt(np.diag(K))
    mu, V = np.linalg.eigh(k[:, None] * M * k[None, :])
    order = np.argsort(-mu)                      # (lam ascending)
    mu, V = mu[order], V[:, order]
    S = (k[:, None] * V) / np.sqrt(mu)[None, :]
    S *= np.where(S[np.argmax(np.abs(S), axis=0), np.arange(S.shape[1])] < 0.0, -1.0, 1.0)[None, :]      # (a fixed sign per column)
    return S, 1.0 / mu


def gram_stacks(nt):
    """(S_stack (nt, nt, nt), lam_stack (nt, nt)): gram_eig of every count 1 .. nt, count n at [n - 1] in the leading n x n block,
    zero-padded -- per-element counts use the leading functions, and S of n functions is not a sub-block of S of n + 1
    (hpv_set_residual_norm)."""
    nt = int(nt)
    S, lam = np.zeros((nt, nt, nt)), np.zeros((nt, nt))
    for n in range(1, nt + 1):
        S[n - 1, :n, :n], lam[n - 1, :n] = gram_eig(n)
    return S, lam


# ---- dense Gram factors: the inner products whose Gram matrix is no Kronecker sum (hpv_set_residual_gram) ----------------------------
def gram_rule(ntx, nty=1, gram_points=None):
    """(nodes, weights) of the Gram matrices' own Gauss-Legendre rule: max(ntx, nty) + 3 points per direction unless `gram_points`
    says otherwise -- exact for a constant weight tensor on affine elements (degree 2 nt + 2 <= 2 nt + 5).  Not the handle's Lobatto
    rule: that one may under-integrate the test functions' products and leave the matrix singular."""
    n = max(int(ntx), int(nty)) + 3 if gram_points is None else int(gram_points)
    if n < 1:
        raise ValueError("gram_points is a positive number of Gauss-Legendre points per direction")
    return np.polynomial.legendre.leggauss(n)


def gram_factors(dim, ntx, nty, nax, nay, A, S=None, mass=0.0, gram_points=None, first=0):
    """W (n, NR, NR), NR = ntx * nty: per element the inverse Cholesky factor W_e = L_e^{-1} of the Gram matrix G_e = L_e L_e^T of its
    ACTIVE test functions phi_kr = phi_r(xi) phi_k(eta), r < nax[e], k < nay[e], in the inner product

        G_e[(k, r), (k', r')] = sum_g w_g [ grad^ phi_kr^T C_g grad^ phi_k'r' + m_g phi_kr phi_k'r' ]
        C = adj(A) S adj(A)^T / det A          m = mass det A                  (1-D: C = S / Jx, m = mass Jx)

    at the points of `gram_rule` (g = j * n_gram + i in 2-D), so that loss_e = |W_e R_e|^2 = R_e^T G_e^{-1} R_e.  W_e is row-major in
    the full index k * ntx + r (the order of R[k][r]), lower triangular, exactly zero in the rows and columns of inactive functions:
    a sub-selection of indices keeps its order, so it is a valid inverse factor of the active sub-matrix.
    A: the Jacobian of each element's map with respect to its reference coordinates at the Gram points -- 2-D (n, n_gram^2, 2, 2),
    1-D (n, n_gram) (= Jx); boxes are diag(Jx, Jy).  S: the physical weight tensor there, None for the identity (the physical H^1
    product), else sym(K) of (n, n_gram^2, 2, 2) / the diagonal of (n, n_gram^2, 2) / the scalars of (n, n_gram) in 1-D (the energy
    product).  Assembled by sum factorisation, numpy only.  ValueError naming the element (numbered from `first`) where S is not
    positive definite at a Gram point or the Cholesky factorisation fails."""
    from .testfcn import Test_fcn, dTest_fcn
    dim, ntx, nty = int(dim), int(ntx), int(nty)
    x, w = gram_rule(ntx, nty, gram_points)
    ng = x.size
    A = np.asarray(A, dtype=np.float64)
    ne = A.shape[0]
    if A.shape != ((ne, ng) if dim == 1 else (ne, ng * ng, 2, 2)):
        raise ValueError(f"A has shape {A.shape}; expected {(ne, ng) if dim == 1 else (ne, ng * ng, 2, 2)}")
    nax = np.broadcast_to(np.asarray(nax, dtype=np.int64), (ne,))
    nay = np.broadcast_to(np.asarray(nay, dtype=np.int64), (ne,))
    NR = ntx * nty
    W = np.zeros((ne, NR, NR))
    px, dpx = Test_fcn(ntx, x), dTest_fcn(ntx, x)[0]
    if dim == 2:
        py, dpy = Test_fcn(nty, x), dTest_fcn(nty, x)[0]
        if S is not None:
            S = np.asarray(S, dtype=np.float64)
            if S.shape == (ne, ng * ng, 2):
                S = S[..., None] * np.eye(2)
            if S.shape != (ne, ng * ng, 2, 2):
                raise ValueError(f"S has shape {S.shape}; expected {(ne, ng * ng, 2, 2)} or {(ne, ng * ng, 2)}")
            S = 0.5 * (S + S.transpose(0, 1, 3, 2))
    elif S is not None:
        S = np.asarray(S, dtype=np.float64).reshape(ne, ng)
    I = np.eye(NR)
    for e in range(ne):
        na, nb = int(nax[e]), int(nay[e])
        if dim == 1:
            s = np.ones(ng) if S is None else S[e]
            if not np.all(s > 0.0):
                raise ValueError(f"element {first + e}: kappa is {s.min():.6g} at a Gram point; the energy inner product needs kappa > 0")
            G = np.einsum("i,ri,si->rs", w * s / A[e], dpx[:na], dpx[:na]) + np.einsum("i,ri,si->rs", w * mass * A[e], px[:na], px[:na])
        else:
            a = A[e]
            det = a[:, 0, 0] * a[:, 1, 1] - a[:, 0, 1] * a[:, 1, 0]
            adj = np.stack([np.stack([a[:, 1, 1], -a[:, 0, 1]], 1), np.stack([-a[:, 1, 0], a[:, 0, 0]], 1)], 1)
            if S is None:
                C = np.einsum("gab,gcb->gac", adj, adj) / det[:, None, None]
            else:
                s = S[e]
                lo = 0.5 * (s[:, 0, 0] + s[:, 1, 1]) - np.sqrt((0.5 * (s[:, 0, 0] - s[:, 1, 1])) ** 2 + s[:, 0, 1] ** 2)
                if not np.all(lo > 0.0):
                    raise ValueError(f"element {first + e}: the smallest eigenvalue of sym(kappa) is {lo.min():.6g} at a Gram point; "
                                     "the energy inner product needs a positive definite kappa")
                C = np.einsum("gab,gbc,gdc->gad", adj, s, adj) / det[:, None, None]
            C = C.reshape(ng, ng, 2, 2)                                  # [j][i]
            m = (mass * det).reshape(ng, ng)
            X, Y = (px[:na], dpx[:na]), (py[:nb], dpy[:nb])              # [derivative order][function][point]
            G = np.zeros((nb, na, nb, na))
            # (a, b): the reference derivative taken of the first / the second function -- 0: d/dxi (x table differentiated), 1: d/deta
            for ca, cb, c in ((0, 0, C[:, :, 0, 0]), (0, 1, C[:, :, 0, 1]), (1, 0, C[:, :, 1, 0]), (1, 1, C[:, :, 1, 1]), (2, 2, m)):
                T = np.einsum("ji,ri,si->jrs", c * w[None, :], X[ca == 0], X[cb == 0])      # the x direction, per row j of points
                G += np.einsum("j,kj,lj,jrs->krls", w, Y[ca == 1], Y[cb == 1], T)
            G = G.reshape(nb * na, nb * na)
        try:
            L = np.linalg.cholesky(0.5 * (G + G.T))
        except np.linalg.LinAlgError:
            raise ValueError(f"element {first + e}: the Gram matrix of its {na} x {nb} test functions is not positive definite "
                             "(Cholesky failed): a degenerate element, or too few gram_points") from None
        idx = (np.arange(nb)[:, None] * ntx + np.arange(na)[None, :]).reshape(-1)
        # W_e = L^{-1}: forward substitution against the identity, row by row (numpy has no triangular solve)
        n = L.shape[0]
        Wi = np.zeros((n, n))
        for i in range(n):
            Wi[i] = (I[i, :n] - L[i, :i] @ Wi[:i]) / L[i, i]
        W[e][np.ix_(idx, idx)] = np.tril(Wi)
    return W
