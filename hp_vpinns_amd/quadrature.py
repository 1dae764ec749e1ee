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
