"""tests/linadapt_reference.py and its inputs, proved on the CPU (no GPU): the differentiation matrix, the strong residual of the
reference against the analytic one for a polynomial kappa, a piecewise-constant kappa with its jump on an element edge, and the
well-posedness of every case tests/test_gpu_linadapt.py runs.  The measured figures are in profiles/linear_adaptivity.md."""
import numpy as np
import pytest

import linadapt_reference as la
import linear_reference as lr
from hp_vpinns_amd.quadrature import diff_matrix

# (a): measured worst |D x^k - k x^(k-1)| over k < q, at the GLL nodes: q = 3 -> 0, 5 -> 8.9e-16, 11 -> 1.0e-14, 20 -> 5.7e-14; the
# bound is 100x the largest (q = 20).  Row sums, measured: 0, 2.2e-16, 1.2e-15, 3.4e-15 (the diagonal is the negative sum of the
# row's other entries; what is left is the rounding of summing the row again); 100x the largest.
DIFF_BOUND = 5.7e-12
ROWSUM_BOUND = 3.4e-13
# (b): measured |r_reference - r_analytic| / max|r|: 9.3e-16 (7 x 5), 6.7e-15 (17 x 16), 2.8e-14 (33 points, 1-D); 100x the largest.
POLY_BOUND = 2.8e-12
# (c): measured worst |dk| / |kappa| in an element whose neighbours hold other values: 7.0e-13 (33 points: the entries of D reach
# q^2 / 2 and 1 / Jx = 5.7); 100x.
JUMP_BOUND = 7.0e-11
FLOOR = 1e-3       # (d): the share below which a column or a term would be compared at round-off level


def _monomial_error(q):
    x = lr.rule(q)[0]
    D = diff_matrix(x)
    err = 0.0
    for k in range(q):
        exact = k * x ** (k - 1) if k else np.zeros_like(x)
        err = max(err, float(np.abs(D @ x ** k - exact).max()))
    return err, float(np.abs(D.sum(axis=1)).max())


@pytest.mark.parametrize("q", [3, 5, 11, 20])
def test_diff_matrix_differentiates_polynomials_exactly(q):
    err, rows = _monomial_error(q)
    print("diff_matrix q = %d: worst monomial error %.2e, worst row sum %.2e" % (q, err, rows))
    assert err < DIFF_BOUND and rows < ROWSUM_BOUND


def test_diff_matrix_refuses_repeated_nodes():
    x = lr.rule(6, pad=1)[0]                                      # (a padded rule repeats its last node)
    with pytest.raises(ValueError):
        diff_matrix(x)
    with pytest.raises(ValueError):
        diff_matrix([0.0, 0.5, 0.5])
    D = diff_matrix([-1.0, 0.0, 1.0])
    assert np.allclose(D, [[-1.5, 2.0, -0.5], [-0.5, 0.0, 0.5], [0.5, -2.0, 1.5]], rtol=0, atol=1e-15)


def _poly(P, qx, qy):
    """kx, ky of degree qx - 1 in x and qy - 1 in y (Chebyshev polynomials: bounded on [-1, 1]) with their analytic derivatives"""
    from numpy.polynomial import chebyshev as ch
    x = P[:, 0]
    y = P[:, 1] if P.shape[1] == 2 else np.zeros_like(x)
    cx, cy = np.zeros(qx), np.zeros(max(qy, 1))
    cx[0], cx[qx - 1], cy[0] = 1.3, 0.4, 1.0
    if qy > 1:
        cy[qy - 1] = 0.3
    kx = ch.chebval(x, cx) * ch.chebval(y, cy)
    dkx = ch.chebval(x, ch.chebder(cx)) * ch.chebval(y, cy)
    ky = 0.8 * kx + 0.2
    dky = 0.8 * ch.chebval(x, cx) * (ch.chebval(y, ch.chebder(cy)) if qy > 1 else 0.0)
    return kx, ky, dkx, dky


@pytest.mark.parametrize("name", ["2d-7x5", "2d-17x16-counts", "1d-33-counts"])
def test_polynomial_kappa_gives_the_analytic_strong_residual(name):
    p = la.problem(la.CASES[name])
    dim, b = p["dim"], p["boxes"][p["eb"]:p["ee"]]
    xi, yi = p["xr"][0], (p["yr"][0] if dim == 2 else None)
    P = lr.quad_points(b, xi, yi)
    sh = (b.shape[0], 1 if yi is None else yi.size, xi.size)
    kx, ky, dkx, dky = _poly(P, xi.size, 0 if yi is None else yi.size)
    if dim == 2:
        p["planes"][0], p["planes"][1] = kx, ky
    else:
        p["planes"][0] = kx
    ref = la.strong_parts(p)
    exact = la.strong_parts(p, dk=(dkx.reshape(sh), dky.reshape(sh) if dim == 2 else None))
    err = float(np.abs(ref["r"] - exact["r"]).max() / np.abs(exact["r"]).max())
    print("%s: polynomial kappa, |r_reference - r_analytic| / max|r| = %.2e; share of dk terms %.2e"
          % (name, err, np.abs(exact["dkx"]).max() / np.abs(exact["r"]).max()))
    assert np.abs(exact["dkx"]).max() > FLOOR * np.abs(exact["r"]).max()      # (the term under test is there)
    assert err < POLY_BOUND


def test_piecewise_constant_kappa_with_the_jump_on_an_element_edge():
    worst = 0.0
    for name in ("2d-7x5", "1d-33-counts"):
        p = la.problem(la.CASES[name])
        ne = p["ee"] - p["eb"]
        nq = p["planes"].shape[1] // ne
        vals = np.array([1.0, 7.5, 0.2, 3.0, 11.0])[:ne]                       # one value per element: every edge is a jump
        k = np.repeat(vals, nq)
        sh = (ne, 1 if p["dim"] == 1 else p["yr"][0].size, p["xr"][0].size)
        dkx, dky = la.plane_derivatives(p, k.reshape(sh), k.reshape(sh) if p["dim"] == 2 else None)
        for d in (dkx, dky):
            if d is not None:
                worst = max(worst, float((np.abs(d) / vals[:, None, None]).max()))
    print("piecewise-constant kappa: worst |dk| / |kappa| = %.2e" % worst)
    assert worst < JUMP_BOUND


def _check_case(name, p):
    ref = la.reference(p)
    ind, parts = ref["ind"], ref["parts"]
    col = np.abs(ind).max(axis=0)
    cols = [c for c in range(5) if not (p["dim"] == 1 and c == 4)]
    share = col[cols] / col.max()
    rmax = np.abs(parts["r"]).max()
    terms = {k: float(np.abs(v).max() / rmax) for k, v in parts.items() if k in ("dkx", "dky", "N", "f")}
    print("%s: column shares %s, term shares %s" % (name, np.array2string(share, precision=2), {k: "%.2e" % v for k, v in terms.items()}))
    assert share.min() >= FLOOR, (name, share)
    assert np.all(ind[:, cols] > 0.0)
    if p["dim"] == 1:
        assert np.all(ind[:, 4] == 0.0)
    assert min(terms.values()) >= FLOOR, (name, terms)
    has_n = bool(p["terms"]) or bool(np.any(p["dirs"][:, p["planes"].shape[0]:] != 0.0))      # (a base term, or a direction on one)
    assert ("dky" in terms) == (p["dim"] == 2) and ("N" in terms) == has_n
    return ref


@pytest.mark.parametrize("name", list(la.CASES) + ["twin"])
def test_gpu_cases_are_well_posed(name):
    if name == "twin":
        p = la.twin_problem()
        ref = la.reference(p)
        col = np.abs(ref["ind"]).max(axis=0)
        print("twin: column shares %s" % np.array2string(col / col.max(), precision=2))
        assert (col / col.max()).min() >= FLOOR                                # (kappa = 1: no dk term to ask for)
        return
    _check_case(name, la.problem(la.CASES[name]))


def test_transposed_dy_or_a_dropped_term_is_visible():
    """what (d) is for: on the qx != qy case, Dy applied along the wrong axis of a square sub-block, or a term left out, moves r by far
    more than the GPU test's tolerance"""
    p = la.problem(la.CASES["nl-6x6-exp-adv"])
    ref = la.strong_parts(p)
    wrong = la.strong_parts(p, Dy=la.diff(p["yr"][0]).T.copy())
    rmax = np.abs(ref["r"]).max()
    assert np.abs(wrong["r"] - ref["r"]).max() > FLOOR * rmax
    for k in ("dkx", "dky", "N", "f"):
        assert np.abs(ref[k]).max() > FLOOR * rmax


def test_the_marked_set_of_the_class_case_is_stable():
    from hp_vpinns_amd.adapt import ElementMesh, mark
    p = la.class_problem()
    ref = _check_case("class", p)
    mesh = ElementMesh(p["boxes"], p["ntx"])
    base = mark(ref["ind"], mesh)
    assert base, "the class case marks something"
    rng = np.random.default_rng(5)
    for _ in range(20):
        pert = ref["ind"] * (1.0 + 1e-6 * rng.choice([-1.0, 1.0], ref["ind"].shape))
        assert mark(pert, mesh) == base
    print("class case: marked", base)
