"""tests/nonlinear_reference.py on the CPU alone: its cases tell a skipped term, a wrong plane or a wrong channel apart (the conditions
the GPU test asserts again before it reads a device number), its gradient is the derivative of its loss, it is linear_reference at
N = 0, and the adjoint formulas of include/hpvpinn.h / csrc/kernels_nonlin.hip restated in numpy are autograd's.  Also the host side of
the class and the driver: the Bratu closed form, `_coef_field` on `advection`, the drivers' setup().  No GPU needed."""
import numpy as np
import pytest

import linear_reference as lr
import nonlinear_reference as nr
from cases import rel


@pytest.mark.parametrize("name", list(nr.CASES))
def test_conditions_on_the_reference_alone(name):
    p = nr.problem(nr.CASES[name])
    fig = nr.conditions(p)
    print(name, fig)
    rows = nr.term_rows(p["dim"])
    for t in nr.TERMS:                      # an absent term is a plane of exact zeros: what the host turns into the mask
        assert np.any(p["nl"][rows[t]] != 0.0) == (t in p["terms"])
    R = nr.var_part(p)["R"]
    if p["nax"] is not None:
        nax = p["nax"][p["eb"]:p["ee"]]
        assert all(np.all(R[e][:, nax[e]:] == 0.0) for e in range(R.shape[0]))


@pytest.mark.parametrize("name", ["2d-h8-counts-flux", "1d-sin", "only-exp"])
def test_gradient_against_central_differences(name):
    p = nr.problem(nr.CASES[name])
    _, g, _ = nr.reference(p)
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(4):
        d = rng.standard_normal(g.size)
        d /= np.linalg.norm(d)
        h = 1e-5
        fd = (nr.reference(p, p["theta"] + h * d)[0][0] - nr.reference(p, p["theta"] - h * d)[0][0]) / (2 * h)
        worst = max(worst, abs(fd - g @ d) / abs(g @ d))
    print(name, "directional derivative against central differences: %.2e" % worst)
    assert worst < 1e-6       # the tolerance of tests/test_linear_host.py: h^2 |f'''| / 6 ~ 1e-10 plus rounding eps |f| / h ~ 1e-10


@pytest.mark.parametrize("name", ["2d-h8-counts-flux", "1d-sin"])
def test_zero_planes_are_the_linear_reference_exactly(name):
    p = nr.problem(nr.CASES[name])
    l3, g, R = nr.reference(p, nl=np.zeros_like(p["nl"]))
    l3o, go, Ro = lr.reference(p)
    assert np.array_equal(l3, l3o) and np.array_equal(g, go) and np.array_equal(R, Ro)
    assert nr.reference(p)[0][2] != l3o[2]


@pytest.mark.parametrize("name", ["2d-h8-counts-flux", "1d-sin", "lds-21x21-padded"])
def test_adjoint_formulas_restated_in_numpy(name):
    """GBAR[u] = (s + dN/du) g0, GBAR[u_x] = kx g1 + (bx + gx u) g0, GBAR[u_y] = ky g2 + (by + gy u) g0 with g_t = d lossv / d G_t"""
    p = nr.problem(nr.CASES[name])
    a = nr.channel_adjoints(p)
    u, ux = a["ch"][0], a["ch"][1]
    g0, g1 = a["g"][0], a["g"][1]
    a2, a3, ae = p["nl"][:3]
    if p["dim"] == 2:
        uy, g2 = a["ch"][2], a["g"][2]
        kx, ky, bx, by, s = p["planes"]
        gx, gy = p["nl"][3:]
        dN = 2 * a2 * u + 3 * a3 * u ** 2 + ae * np.exp(u) + gx * ux + gy * uy
        gbar = [(s + dN) * g0, kx * g1 + (bx + gx * u) * g0, ky * g2 + (by + gy * u) * g0]
    else:
        k, b, s = p["planes"]
        gx = p["nl"][3]
        dN = 2 * a2 * u + 3 * a3 * u ** 2 + ae * np.exp(u) + gx * ux
        gbar = [(s + dN) * g0, k * g1 + (b + gx * u) * g0]
    e = [rel(x, y) for x, y in zip(gbar, a["gbar"])]
    print(name, "channel adjoints against autograd:", e)
    assert max(e) < 1e-13                   # a handful of products and sums per point in fp64
    if "pad" in nr.CASES[name]:             # a zero-weight padding point receives exactly 0
        ne = p["ee"] - p["eb"]
        for v in a["gbar"]:
            v = v.reshape(ne, 21, 21)
            assert np.all(v[:, 20, :] == 0.0) and np.all(v[:, :, 20] == 0.0)


@pytest.mark.parametrize("lam", [1.0, 2.0, 3.0])
def test_bratu_closed_form(lam):
    """u'' + lam e^u = 0 by a second difference on a fine grid.  Bound: the difference's truncation h^2 / 12 max|u''''| with
    |u''''| = lam e^u |u'^2 - lam e^u| <= lam e^u (u'^2 + lam e^u) from the ODE itself and u' = -th tanh((x - 1/2) th / 2), plus rounding: u = -2 ln(ratio of two cosh near 1)
    carries an ABSOLUTE error of about 4 eps (two cosh, a division, the logarithm), and the difference weighs values by 1, 2, 1: 16 eps / h^2."""
    from hp_vpinns_amd.drivers.nonlinear import bratu_exact, bratu_theta
    th = bratu_theta(lam)
    assert abs(th - np.sqrt(2 * lam) * np.cosh(th / 4)) < 1e-14 * th
    assert th < 4.0 * np.arcsinh(4.0 / np.sqrt(2 * lam))           # the lower of the two roots
    h = 1e-3
    x = np.linspace(0.0, 1.0, 1001)
    u = bratu_exact(x, lam)
    assert abs(u[0]) < 1e-15 and abs(u[-1]) < 1e-15 and np.all(u[1:-1] > 0)
    up = -th * np.tanh((x - 0.5) * th / 2)
    m4 = np.max(lam * np.exp(u) * (up ** 2 + lam * np.exp(u)))
    bound = h * h / 12 * m4 + 16 * np.finfo(float).eps / (h * h)
    res = (u[2:] - 2 * u[1:-1] + u[:-2]) / (h * h) + lam * np.exp(u[1:-1])
    print("Bratu lam = %g: th = %.12f, max u = %.6f, ODE residual %.2e (bound %.2e)" % (lam, th, u.max(), np.abs(res).max(), bound))
    assert np.abs(res).max() < bound


def test_coef_field_on_advection():
    from hp_vpinns_amd.vpinn import _coef_field
    P = np.random.default_rng(3).uniform(-1, 1, (7, 2))
    assert np.array_equal(_coef_field(0.0, P, 2, "advection", True), np.zeros((7, 2)))
    assert np.array_equal(_coef_field(np.array([1.0, 0.0]), P, 2, "advection", True), np.repeat([[1.0, 0.0]], 7, 0))
    assert np.array_equal(_coef_field(lambda X: np.stack([X[:, 1], -X[:, 0]], 1), P, 2, "advection", True), np.stack([P[:, 1], -P[:, 0]], 1))
    assert np.array_equal(_coef_field(lambda X: X[:, 0], P, 2, "advection", True), np.repeat(P[:, :1], 2, 1))      # one field for both directions
    assert _coef_field(2.5, P[:, :1], 1, "advection", True).shape == (7, 1)
    for bad in (np.ones(3), lambda X: np.ones((7, 3))):
        with pytest.raises(ValueError):
            _coef_field(bad, P, 2, "advection", True)


@pytest.mark.parametrize("problem", ["bratu", "burgers", "allen-cahn"])
def test_driver_setup_builds_without_a_gpu(problem):
    """setup() is host-only; its f is the manufactured solution's: checked by second differences of the exact solution (h = 1e-3,
    truncation h^2 / 12 |u''''|: 1e-6 pi^4 / 12 ~ 1e-5 for Burgers' sine, eps^2 1e-6 / 12 * 16 / (2 eps)^4 ~ 2e-6 for the front; bound 1e-4)"""
    from hp_vpinns_amd.drivers import nonlinear as drv
    s = drv.setup(problem, n_quad=6, n_test=3, width=8, depth=2)
    mk = s["model"]
    dim = s["layers"][0]
    assert s["X_test"].shape[1] == dim and s["u_test"].shape[0] == s["X_test"].shape[0]
    assert np.asarray(mk["X_u_train"]).shape == (np.asarray(mk["u_train"]).size, dim)
    if problem == "bratu":
        assert mk["exponential"] == 1.0 and mk["kappa"] == 1.0 and mk["f"] == 0.0
        return
    exact = drv._burgers_exact if problem == "burgers" else (lambda P: drv._allen_cahn_exact(P, 0.2))
    P = np.random.default_rng(1).uniform([-0.9, 0.1], [0.9, 0.9], (50, 2))
    h = 1e-3
    ex, ey = np.array([h, 0.0]), np.array([0.0, h])
    u = exact(P)
    ux, uy = (exact(P + ex) - exact(P - ex)) / (2 * h), (exact(P + ey) - exact(P - ey)) / (2 * h)
    uxx, uyy = (exact(P + ex) - 2 * u + exact(P - ex)) / h ** 2, (exact(P + ey) - 2 * u + exact(P - ey)) / h ** 2
    if problem == "burgers":
        assert np.array_equal(mk["advection"], [1.0, 0.0]) and np.array_equal(mk["beta"], [0.0, 1.0]) and np.array_equal(mk["kappa"], [-0.05, 0.0])
        f = uy + u * ux - 0.05 * uxx
    else:
        assert mk["cubic"] == -1.0 and mk["sigma"] == 1.0 and mk["kappa"] == pytest.approx(0.04)
        f = 0.04 * (uxx + uyy) + u - u ** 3
    fd = mk["f"](P) if callable(mk["f"]) else mk["f"]             # (Allen-Cahn's front is exact: f = 0)
    assert np.abs(fd - f).max() < 1e-4
