"""tests/quasilinear_reference.py proved on the CPU (no GPU): its gradient against central differences and its channel adjoints against
the formulas of csrc/kernels_nonlin.hip, mu == 1 against nonlinear_reference, the three driver problems' exact solutions against the
weak and the strong residual, the driver's f against central differences of the flux, and the plane assembly of the class."""
import numpy as np
import pytest

import linear_reference as lr
import mapped_reference as mr
import nonlinear_reference as nr
import quasilinear_reference as qr

L2 = [2, 8, 8, 1]
QUADS = np.array([[[-1.0, -1.0], [-0.1, -0.9], [-0.25, 0.05], [-0.9, -0.2]],
                  [[-0.1, -0.9], [1.0, -1.0], [0.8, -0.15], [-0.25, 0.05]]])
BOXES = np.array([[-1.0, 0.3, -1.0, -0.2], [0.3, 1.0, -1.0, -0.2]])


def _case(kind, r=-0.5, terms=("u3", "adv"), seed=9650):
    rng = np.random.default_rng(seed)
    if kind == "1d":
        rx = lr.rule(5)
        b = np.array([[0.0, 0.3], [0.3, 1.0]])
        X, A = qr.geom_1d(b, rx[0])
        coefs = dict(K=mr._signed(rng, (2, 5, 1, 1)), b=mr._signed(rng, (2, 5, 1)), s=mr._signed(rng, (2, 5)), a3=mr._signed(rng, (2, 5)))
        return qr.problem(1, [1, 8, 8, 1], seed, X, A, (rx, None), 3, coefs, qr.quasi_planes(rng, 2, 5, True, True, r), counts=[3, 2], boxes=b)
    rx, ry = lr.rule(5), lr.rule(4)
    X, A = mr.geom_quads(QUADS, rx[0], ry[0]) if kind == "quads" else mr.geom_boxes(BOXES, rx[0], ry[0])
    coefs = mr.random_coefs(rng, 2, 20, terms, diagonal=kind != "quads")
    return qr.problem(2, L2, seed, X, A, (rx, ry), (3, 2), coefs, qr.quasi_planes(rng, 2, 20, True, True, r), counts=([3, 2], [1, 2]), data=5,
                      boxes=None if kind == "quads" else BOXES)


@pytest.mark.parametrize("kind", ["1d", "boxes", "quads"])
def test_gradient_against_central_differences(kind):
    """autograd of the reference's own loss IS its gradient; central differences along three random directions confirm it"""
    p = _case(kind)
    l3, g, _ = qr.reference(p)
    rng = np.random.default_rng(5)
    h = float(np.finfo(np.float64).eps ** (1.0 / 3.0))
    for _ in range(3):
        v = rng.standard_normal(g.size)
        v /= np.linalg.norm(v)
        fd = (qr.reference(p, p["theta"] + h * v)[0][0] - qr.reference(p, p["theta"] - h * v)[0][0]) / (2 * h)
        assert abs(fd - g @ v) < 1e-7 * max(1.0, abs(g @ v)), (kind, fd, g @ v)


@pytest.mark.parametrize("kind,r", [("boxes", -0.5), ("boxes", 0.5), ("quads", -0.5), ("1d", 0.5)])
def test_channel_adjoints_are_the_kernels_formulas(kind, r):
    """GBAR by autograd: against a directional derivative of lossv with respect to the channels, and against the chain rule the kernel
    applies -- GBAR minus the adjoints of the problem with mu frozen into K is (mu_u h, 2 grad u mu_s h) with one and the same h"""
    p = _case(kind, r)
    adj = qr.channel_adjoints(p)
    rng = np.random.default_rng(6)
    du_, ddu_ = rng.standard_normal(adj["u"].shape), rng.standard_normal(adj["du"].shape)
    h = 1e-6
    import torch

    def lossv(t):
        return float(qr._loss(p, torch.tensor(adj["u"] + t * du_), torch.tensor(adj["du"] + t * ddu_))["lossv"])
    fd = (lossv(h) - lossv(-h)) / (2 * h)
    an = float(np.sum(adj["gbar_u"] * du_) + np.sum(adj["gbar_du"] * ddu_))
    assert abs(fd - an) < 1e-6 * max(1.0, abs(an)), (fd, an)
    q = p["q"]
    u, du = adj["u"], adj["du"]
    s = np.sum(du * du, axis=2)
    P, dP = q["m"][..., 0] + q["m"][..., 1] * u + q["m"][..., 2] * u * u, q["m"][..., 1] + 2 * q["m"][..., 2] * u
    B = (q["delta"] + s) ** q["r"]
    mu, mu_u, mu_s = P * B, dP * B, q["r"] * P * B / (q["delta"] + s)
    assert np.allclose(qr.mu_of(q, torch.tensor(u), torch.tensor(s)).numpy(), mu, rtol=1e-14)
    # freeze mu: the problem with K' = mu K and no multiplier has the adjoints mu K^T g; the difference is mu_u h, 2 u_x mu_s h
    frozen = dict(p, coefs=dict(p["coefs"], K=mu[..., None, None] * p["coefs"]["K"]), q=dict(q, use_u=False, use_grad=False))
    fa = qr.channel_adjoints(frozen, (u, du))
    extra_u = adj["gbar_u"] - fa["gbar_u"]                                           # = mu_u h
    extra_d = adj["gbar_du"] - fa["gbar_du"]                                         # = 2 grad u mu_s h
    hq = np.where(np.abs(mu_u) > 1e-3, extra_u / np.where(mu_u == 0, 1, mu_u), np.nan)
    ok = ~np.isnan(hq)
    assert ok.sum() > ok.size // 2                                                  # (h recovered from GBAR[u] wherever mu_u is not tiny ...)
    assert np.allclose(extra_d[ok], (2.0 * du * (mu_s * np.nan_to_num(hq))[..., None])[ok], rtol=1e-8, atol=1e-11)      # (... gives GBAR[grad u]'s extra term)


@pytest.mark.parametrize("name", ["2d-h8", "2d-h8-counts-flux", "1d-sin"])
def test_mu_one_reproduces_the_nonlinear_reference(name):
    """the same problem stated in this module's physical terms, mu switched off: R, lossv and the gradient of nonlinear_reference"""
    p0 = nr.problem(dict(nr.CASES[name], data=0, flux=0))
    v0 = nr.var_part(p0)
    dim, b = p0["dim"], p0["boxes"]
    ne = b.shape[0]
    if dim == 2:
        X, A = mr.geom_boxes(b, p0["xr"][0], p0["yr"][0])
        kx, ky, bx, by, s = (r.reshape(ne, -1) for r in p0["planes"])
        K = np.zeros(kx.shape + (2, 2))
        K[..., 0, 0], K[..., 1, 1] = kx, ky
        coefs = dict(K=K, b=np.stack([bx, by], -1), s=s, g=np.stack([p0["nl"][3].reshape(ne, -1), p0["nl"][4].reshape(ne, -1)], -1))
    else:
        X, A = qr.geom_1d(b, p0["xr"][0])
        k, bb, s = (r.reshape(ne, -1) for r in p0["planes"])
        coefs = dict(K=k[..., None, None], b=bb[..., None], s=s, g=p0["nl"][3].reshape(ne, -1)[..., None])
    coefs.update(a2=p0["nl"][0].reshape(ne, -1), a3=p0["nl"][1].reshape(ne, -1), ae=p0["nl"][2].reshape(ne, -1))
    nq = X.shape[1]
    q = qr.quasi_planes(np.random.default_rng(1), ne, nq, False, False)
    counts = None if p0["nax"] is None else ((p0["nax"], p0["nay"]) if dim == 2 else p0["nax"])
    p = qr.problem(dim, p0["layers"], 1, X, A, (p0["xr"], p0["yr"]), (p0["ntx"], p0["nty"]) if dim == 2 else p0["ntx"], coefs, q, counts=counts, boxes=b)
    p["theta"], p["F"] = p0["theta"], p0["F"]
    t = qr.terms(p)
    assert np.allclose(t["R"], v0["R"], rtol=1e-12, atol=1e-14) and abs(t["lossv"] - v0["lossv"]) < 1e-12 * abs(v0["lossv"])
    assert np.linalg.norm(t["grad"] - v0["grad"]) < 1e-12 * np.linalg.norm(v0["grad"])


def _exact_problem(name, q_pts, quads=False):
    """the driver problem `name` on two elements with a q_pts-point rule, its exact solution in the network's place"""
    from hp_vpinns_amd.drivers import nonlinear as drv
    dif = drv.quasi_diffusivity(name, p=3.0, eps=1.0)
    exact = drv.scherk if name == "minimal-surface" else drv.manufactured
    rx = ry = lr.rule(q_pts)
    X, A = mr.geom_quads(QUADS, rx[0], ry[0]) if quads else mr.geom_boxes(BOXES, rx[0], ry[0])
    ne, nq = X.shape[:2]
    K = np.zeros((ne, nq, 2, 2))
    K[..., 0, 0] = K[..., 1, 1] = 1.0
    m = np.zeros((ne, nq, 3))
    m[...] = np.asarray(dif["poly"])
    q = dict(m=m, delta=np.full((ne, nq), dif["shift"]), r=dif["power"], use_u=dif["poly"] != (1.0, 0.0, 0.0), use_grad=dif["power"] != 0.0)
    p = qr.problem(2, L2, 3, X, A, (rx, ry), (3, 3), dict(K=K), q, boxes=None if quads else BOXES)
    u, du, _ = exact(X.reshape(-1, 2))
    f = np.zeros(ne * nq) if name == "minimal-surface" else drv.quasi_rhs(dif, exact, X.reshape(-1, 2))
    return p, (u.reshape(ne, nq), du.reshape(ne, nq, 2)), f.reshape(ne, nq), dif, exact


@pytest.mark.parametrize("quads", [False, True], ids=["boxes", "quads"])
@pytest.mark.parametrize("name", ["heat-ku", "p-laplace", "minimal-surface"])
def test_exact_solutions_annihilate_the_residuals_at_spectral_rate(name, quads):
    """weak: R - (projection of f) -> 0; strong (divergence form): r -> 0, geometrically as the rule grows: each step of four points
    (6 -> 10 -> 14) gains at least a factor 10 -- an algebraic rate of order k would gain (14 / 10)^k on the second step, a factor 10
    only for k >= 6.8 -- or the error has reached rounding.  (The p-Laplacian's sqrt(eps^2 + |grad u|^2) has its branch points a
    distance ~eps off the real axis, so its geometric rate falls with eps; the case takes eps = 1 to keep them as far away as the
    singularities of the other two.)"""
    import torch
    from hp_vpinns_amd.testfcn import tables_1d
    weak, strong = [], []
    for n in (6, 10, 14):
        p, (u, du), f, _, _ = _exact_problem(name, n, quads)
        (xi, wx), (yi, wy) = p["xr"], p["yr"]
        det = np.linalg.det(p["A"])
        ax, by = tables_1d(3, xi)[0] * wx[None, :], tables_1d(3, yi)[0] * wy[None, :]
        p["F"] = np.einsum("kj,ri,eji->ekr", by, ax, (det * f).reshape(-1, n, n))
        R = qr._loss(p, torch.tensor(u), torch.tensor(du))["R"].numpy()
        weak.append(float(np.abs(R).max()))
        strong.append(float(np.abs(qr.strong(p, f, u_du=(u, du))).max()))
    print(name, "quads" if quads else "boxes", "weak", weak, "strong", strong)
    assert weak[1] < 0.1 * weak[0] and (weak[2] < 0.1 * weak[1] or weak[2] < 1e-12)
    assert strong[1] < 0.1 * strong[0] and (strong[2] < 0.1 * strong[1] or strong[2] < 1e-10)


@pytest.mark.parametrize("name", ["heat-ku", "p-laplace", "minimal-surface"])
def test_driver_rhs_against_central_differences(name):
    """f of the driver = div(mu grad u), the divergence by central differences of the flux (the flux itself from the exact gradient)"""
    from hp_vpinns_amd.drivers import nonlinear as drv
    s = drv.setup(name, p=3.0, eps=0.3)
    dif, exact = s["model"]["diffusivity"], s["exact"]
    P = np.random.default_rng(4).uniform(-0.9, 0.9, (40, 2))

    def flux(X):
        u, du, _ = exact(X)
        return drv.quasi_mu(dif["poly"], dif["shift"], dif["power"], u, np.sum(du * du, axis=1))[0][:, None] * du
    h = 1e-5
    div = sum((flux(P + h * e)[:, a] - flux(P - h * e)[:, a]) / (2 * h) for a, e in enumerate(np.eye(2)))
    f = s["model"]["f"]
    fv = f(P) if callable(f) else np.full(P.shape[0], f)
    assert np.abs(div - fv).max() < 1e-7 * max(1.0, np.abs(div).max())
    # ... and the reference's divergence-form residual of the exact solution against the same f is covered by the test above


def test_plane_assembly_is_not_scaled_by_det_a():
    """the class hands m0, m1, m2, delta at the PHYSICAL points of a MappedMesh as plain rows (mu multiplies K_eff, which carries the
    geometry), while the pointwise terms next to them are times det A"""
    from hp_vpinns_amd.adapt import MappedMesh
    from hp_vpinns_amd.vpinn import VPINNNonlinear
    mesh = MappedMesh.from_quads(QUADS, [3, 2], [2, 2])
    m = object.__new__(VPINNNonlinear)
    m._rule = (lr.rule(5), lr.rule(4))
    m._dev_rule = (m._rule[0][0], m._rule[1][0])
    m._diffusivity = VPINNNonlinear._check_diffusivity(dict(poly=(lambda P: 1.0 + P[:, 0] ** 2, 0.5, lambda P: P[:, 1]), shift=lambda P: 2.0 + P[:, 0] * P[:, 1],
                                                            power=-0.5), None, "divergence")
    rows = m._quasi_planes(mesh, 0, 2)
    P, A = mesh.geometry(m._dev_rule[0], m._dev_rule[1], 0, 2)
    want = np.stack([1.0 + P[:, 0] ** 2, np.full(P.shape[0], 0.5), P[:, 1], 2.0 + P[:, 0] * P[:, 1]], 0)
    assert rows.shape == (4, 40) and np.array_equal(rows, want)
    det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    assert np.abs(det - 1.0).min() > 1e-3                                           # (a det-scaled row would differ)
    X, _ = mr.geom_quads(QUADS, m._dev_rule[0], m._dev_rule[1])
    assert np.allclose(P, X.reshape(-1, 2), rtol=0, atol=1e-14)
    for bad, msg in ((dict(shift=lambda P: P[:, 0], power=0.5), "shift"), (dict(poly=(1.0, 0.0)), "poly"), (dict(power=np.inf), "power"), (dict(exp=1.0), "diffusivity is")):
        with pytest.raises(ValueError, match=msg):
            m._diffusivity = VPINNNonlinear._check_diffusivity(bad, None, None)
            m._quasi_planes(mesh, 0, 2)
    with pytest.raises(ValueError, match="trainable"):
        VPINNNonlinear._check_diffusivity({}, [dict(name="c", init=1.0)], None)
    with pytest.raises(ValueError, match="elementwise"):
        VPINNNonlinear._check_diffusivity({}, None, "elementwise")
