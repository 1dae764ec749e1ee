"""tests/dualdense_reference.py and quadrature.gram_factors on the CPU, before any device number is looked at: the product's factors
against the dense solve and against the table route of the separable case, rotation invariance, the layout of W_e, conditioning, the
two derivations of the loss and gradient and central differences, and the refusals of the Python surface."""
import numpy as np
import pytest

import dualdense_reference as dd
import dualnorm_reference as dn
import generic_point as gp
import linop_sweep as ls
import mapped_reference as mr

CASES = {c["name"]: c for c in dd.cases()}


def _masked_R(p, seed):
    nax, nay = dd._counts(p)
    R = np.random.default_rng(seed).standard_normal((p["ee"] - p["eb"], p["nty"], p["ntx"]))
    for e in range(R.shape[0]):
        R[e, nay[e]:, :] = 0.0
        R[e, :, nax[e]:] = 0.0
    return R


def test_physical_on_boxes_is_the_table_route():
    """boxes of aspect ratio up to 24 with per-element counts, the dense route forced: W_e on random R against the eigen tables and
    against dualnorm_reference's dense solve, loss_e and Rbar"""
    p = dd.problem(CASES["aspect-lin"])
    R = _masked_R(p, 5)
    le, rb = dd.factor_route(dd.box_factors(p), R)
    for name, (lo, ro) in (("tables", dn.table_route(p, R)), ("dense", dn.dense_route(p, R))):
        e = (float(np.max(np.abs(le - lo) / np.abs(lo))), float(np.linalg.norm(rb - ro) / np.linalg.norm(ro)))
        print(name, e)
        assert max(e) < ls.AGREE, (name, e)


def _mesh_factors(mesh, mass=0.0):
    from hp_vpinns_amd.quadrature import gram_factors, gram_rule
    ntx, nty = int(mesh.nax.max()), int(mesh.nay.max())
    x = gram_rule(ntx, nty)[0]
    A = mesh.geometry(x, x)[1].reshape(len(mesh), x.size ** 2, 2, 2)
    return gram_factors(2, ntx, nty, mesh.nax, mesh.nay, A, None, mass)


def test_rotation_invariance_and_the_identity_map():
    from hp_vpinns_amd.adapt import MappedMesh
    box = (-0.3, 0.5, 0.1, 0.4)
    Jx, Jy = 0.4, 0.15
    for mass in (0.0, 3.0):
        Ginv = np.linalg.inv(dn.gram_element(2, 4, 3, Jx, Jy, mass))
        W = _mesh_factors(MappedMesh.from_quads(dd.rotated_rectangle(box, 0.3)[None], 4, 3), mass)[0]
        e = float(np.abs(W.T @ W - Ginv).max() / np.abs(Ginv).max())
        print("rotated by 0.3 rad, mass %g: %.2e" % (mass, e))
        assert e < ls.AGREE
        ident = MappedMesh(np.array([box]), 4, 3, map=lambda P: (P.copy(), np.tile(np.eye(2), (P.shape[0], 1, 1))))
        Wi = _mesh_factors(ident, mass)[0]
        e = float(np.abs(Wi.T @ Wi - Ginv).max() / np.abs(Ginv).max())
        assert e < ls.AGREE, e


@pytest.mark.parametrize("name", list(CASES))
def test_conditions_of_the_box_cases(name):
    """conditioning, layout of W_e, factors against the dense solve on the reference's R, the two derivations, central differences"""
    c = CASES[name]
    p = dd.problem(c)
    Gs = dd.grams(p, dd.S_of(p))
    cond = max(float(np.linalg.cond(G)) for G in Gs)
    assert cond < dn.COND_D, cond
    W = dd.box_factors(p)
    nax, nay = dd._counts(p)
    for e in range(W.shape[0]):
        assert np.all(np.triu(W[e], 1) == 0.0)
        act = ((np.arange(p["nty"])[:, None] < nay[e]) & (np.arange(p["ntx"])[None, :] < nax[e])).reshape(-1)
        assert np.all(W[e][~act, :] == 0.0) and np.all(W[e][:, ~act] == 0.0) and np.all(np.diag(W[e])[act] > 0.0)
    ref = dd.reference(p)
    (la, ra), (lb, rb) = dd.loss_e(Gs, p, ref[2]), dd.factor_route(W, ref[2])
    routes = (float(np.max(np.abs(la - lb) / np.abs(la))), float(np.linalg.norm(ra - rb) / np.linalg.norm(ra)))
    assert max(routes) < ls.AGREE, routes
    assert abs(la.sum() - ref[0][2]) < ls.AGREE * abs(ref[0][2])
    l3b, gb = dd.reference_autograd(p)
    agree = (dn._rel0(np.asarray(ref[0]), np.asarray(l3b)), float(gp.block_rel(ref[1], gb, p["layers"], p["c0"].size)))
    assert max(agree) < ls.AGREE, agree
    rng = np.random.default_rng(c["seed"] + 41)
    fd = []
    for _ in range(dn.N_FD):
        v = rng.standard_normal(p["full"].size)
        v /= np.linalg.norm(v)
        lp, lm = dd.reference(p, p["full"] + dn.FD_H * v)[0][0], dd.reference(p, p["full"] - dn.FD_H * v)[0][0]
        fd.append(abs((lp - lm) / (2 * dn.FD_H) - ref[1] @ v) / np.linalg.norm(ref[1]))
    print("%s | cond %.1e | routes %s | derivations %s | fd %.2e" % (name, cond, routes, agree, max(fd)))
    assert max(fd) < dn.FD_TOL, fd


def test_quadrilaterals_factors_against_the_dense_solve():
    """the product's route on three non-parallelogram quadrilaterals with counts (MappedMesh.geometry, gram_factors) against the
    loops of the reference"""
    from hp_vpinns_amd.adapt import MappedMesh
    from test_mapped_host import COUNTS, QUADS
    mesh = MappedMesh.from_quads(QUADS, *COUNTS)
    for mass in (0.0, 0.5):
        W = _mesh_factors(mesh, mass)
        p = dict(dim=2, ntx=4, nty=3, nax=np.array(COUNTS[0]), nay=np.array(COUNTS[1]), eb=0, ee=3, mass=mass, boxes=None)
        Gs = dd.grams(p, None, dd.quad_geom(QUADS))
        assert max(float(np.linalg.cond(G)) for G in Gs) < dn.COND_D
        R = _masked_R(p, 9)
        (la, ra), (lb, rb) = dd.loss_e(Gs, p, R), dd.factor_route(W, R)
        e = (float(np.max(np.abs(la - lb) / np.abs(la))), float(np.linalg.norm(ra - rb) / np.linalg.norm(ra)))
        print("quads, mass %g: %s" % (mass, e))
        assert max(e) < ls.AGREE


def test_gram_factors_refuses_by_element():
    from hp_vpinns_amd.quadrature import gram_factors, gram_rule
    ng = gram_rule(2, 2)[0].size
    A = np.tile(np.eye(2), (2, ng * ng, 1, 1))
    S = np.tile(np.eye(2), (2, ng * ng, 1, 1))
    S[1, 3] = [[1.0, 2.0], [2.0, 1.0]]                   # eigenvalues 3, -1
    with pytest.raises(ValueError, match="element 6"):
        gram_factors(2, 2, 2, 2, 2, A, S, first=5)
    with pytest.raises(ValueError, match="element 0.*Cholesky"):      # one Gauss point cannot carry four functions
        gram_factors(2, 2, 2, 2, 2, np.tile(np.eye(2), (1, 1, 1, 1)), None, gram_points=1)


def test_the_python_surface_refuses_with_reasons():
    """checked before a handle exists: _check_residual_norm and _check_scope need no device"""
    from hp_vpinns_amd.adapt import ElementMesh, MappedMesh
    from hp_vpinns_amd.vpinn import VPINNLinear
    chk = VPINNLinear._check_residual_norm
    chk = VPINNLinear._norm4
    assert chk("dual") == ("dual", 0.0, "reference", None) and chk(dict(kind="dual", mass=2.0)) == ("dual", 2.0, "reference", None)
    assert chk(dict(kind="dual", metric="energy", gram_points=9)) == ("dual", 0.0, "energy", 9)
    with pytest.raises(ValueError, match="metric"):
        chk(dict(kind="l2", metric="physical"))
    with pytest.raises(ValueError, match="metric"):
        chk(dict(kind="dual", metric="euclid"))

    class Stub:                                          # what _check_scope reads of a model
        _strong_form = None
        _residual_norm = chk("l2")
        _trainable = ()
    mapped = MappedMesh.from_quads(dd.rotated_rectangle((-1.0, 1.0, -1.0, 1.0), 0.3)[None], 2, 2)
    with pytest.raises(ValueError, match='metric="physical"'):      # plain "dual" on a MappedMesh still raises, and says what does work
        VPINNLinear._check_scope(Stub(), mapped, chk("dual"))
    VPINNLinear._check_scope(Stub(), mapped, chk(dict(kind="dual", metric="physical")))
    s = Stub()
    s._trainable = (dict(name="k", init=1.0, kappa=1.0),)
    with pytest.raises(ValueError, match="trainable kappa"):
        VPINNLinear._check_scope(s, ElementMesh(np.array([[-1.0, 1.0, -1.0, 1.0]]), 2, 2), chk(dict(kind="dual", metric="energy")))


# ---- the estimator identity: a polynomial in the network's place ---------------------------------------------------------------------
def _K_poly(P):
    """a 2 x 2 SPD field, linear in the point: eigenvalues above 1 on [-1, 1]^2"""
    x, y = P[:, 0], P[:, 1]
    return np.stack([np.stack([2.0 + 0.3 * x, 0.2 * y], 1), np.stack([0.2 * y, 1.5 + 0.2 * y], 1)], 1)


def _estimator(geom, S, seed, q=8, nt=4, deg=2, n_gauss=12):
    """(loss of the dense dual norm, |P_h(pt - u)|^2 in the S-weighted seminorm computed independently) on ONE element: F is the
    projection of div(S grad u) (by parts: -(S grad u, grad v), the reference's own weak form of u), the channels are pt's"""
    import torch
    import linear_reference as lr
    from hp_vpinns_amd.testfcn import Test_fcn, dTest_fcn
    rng = np.random.default_rng(seed)
    cu, cp = rng.standard_normal((deg + 1, deg + 1)), rng.standard_normal((deg + 1, deg + 1))
    rx = lr.rule(q)
    X, A = geom(rx[0], rx[0])
    Sq = np.tile(np.eye(2), (1, q * q, 1, 1)) if S is None else S(X.reshape(-1, 2)).reshape(1, q * q, 2, 2)
    coefs = dict(K=Sq, b=np.zeros((1, q * q, 2)), s=np.zeros((1, q * q)))
    p = mr.problem([2, 4, 1], seed, X, A, rx, rx, (nt, nt), coefs, mass=0.0, boxes=np.zeros((1, 4)))

    def fn(c):
        def u_fn(Xt):
            v, g, _ = dn._poly(c, Xt.numpy())
            return torch.tensor(v), torch.tensor(g)
        return u_fn
    Gs = dd.grams(p, S, geom)
    p["F"] = np.zeros_like(p["F"])
    with dd._dense(Gs, p):
        p["F"] = mr.terms(dict(p, u_fn=fn(cu)))["R"]              # -(S grad u, grad v): what the projection of f = div(S grad u) is
        loss = mr.terms(dict(p, u_fn=fn(cp)))["lossv"]
    # independently: b = (S grad(pt - u), grad v) by Gauss-Legendre in physical terms, b^T G^-1 b
    x, w = np.polynomial.legendre.leggauss(n_gauss)
    Xg, Ag = geom(x, x)
    Xg, Ag = Xg[0], Ag[0]
    ge = dn._poly(cp, Xg)[1] - dn._poly(cu, Xg)[1]
    Sg = np.tile(np.eye(2), (Xg.shape[0], 1, 1)) if S is None else S(Xg)
    phi, dphi = Test_fcn(nt, x), dTest_fcn(nt, x)[0]
    b = np.zeros(nt * nt)
    for j in range(n_gauss):
        for i in range(n_gauss):
            g = j * n_gauss + i
            a = Ag[g]
            det = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
            gref = np.array([[dphi[r, i] * phi[k, j], phi[r, i] * dphi[k, j]] for k in range(nt) for r in range(nt)])
            b += w[j] * w[i] * det * (gref @ np.linalg.inv(a)) @ (0.5 * (Sg[g] + Sg[g].T) @ ge[g])
    return loss, float(b @ np.linalg.solve(Gs[0], b))


ESTIMATOR_CASES = {
    "sheared quadrilateral, physical": (lambda xi, yi: mr.geom_quads(np.array([[[-0.8, -0.5], [0.6, -0.3], [0.9, 0.4], [-0.5, 0.2]]]), xi, yi), None, 7401),
    "box, energy with a 2 x 2 SPD K(x)": (lambda xi, yi: mr.geom_boxes(np.array([[-0.7, 0.4, -0.2, 0.5]]), xi, yi), _K_poly, 7402),
}


@pytest.mark.parametrize("name", list(ESTIMATOR_CASES))
def test_estimator_identity(name):
    """loss_e equals the squared energy norm of the Galerkin projection of the error onto the element's bubble space"""
    geom, S, seed = ESTIMATOR_CASES[name]
    loss, proj = _estimator(geom, S, seed)
    e = abs(loss - proj) / proj
    print("%s: loss %.12e, projected error %.12e, relative difference %.2e" % (name, loss, proj, e))
    assert proj > 1e-3 and e < dd.ESTIMATOR_TOL, (loss, proj, e)
