"""Textbook problems of the variable-coefficient linear class (VPINNLinear), each with a manufactured solution; prints the
relative L2 error.

  boundary layer   -eps u'' + u' = 1 on [0, 1], u(0) = u(1) = 0:  u = x - (exp((x - 1) / eps) - exp(-1 / eps)) / (1 - exp(-1 / eps)),
                   a layer of width eps at x = 1; the elements are graded towards it.  In the class's convention
                   (k u')' + b u' + s u = f this is k = -eps, b = 1, s = 0, f = 1.
  L-shape          div(kappa grad u) + beta . grad u + sigma u = f on [-1, 1]^2 without its lower right quadrant, as three boxes;
                   kappa = 1 + x y, beta = (1, -1), sigma = 2, u = sin(pi x) sin(pi y) (zero on the whole boundary), f manufactured.

  annulus          lap u = f on the quarter annulus 1 < r < 2, 0 < theta < pi / 2: mapped elements (adapt.MappedMesh, polar map of boxes
                   in the (r, theta) plane); u = (r - 1)(2 - r) sin(2 theta), zero on all four sides, f manufactured.
  anisotropic      div(K grad u) = f on [-1, 1]^2 with K = Q diag(1, --ratio) Q^T, Q the rotation by --angle degrees: a full tensor
                   (hpv_set_operator_tensor); u = sin(pi x) sin(pi y), f manufactured.

  neumann          lap u = f on the unit square with du/dn = g on all four sides (set_flux_data) and no Dirichlet data: the solution is
                   fixed only up to a constant, which the integral constraint int u = c (constraints=[dict(kind="mean", ..)]) picks;
                   u = cos(pi x) cos(pi y) + 0.3 x^2 - 0.2 y + 0.5 (mean 0.5), f and g manufactured.  --no-mean leaves the constraint out.

    python -m hp_vpinns_amd.drivers.linear boundary-layer --eps 0.05
    python -m hp_vpinns_amd.drivers.linear neumann
    python -m hp_vpinns_amd.drivers.linear l-shape
    python -m hp_vpinns_amd.drivers.linear annulus --hard-bc
    python -m hp_vpinns_amd.drivers.linear anisotropic --angle 30
    python -m hp_vpinns_amd.drivers.linear boundary-layer --eps 0.05 --adapt-every 500 --max-elements 16

    python -m hp_vpinns_amd.drivers.linear boundary-layer --eps 0.05 --hard-bc

--hard-bc (boundary layer, annulus): the Dirichlet conditions are built into the trial function, u = G + D N with D = (x - a)(b - x) and G the
linear interpolant of the end values (VPINNLinear(hard_bc=...)): no boundary points, no penalty weight.

--adapt-every K: local hp-refinement (VPINNLinear(strong_form=...).train_adaptive) after every K-th update, at most
--max-elements elements; one (iteration, elements, loss) row is printed per round.  boundary-layer and l-shape take the strong
residual elementwise ("elementwise"); the annulus (mapped elements), anisotropic (a full tensor) and boundary-layer --hard-bc (an
ansatz) take it in divergence form ("divergence"), which needs no second derivatives.

    python -m hp_vpinns_amd.drivers.linear annulus --adapt-every 500 --max-elements 40
    python -m hp_vpinns_amd.drivers.linear boundary-layer --eps 0.05 --hard-bc --adapt-every 500 --max-elements 16
"""
import argparse

import numpy as np

from ..adapt import ElementMesh, MappedMesh
from ..vpinn import VPINNLinear

# the smallest setting of the boundary-layer run (tests/test_gpu_linear.py trains it once)
SMALLEST = dict(eps=0.2, n_elements=3, n_quad=8, n_test=4, n_iter=600, layers=[1, 8, 8, 1], LR=5e-3)


def boundary_layer_exact(x, eps):
    x = np.asarray(x, dtype=np.float64)
    return x - (np.exp((x - 1.0) / eps) - np.exp(-1.0 / eps)) / (1.0 - np.exp(-1.0 / eps))


def graded_grid(n, grade=2.0):
    """n elements on [0, 1] with widths shrinking towards x = 1: x_i = 1 - (1 - i / n)^grade"""
    return 1.0 - (1.0 - np.arange(n + 1) / n) ** grade


def interval_hard_bc(a, b, ua, ub):
    """dict(g=, d=) for VPINNLinear(hard_bc=...) on [a, b]: D = (x - a)(b - x), G the linear interpolant of the end values ua, ub
    (written so that G(a) == ua and G(b) == ub to the last bit)"""
    a, b, ua, ub = float(a), float(b), float(ua), float(ub)

    def g(P):
        x = P[:, 0]
        return np.stack([ua * ((b - x) / (b - a)) + ub * ((x - a) / (b - a)), np.full(x.shape, (ub - ua) / (b - a))], 1)

    def d(P):
        x = P[:, 0]
        return np.stack([(x - a) * (b - x), (a + b) - 2.0 * x], 1)
    return dict(g=g, d=d)


def _norm_arg(residual_norm, gram_mass, mapped=False):
    """the residual_norm= of the classes from the command line's --residual-norm / --gram-mass: "dual" is the reference metric on
    boxes and the physical one on a mapped mesh (dense Gram factors), "energy" the inner product of the problem's own kappa"""
    if residual_norm == "l2":
        return "l2"
    if residual_norm == "energy":
        return dict(kind="dual", mass=float(gram_mass), metric="energy")
    return dict(kind="dual", mass=float(gram_mass), metric="physical") if mapped else dict(kind="dual", mass=float(gram_mass))


def _loss_line(m, err):
    """sqrt(lossv) beside the relative L2 error, for the drivers that know no H^1 error of their solution"""
    return "sqrt(lossv) %.4e beside the relative L2 error %.4e (residual norm %s)" % (np.sqrt(float(np.asarray(m.loss())[2])), err, m.residual_norm)


def _estimator_line(m, h1_err):
    """sqrt(lossv) beside the H^1-seminorm error the driver knows from its manufactured solution: under residual_norm="dual" the
    first estimates the second (exactly the projected error's energy for kappa = 1, beta = sigma = 0; up to the operator's
    continuity and inf-sup constants otherwise), under "l2" it does not"""
    lossv = float(np.asarray(m.loss())[2])
    return "sqrt(lossv) %.4e beside the H^1 error %.4e (residual norm %s)" % (np.sqrt(lossv), h1_err, m.residual_norm)


def _train(m, n_iter, adapt_every, max_elements, verbose, lbfgs=0, test=None):
    """train, or train_adaptive with its rows [(iterations done, elements, loss on the new mesh)] printed like the Poisson-2D driver's;
    then lbfgs iterations of the L-BFGS stage, the error on the points test = (X, u) printed before and after"""
    from . import lbfgs_stage
    if not adapt_every:
        m.train(int(n_iter), verbose=verbose)
        lbfgs_stage(m, lbfgs, (lambda: m.rel_l2_error(*test)) if test is not None else None, verbose=verbose)
        return []
    rows = m.train_adaptive(int(n_iter), int(adapt_every), max_elements=max_elements)
    if verbose:
        for it, ne, loss in rows:
            print("It: %d, adapted to %d elements, loss on the new mesh: %.3e" % (it, ne, loss))
    lbfgs_stage(m, lbfgs, (lambda: m.rel_l2_error(*test)) if test is not None else None, verbose=verbose)
    return rows


def run_boundary_layer(eps=0.05, n_elements=8, n_quad=20, n_test=10, n_iter=2000, layers=(1, 20, 20, 20, 1), grade=2.0, LR=1e-3,
                       lossb_weight=10.0, seed=1234, backend="auto", device=None, verbose=True, adapt_every=None, max_elements=None, hard_bc=False,
                       residual_norm="l2", lbfgs=0):
    grid = graded_grid(int(n_elements), grade)
    bc = dict(hard_bc=interval_hard_bc(0.0, 1.0, 0.0, 0.0)) if hard_bc else dict(X_u_train=np.array([[0.0], [1.0]]), u_train=np.zeros(2))
    m = VPINNLinear(list(layers), grid_x=grid, n_quad=int(n_quad), n_test=int(n_test), kappa=-float(eps), beta=1.0, sigma=0.0, f=1.0,
                    lossb_weight=lossb_weight, activation="sin", LR=LR,
                    seed=seed, backend=backend, device=device,
                    strong_form=("divergence" if hard_bc else "elementwise") if adapt_every else None,      # (the ansatz has no second derivatives)
                    residual_norm=residual_norm, **bc)
    X = np.linspace(0.0, 1.0, 401)[:, None]
    u = boundary_layer_exact(X, eps)
    rows = _train(m, n_iter, adapt_every, max_elements, verbose, lbfgs, (X, u))
    err = m.rel_l2_error(X, u)
    ux = 1.0 - np.exp((X[:, 0] - 1.0) / eps) / (eps * (1.0 - np.exp(-1.0 / eps)))
    d2 = (np.asarray(m.evaluate(X)["u_x"]).reshape(-1) - ux) ** 2
    h1 = float(np.sqrt(np.sum(0.5 * (d2[1:] + d2[:-1]) * np.diff(X[:, 0]))))      # (trapezoidal rule on the test points)
    bnd = float(np.max(np.abs(m.predict(np.array([[0.0], [1.0]])))))      # (both end values are 0)
    if verbose:
        print("boundary layer eps = %g, %d elements (%d graded at the start), %s: relative L2 error %.4e, boundary error %.3e (%s)"
              % (eps, len(m.mesh), n_elements, "exact conditions (ansatz)" if hard_bc else "penalty", err, bnd, m.h.kernel_variant()))
        print(_estimator_line(m, h1))
    return dict(model=m, rel_l2=err, bnd_err=bnd, h1_err=h1, X_test=X, u_test=u, loss_his=np.asarray(m.loss_his), adapt_rows=rows)


L_BOXES = np.array([[-1.0, 0.0, -1.0, 0.0], [-1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 1.0]])


def _l_exact(P):
    return np.sin(np.pi * P[:, 0]) * np.sin(np.pi * P[:, 1])


def _l_f(P):
    x, y = P[:, 0], P[:, 1]
    u = _l_exact(P)
    ux, uy = np.pi * np.cos(np.pi * x) * np.sin(np.pi * y), np.pi * np.sin(np.pi * x) * np.cos(np.pi * y)
    kappa = 1.0 + x * y
    return kappa * (-2.0 * np.pi ** 2 * u) + y * ux + x * uy + ux - uy + 2.0 * u


def _l_boundary(n):
    """n points per edge on the six edges of the L"""
    t = np.linspace(0.0, 1.0, n)
    c = [(-1, -1), (0, -1), (0, 0), (1, 0), (1, 1), (-1, 1), (-1, -1)]
    return np.concatenate([np.stack([a[0] + (b[0] - a[0]) * t, a[1] + (b[1] - a[1]) * t], 1) for a, b in zip(c[:-1], c[1:])])


def run_l_shape(n_iter=2000, n_quad=20, n_test=10, layers=(2, 20, 20, 20, 1), n_bound=40, LR=1e-3, lossb_weight=10.0, seed=1234,
                backend="auto", device=None, verbose=True, adapt_every=None, max_elements=None, residual_norm="l2", lbfgs=0):
    Xb = _l_boundary(int(n_bound))
    m = VPINNLinear(list(layers), mesh=ElementMesh(L_BOXES, int(n_test), int(n_test)), n_quad=int(n_quad),
                    kappa=lambda P: 1.0 + P[:, 0] * P[:, 1], beta=np.array([1.0, -1.0]), sigma=2.0, f=_l_f, X_u_train=Xb, u_train=_l_exact(Xb),
                    lossb_weight=lossb_weight, LR=LR, seed=seed, backend=backend, device=device,
                    strong_form="elementwise" if adapt_every else None, residual_norm=residual_norm)
    g = np.linspace(-1.0, 1.0, 81)
    X = np.stack([v.reshape(-1) for v in np.meshgrid(g, g)], 1)
    X = X[~((X[:, 0] > 0) & (X[:, 1] < 0))]
    u = _l_exact(X)[:, None]
    rows = _train(m, n_iter, adapt_every, max_elements, verbose, lbfgs, (X, u))
    err = m.rel_l2_error(X, u)
    ev = m.evaluate(X)
    gx = np.pi * np.cos(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]) - np.asarray(ev["u_x"]).reshape(-1)
    gy = np.pi * np.sin(np.pi * X[:, 0]) * np.cos(np.pi * X[:, 1]) - np.asarray(ev["u_y"]).reshape(-1)
    h1 = float(np.sqrt(3.0 * np.mean(gx ** 2 + gy ** 2)))      # (the L has area 3; a mean over the uniform test points)
    if verbose:
        print("L-shape, kappa = 1 + x y, beta = (1, -1), sigma = 2, %d elements: relative L2 error %.4e (%s)" % (len(m.mesh), err, m.h.kernel_variant()))
        print(_estimator_line(m, h1))
    return dict(model=m, rel_l2=err, h1_err=h1, X_test=X, u_test=u, loss_his=np.asarray(m.loss_his), adapt_rows=rows)


# the smallest setting of the annulus run (tests/test_gpu_mapped.py trains it once)
ANNULUS_SMALLEST = dict(n_r=2, n_theta=2, n_quad=8, n_test=4, n_iter=300, layers=[2, 8, 8, 1], LR=5e-3)


def polar_map(P):
    """(r, theta) -> (x, y) = r (cos theta, sin theta) with its Jacobian: the map= of adapt.MappedMesh"""
    r, t = P[:, 0], P[:, 1]
    return (np.stack([r * np.cos(t), r * np.sin(t)], 1),
            np.stack([np.stack([np.cos(t), -r * np.sin(t)], 1), np.stack([np.sin(t), r * np.cos(t)], 1)], 1))


def annulus_mesh(n_r, n_theta, n_test):
    """n_r x n_theta boxes of the (r, theta) plane on 1 < r < 2, 0 < theta < pi / 2 under the polar map"""
    g = ElementMesh.from_grid(np.linspace(1.0, 2.0, int(n_r) + 1), np.linspace(0.0, np.pi / 2, int(n_theta) + 1))
    return MappedMesh(g.boxes, int(n_test), int(n_test), map=polar_map)


def _annulus_exact(P):
    x, y = P[:, 0], P[:, 1]
    r = np.hypot(x, y)
    return (r - 1.0) * (2.0 - r) * 2.0 * x * y / r ** 2


def _annulus_f(P):
    """the Laplacian of g(r) sin(2 theta), g = (r - 1)(2 - r):  (g'' + g' / r - 4 g / r^2) sin(2 theta)"""
    x, y = P[:, 0], P[:, 1]
    r = np.hypot(x, y)
    return (-2.0 + (3.0 - 2.0 * r) / r - 4.0 * (r - 1.0) * (2.0 - r) / r ** 2) * 2.0 * x * y / r ** 2


def annulus_hard_bc():
    """dict(g=, d=): D = (r - 1)(2 - r) x y vanishes on the two arcs and the two straight sides, G = 0"""
    def d(P):
        x, y = P[:, 0], P[:, 1]
        r = np.hypot(x, y)
        g, dg = (r - 1.0) * (2.0 - r), 3.0 - 2.0 * r
        return np.stack([g * x * y, dg * (x / r) * x * y + g * y, dg * (y / r) * x * y + g * x], 1)
    return dict(g=0.0, d=d)


def _annulus_boundary(n):
    t, r = np.linspace(0.0, np.pi / 2, n), np.linspace(1.0, 2.0, n)
    z = np.zeros(n)
    return np.concatenate([np.stack([np.cos(t), np.sin(t)], 1), 2.0 * np.stack([np.cos(t), np.sin(t)], 1), np.stack([r, z], 1), np.stack([z, r], 1)])


def run_annulus(n_r=4, n_theta=4, n_quad=10, n_test=5, n_iter=2000, layers=(2, 20, 20, 20, 1), n_bound=40, LR=1e-3, lossb_weight=10.0,
                seed=1234, backend="auto", device=None, verbose=True, hard_bc=False, record_every=None, residual_norm="l2",
                adapt_every=None, max_elements=None):
    """record_every: also the error curve [(iteration, relative L2 error)], one row per that many updates (runs without adapt_every);
    adapt_every: local hp-refinement of the polar elements from the strong residual in divergence form"""
    Xb = _annulus_boundary(int(n_bound))
    bc = dict(hard_bc=annulus_hard_bc()) if hard_bc else dict(X_u_train=Xb, u_train=np.zeros(Xb.shape[0]))
    m = VPINNLinear(list(layers), mesh=annulus_mesh(n_r, n_theta, n_test), n_quad=int(n_quad), kappa=1.0, f=_annulus_f, lossb_weight=lossb_weight,
                    LR=LR, seed=seed, backend=backend, device=device, residual_norm=residual_norm,
                    strong_form="divergence" if adapt_every else None, **bc)
    rr, tt = np.meshgrid(np.linspace(1.0, 2.0, 41), np.linspace(0.0, np.pi / 2, 41))
    X = np.stack([(rr * np.cos(tt)).reshape(-1), (rr * np.sin(tt)).reshape(-1)], 1)
    u = _annulus_exact(X)[:, None]
    curve, it = [], 0
    rows = _train(m, n_iter, adapt_every, max_elements, verbose) if adapt_every else []
    while not adapt_every and it < int(n_iter):
        n = min(int(record_every or n_iter), int(n_iter) - it)
        m.train(n, verbose=False)
        it += n
        curve.append((it, m.rel_l2_error(X, u)))
    err = m.rel_l2_error(X, u)
    if verbose:
        for row in curve:
            print("It: %d, relative L2 error %.4e" % row)
        print("quarter annulus, %d polar elements (area %.6f), %s: relative L2 error %.4e (%s)"
              % (len(m.mesh), m.mesh.area(), "exact conditions (ansatz)" if hard_bc else "penalty", err, m.h.kernel_variant()))
        if residual_norm != "l2":
            print(_loss_line(m, err))
    return dict(model=m, rel_l2=err, X_test=X, u_test=u, loss_his=np.asarray(m.loss_his), curve=curve, adapt_rows=rows)


def rotated_tensor(angle_deg, ratio):
    """K = Q diag(1, ratio) Q^T, Q the rotation by angle_deg"""
    a = np.deg2rad(float(angle_deg))
    Q = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return Q @ np.diag([1.0, float(ratio)]) @ Q.T


def run_anisotropic(angle=30.0, ratio=0.05, n_elements=2, n_quad=10, n_test=5, n_iter=2000, layers=(2, 20, 20, 20, 1), n_bound=40, LR=1e-3,
                    lossb_weight=10.0, seed=1234, backend="auto", device=None, verbose=True, residual_norm="l2", adapt_every=None,
                    max_elements=None):
    K = rotated_tensor(angle, ratio)

    def f(P):
        s, c = np.sin(np.pi * P), np.cos(np.pi * P)
        return np.pi ** 2 * (-(K[0, 0] + K[1, 1]) * s[:, 0] * s[:, 1] + (K[0, 1] + K[1, 0]) * c[:, 0] * c[:, 1])
    t = np.linspace(-1.0, 1.0, int(n_bound))
    o = np.ones_like(t)
    Xb = np.concatenate([np.stack([t, -o], 1), np.stack([t, o], 1), np.stack([-o, t], 1), np.stack([o, t], 1)])
    g = np.linspace(-1.0, 1.0, int(n_elements) + 1)
    m = VPINNLinear(list(layers), grid_x=g, grid_y=g, n_quad=int(n_quad), n_test=int(n_test), kappa=K, f=f, X_u_train=Xb,
                    u_train=np.zeros(Xb.shape[0]), lossb_weight=lossb_weight, LR=LR, seed=seed, backend=backend, device=device,
                    residual_norm=residual_norm, strong_form="divergence" if adapt_every else None)
    rows = _train(m, n_iter, adapt_every, max_elements, verbose)
    gg = np.linspace(-1.0, 1.0, 81)
    X = np.stack([v.reshape(-1) for v in np.meshgrid(gg, gg)], 1)
    u = _l_exact(X)[:, None]
    err = m.rel_l2_error(X, u)
    if verbose:
        print("rotated anisotropy, angle %g degrees, ratio %g, K = %s, %d elements: relative L2 error %.4e (%s)"
              % (angle, ratio, K.round(4).tolist(), len(m.mesh), err, m.h.kernel_variant()))
        if residual_norm != "l2":
            print(_loss_line(m, err))
    return dict(model=m, rel_l2=err, X_test=X, u_test=u, loss_his=np.asarray(m.loss_his), adapt_rows=rows)


def _neumann_exact(P):
    x, y = P[:, 0], P[:, 1]
    return np.cos(np.pi * x) * np.cos(np.pi * y) + 0.3 * x ** 2 - 0.2 * y + 0.5


def _neumann_grad(P):
    x, y = P[:, 0], P[:, 1]
    return np.stack([-np.pi * np.sin(np.pi * x) * np.cos(np.pi * y) + 0.6 * x, -np.pi * np.cos(np.pi * x) * np.sin(np.pi * y) - 0.2], 1)


def run_neumann(n_elements=2, n_quad=10, n_test=5, n_iter=2000, layers=(2, 20, 20, 20, 1), n_bound=40, LR=1e-3, flux_weight=10.0, mean_weight=10.0,
                with_mean=True, seed=1234, backend="auto", device=None, verbose=True):
    """pure-Neumann Poisson: flux data on all sides and the mean of u (0.5 over the unit square) as an integral constraint; with_mean
    False leaves the constant free, and the error shows it"""
    t = np.linspace(0.0, 1.0, int(n_bound))
    o, z = np.ones_like(t), np.zeros_like(t)
    Xb = np.concatenate([np.stack([t, z], 1), np.stack([t, o], 1), np.stack([z, t], 1), np.stack([o, t], 1)])
    nb = np.concatenate([np.tile([0.0, -1.0], (t.size, 1)), np.tile([0.0, 1.0], (t.size, 1)), np.tile([-1.0, 0.0], (t.size, 1)), np.tile([1.0, 0.0], (t.size, 1))])
    g = np.linspace(0.0, 1.0, int(n_elements) + 1)
    cons = [dict(name="mean", kind="mean", target=0.5, weight=float(mean_weight))] if with_mean else None
    m = VPINNLinear(list(layers), grid_x=g, grid_y=g, n_quad=int(n_quad), n_test=int(n_test), kappa=1.0,
                    f=lambda P: -2.0 * np.pi ** 2 * np.cos(np.pi * P[:, 0]) * np.cos(np.pi * P[:, 1]) + 0.6, constraints=cons,
                    LR=LR, seed=seed, backend=backend, device=device)
    m.set_flux_data(Xb, g=np.sum(_neumann_grad(Xb) * nb, axis=1), b=nb, weight=flux_weight)
    m.train(int(n_iter), verbose=False)
    gg = np.linspace(0.0, 1.0, 41)
    X = np.stack([v.reshape(-1) for v in np.meshgrid(gg, gg)], 1)
    u = _neumann_exact(X)[:, None]
    err = m.rel_l2_error(X, u)
    d = m.predict(X).reshape(-1) - u.reshape(-1)
    err0 = float(np.linalg.norm(d - d.mean()) / np.linalg.norm(u))      # (the error once the best constant is taken out)
    m.loss()
    if verbose:
        print("pure Neumann, %s: relative L2 error %.4e (%.4e up to a constant); constraints %s (%s)"
              % ("int u = 0.5 imposed" if with_mean else "no mean constraint", err, err0, m.constraints(), m.h.kernel_variant()))
    return dict(model=m, rel_l2=err, rel_l2_mod_const=err0, X_test=X, u_test=u, loss_his=np.asarray(m.loss_his))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("problem", choices=["boundary-layer", "l-shape", "annulus", "anisotropic", "neumann"])
    ap.add_argument("--no-mean", action="store_true", help="neumann: leave the mean constraint out")
    ap.add_argument("--angle", type=float, default=30.0, help="anisotropic: rotation of the tensor's principal axes, degrees")
    ap.add_argument("--ratio", type=float, default=0.05, help="anisotropic: the smaller principal conductivity (the larger is 1)")
    ap.add_argument("--eps", type=float, default=0.05)
    ap.add_argument("--elements", type=int, default=8)
    ap.add_argument("--grade", type=float, default=2.0)
    ap.add_argument("--n-quad", type=int, default=None, help="quadrature points per direction (default: 20; neumann: 10)")
    ap.add_argument("--n-test", type=int, default=None, help="test functions per direction (default: 10; neumann: 5)")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--adapt-every", type=int, default=None, help="one local hp-refinement round after every K-th update")
    ap.add_argument("--max-elements", type=int, default=None)
    ap.add_argument("--hard-bc", action="store_true", help="boundary layer, annulus: exact Dirichlet conditions by ansatz instead of the penalty")
    ap.add_argument("--residual-norm", choices=["l2", "dual", "energy"], default="l2",
                    help="dual: each element's residual in the dual norm of its test space (robust VPINNs; on the annulus in the physical metric); "
                         "energy (l-shape, anisotropic, annulus): that norm in the energy inner product of the problem's own kappa")
    ap.add_argument("--gram-mass", type=float, default=0.0, help="weight of the L2 part of the dual norm's inner product")
    ap.add_argument("--lbfgs", type=int, default=0, help="boundary-layer, l-shape: L-BFGS iterations after the Adam iterations")
    a = ap.parse_args(argv)
    if a.lbfgs and a.problem not in ("boundary-layer", "l-shape"):
        ap.error("--lbfgs belongs to boundary-layer and l-shape")
    dq, dt = (10, 5) if a.problem == "neumann" else (20, 10)
    a.n_quad, a.n_test = a.n_quad or dq, a.n_test or dt
    if a.residual_norm == "energy" and a.problem == "boundary-layer":
        ap.error("--residual-norm energy belongs to l-shape, anisotropic and annulus")
    rn = _norm_arg(a.residual_norm, a.gram_mass, mapped=a.problem == "annulus")
    if a.problem == "boundary-layer":
        run_boundary_layer(eps=a.eps, n_elements=a.elements, n_quad=a.n_quad, n_test=a.n_test, n_iter=a.iters, grade=a.grade,
                           adapt_every=a.adapt_every, max_elements=a.max_elements, hard_bc=a.hard_bc, residual_norm=rn, lbfgs=a.lbfgs)
    elif a.problem == "annulus":
        run_annulus(n_quad=a.n_quad, n_test=a.n_test, n_iter=a.iters, hard_bc=a.hard_bc, record_every=max(1, a.iters // 10), residual_norm=rn,
                    adapt_every=a.adapt_every, max_elements=a.max_elements)
    elif a.problem == "neumann":
        run_neumann(n_quad=a.n_quad, n_test=a.n_test, n_iter=a.iters, with_mean=not a.no_mean)
    elif a.problem == "anisotropic":
        run_anisotropic(angle=a.angle, ratio=a.ratio, n_quad=a.n_quad, n_test=a.n_test, n_iter=a.iters, residual_norm=rn,
                        adapt_every=a.adapt_every, max_elements=a.max_elements)
    else:
        run_l_shape(n_iter=a.iters, n_quad=a.n_quad, n_test=a.n_test, adapt_every=a.adapt_every, max_elements=a.max_elements, residual_norm=rn,
                    lbfgs=a.lbfgs)


if __name__ == "__main__":
    main()
