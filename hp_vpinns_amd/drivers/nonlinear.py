"""Standard nonlinear problems on the variable-coefficient class (VPINNNonlinear): three with a pointwise nonlinear term, three with a
solution-dependent diffusion coefficient; each with an exact or manufactured solution and Dirichlet data from it; prints the relative
L2 error.

  bratu        u'' + lam exp(u) = 0 on [0, 1], u(0) = u(1) = 0; the lower branch in closed form,
               u = -2 ln(cosh((x - 1/2) th / 2) / cosh(th / 4)), th the lower root of th = sqrt(2 lam) cosh(th / 4)
               (lam below the critical 3.5138).  In the class's convention: kappa = 1, exponential = lam, f = 0.
  burgers      u_t + u u_x - nu u_xx = f in space-time, (x, t) in [-1, 1] x [0, 1] with y = t: kappa = (-nu, 0), beta = (0, 1),
               advection = (1, 0); u = exp(-t) sin(pi x) manufactured, f from it; data on t = 0 and x = +-1.
  allen-cahn   eps^2 lap u + u - u^3 = 0 on [-1, 1]^2: kappa = eps^2, sigma = 1, cubic = -1; the exact diagonal front
               u = tanh((x + y) / (2 eps)) (the 1-D steady front tanh(s / (sqrt(2) eps)) along s = (x + y) / sqrt(2)), f = 0; data on all four sides.
  heat-ku      div((1 + u^2) grad u) = f on [-1, 1]^2: diffusivity poly = (1, 0, 1); u = 0.8 sin(pi x / 2 + 0.3) cos(pi y / 2 - 0.2)
               manufactured, f from it; data on all four sides.
  p-laplace    div((eps^2 + |grad u|^2)^((p - 2) / 2) grad u) = f, the regularised p-Laplacian: diffusivity shift = eps^2,
               power = (p - 2) / 2; the same manufactured u.
  minimal-surface   div(grad u / sqrt(1 + |grad u|^2)) = 0 on [-1, 1]^2: diffusivity shift = 1, power = -1/2; Scherk's surface
               u = log(cos x) - log(cos y), Dirichlet data from it, f = 0.

    python -m hp_vpinns_amd.drivers.nonlinear bratu --lam 1.0
    python -m hp_vpinns_amd.drivers.nonlinear heat-ku
    python -m hp_vpinns_amd.drivers.nonlinear p-laplace --p 3 --eps 0.1
    python -m hp_vpinns_amd.drivers.nonlinear minimal-surface --adapt-every 500 --max-elements 64
    python -m hp_vpinns_amd.drivers.nonlinear burgers --nu 0.05
    python -m hp_vpinns_amd.drivers.nonlinear allen-cahn --eps 0.2
    python -m hp_vpinns_amd.drivers.nonlinear allen-cahn --eps 0.1 --adapt-every 500 --max-elements 64

    python -m hp_vpinns_amd.drivers.nonlinear burgers --nu 0.05 --hard-bc

--hard-bc (burgers): the initial and boundary conditions are built into the trial function, u = G + D N with D = (1 - x^2) t, which
vanishes on t = 0 and x = +-1, and G = sin(pi x), the driver's own data there (VPINNNonlinear(hard_bc=...)): no data points, no weight.

--adapt-every K (burgers, allen-cahn and the quasilinear three): local hp-refinement (VPINNNonlinear(strong_form="elementwise").train_adaptive) after every
K-th update, at most --max-elements elements; one (iteration, elements, loss) row is printed per round.  Together with --hard-bc the
strong residual is taken in divergence form (strong_form="divergence"): the ansatz has no second derivatives to offer.  The three
quasilinear problems always take the divergence form: the elementwise one would need the derivative of mu along the element.

`setup(problem, ...)` builds everything a run needs on the host (no GPU); `run(s, ...)` creates the model from it and trains.
"""
import argparse

import numpy as np

# the smallest setting of the Bratu run (tests/test_gpu_nonlinear.py trains it once)
SMALLEST = dict(problem="bratu", lam=1.0, n_elements=3, n_quad=8, n_test=4, width=8, depth=2)
# ... and of the minimal-surface run (tests/test_gpu_quasilinear.py)
SMALLEST_QUASI = dict(problem="minimal-surface", n_elements=2, n_quad=6, n_test=3, width=8, depth=2, n_bound=12)
QUASI = ("heat-ku", "p-laplace", "minimal-surface")


def bratu_theta(lam):
    """the lower root of th = sqrt(2 lam) cosh(th / 4), by bisection between 0 and the maximum of th - sqrt(2 lam) cosh(th / 4)"""
    c = np.sqrt(2.0 * float(lam))

    def g(th):
        return th - c * np.cosh(th / 4.0)
    lo, hi = 0.0, 4.0 * np.arcsinh(4.0 / c)
    if not (lam > 0 and g(hi) > 0):
        raise ValueError("Bratu's problem has its two solutions for 0 < lam < 3.5138 only")
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if g(mid) < 0 else (lo, mid)
    return 0.5 * (lo + hi)


def bratu_exact(x, lam):
    th = bratu_theta(lam)
    x = np.asarray(x, dtype=np.float64)
    return -2.0 * np.log(np.cosh((x - 0.5) * th / 2.0) / np.cosh(th / 4.0))


def _burgers_exact(P):
    return np.exp(-P[:, 1]) * np.sin(np.pi * P[:, 0])


def _allen_cahn_exact(P, eps):
    return np.tanh((P[:, 0] + P[:, 1]) / (2.0 * eps))


def manufactured(P):
    """u, grad u (n, 2), Hessian (n, 2, 2) of the manufactured solution of heat-ku and p-laplace"""
    a, b = np.pi / 2 * P[:, 0] + 0.3, np.pi / 2 * P[:, 1] - 0.2
    c, h = 0.8, np.pi / 2
    u = c * np.sin(a) * np.cos(b)
    du = np.stack([c * h * np.cos(a) * np.cos(b), -c * h * np.sin(a) * np.sin(b)], 1)
    uxy = -c * h * h * np.cos(a) * np.sin(b)
    H = np.stack([np.stack([-h * h * u, uxy], 1), np.stack([uxy, -h * h * u], 1)], 1)
    return u, du, H


def scherk(P):
    """Scherk's surface u = log(cos x) - log(cos y), |x|, |y| < pi / 2, with its gradient and Hessian"""
    x, y = P[:, 0], P[:, 1]
    z = np.zeros_like(x)
    return (np.log(np.cos(x)) - np.log(np.cos(y)), np.stack([-np.tan(x), np.tan(y)], 1),
            np.stack([np.stack([-1.0 / np.cos(x) ** 2, z], 1), np.stack([z, 1.0 / np.cos(y) ** 2], 1)], 1))


def quasi_mu(poly, shift, power, u, s):
    """mu = (m0 + m1 u + m2 u^2) (shift + s)^power and its partials (mu, mu_u, mu_s) for constants poly, shift, power"""
    m0, m1, m2 = poly
    Pu, B = m0 + m1 * u + m2 * u * u, (shift + s) ** power
    return Pu * B, (m1 + 2.0 * m2 * u) * B, power * Pu * (shift + s) ** (power - 1.0)


def quasi_rhs(diffusivity, exact, P):
    """f = div(mu grad u) of an exact solution: mu lap u + mu_u |grad u|^2 + 2 mu_s grad u^T H grad u"""
    u, du, H = exact(P)
    s = np.sum(du * du, axis=1)
    mu, mu_u, mu_s = quasi_mu(diffusivity["poly"], diffusivity["shift"], diffusivity["power"], u, s)
    return mu * (H[:, 0, 0] + H[:, 1, 1]) + mu_u * s + 2.0 * mu_s * np.einsum("na,nab,nb->n", du, H, du)


def quasi_diffusivity(problem, p=3.0, eps=0.1):
    """the diffusivity= of the three quasilinear problems, all keys filled in"""
    if problem == "heat-ku":
        return dict(poly=(1.0, 0.0, 1.0), shift=1.0, power=0.0)
    if problem == "p-laplace":
        if not (p > 1.0 and eps > 0.0):
            raise ValueError("p-laplace needs p > 1 and eps > 0")
        return dict(poly=(1.0, 0.0, 0.0), shift=float(eps) ** 2, power=(float(p) - 2.0) / 2.0)
    return dict(poly=(1.0, 0.0, 0.0), shift=1.0, power=-0.5)


def burgers_hard_bc():
    """dict(g=, d=) for VPINNNonlinear(hard_bc=...): D = (1 - x^2) t and G = sin(pi x), each with its gradient (d/dx, d/dt)"""
    def g(P):
        x = P[:, 0]
        return np.stack([np.sin(np.pi * x), np.pi * np.cos(np.pi * x), np.zeros_like(x)], 1)

    def d(P):
        x, t = P[:, 0], P[:, 1]
        return np.stack([(1.0 - x * x) * t, -2.0 * x * t, 1.0 - x * x], 1)
    return dict(g=g, d=d)


def setup(problem, lam=1.0, nu=0.05, eps=0.2, n_elements=None, n_quad=10, n_test=5, width=20, depth=3, n_bound=40, lossb_weight=10.0,
          hard_bc=False, p=3.0):
    """dict(layers, model = the keyword arguments of VPINNNonlinear, X_test, u_test) of one of the problems; hard_bc (burgers):
    the conditions by ansatz instead of data points"""
    hidden = [int(width)] * int(depth)
    if problem in QUASI:
        if hard_bc:
            raise ValueError("hard_bc is set up for burgers")
        ne = 4 if n_elements is None else int(n_elements)
        dif = quasi_diffusivity(problem, p, eps)
        exact = scherk if problem == "minimal-surface" else manufactured
        t = np.linspace(-1.0, 1.0, int(n_bound))
        o = np.ones_like(t)
        Xb = np.concatenate([np.stack([t, -o], 1), np.stack([t, o], 1), np.stack([-o, t], 1), np.stack([o, t], 1)])
        g = np.stack([v.reshape(-1) for v in np.meshgrid(np.linspace(-1.0, 1.0, 81), np.linspace(-1.0, 1.0, 81))], 1)
        f = 0.0 if problem == "minimal-surface" else (lambda P: quasi_rhs(dif, exact, P))
        grid = np.linspace(-1.0, 1.0, ne + 1)
        return dict(layers=[2] + hidden + [1], X_test=g, u_test=exact(g)[0][:, None], exact=exact,
                    model=dict(grid_x=grid, grid_y=grid, n_quad=int(n_quad), n_test=int(n_test), lossb_weight=lossb_weight, kappa=1.0,
                               diffusivity=dif, f=f, X_u_train=Xb, u_train=exact(Xb)[0]))
    if hard_bc and problem != "burgers":
        raise ValueError("hard_bc is set up for burgers")
    if problem == "bratu":
        ne = 4 if n_elements is None else int(n_elements)
        X = np.linspace(0.0, 1.0, 401)[:, None]
        return dict(layers=[1] + hidden + [1], X_test=X, u_test=bratu_exact(X, lam),
                    model=dict(grid_x=np.linspace(0.0, 1.0, ne + 1), n_quad=int(n_quad), n_test=int(n_test), kappa=1.0, exponential=float(lam), f=0.0,
                               X_u_train=np.array([[0.0], [1.0]]), u_train=np.zeros(2), lossb_weight=lossb_weight, activation="sin"))
    ne = 4 if n_elements is None else int(n_elements)
    t = np.linspace(-1.0, 1.0, int(n_bound))
    if problem == "burgers":
        nu = float(nu)

        def f(P):
            u = _burgers_exact(P)
            ux = np.pi * np.exp(-P[:, 1]) * np.cos(np.pi * P[:, 0])
            return -u + u * ux + nu * np.pi ** 2 * u               # u_t + u u_x - nu u_xx
        s = (t + 1.0) / 2.0
        Xb = np.concatenate([np.stack([t, 0 * t], 1), np.stack([0 * s - 1.0, s], 1), np.stack([0 * s + 1.0, s], 1)])
        exact, gy = _burgers_exact, np.linspace(0.0, 1.0, ne + 1)
        op = dict(kappa=np.array([-nu, 0.0]), beta=np.array([0.0, 1.0]), advection=np.array([1.0, 0.0]), f=f)
        g = np.stack([v.reshape(-1) for v in np.meshgrid(np.linspace(-1.0, 1.0, 81), np.linspace(0.0, 1.0, 41))], 1)
    elif problem == "allen-cahn":
        eps = float(eps)

        def exact(P):
            return _allen_cahn_exact(P, eps)
        o = np.ones_like(t)
        Xb = np.concatenate([np.stack([t, -o], 1), np.stack([t, o], 1), np.stack([-o, t], 1), np.stack([o, t], 1)])
        gy = np.linspace(-1.0, 1.0, ne + 1)
        op = dict(kappa=eps ** 2, sigma=1.0, cubic=-1.0, f=0.0)
        g = np.stack([v.reshape(-1) for v in np.meshgrid(np.linspace(-1.0, 1.0, 81), np.linspace(-1.0, 1.0, 81))], 1)
    else:
        raise ValueError("problem is one of bratu, burgers, allen-cahn, heat-ku, p-laplace, minimal-surface")
    bc = dict(hard_bc=burgers_hard_bc()) if hard_bc else dict(X_u_train=Xb, u_train=exact(Xb))
    return dict(layers=[2] + hidden + [1], X_test=g, u_test=exact(g)[:, None],
                model=dict(grid_x=np.linspace(-1.0, 1.0, ne + 1), grid_y=gy, n_quad=int(n_quad), n_test=int(n_test),
                           lossb_weight=lossb_weight, **bc, **op))


def run(s, n_iter=2000, validate_every=0, LR=1e-3, seed=1234, backend="auto", device=None, verbose=True, adapt_every=None,
        max_elements=None, residual_norm="l2", lbfgs=0):
    """lbfgs=N: an L-BFGS stage of N iterations after the Adam iterations.  Train the problem of `setup`'s dict; with validate_every the error history is sampled on the device (train_validated); with
    adapt_every the elements are refined locally (train_adaptive: the model is built with strong_form="elementwise", or
    "divergence" where the setup has an ansatz).  The two are not combined: giving both raises ValueError."""
    from ..vpinn import VPINNNonlinear
    if adapt_every and validate_every:
        raise ValueError("adapt_every and validate_every cannot be combined: run one or the other")
    kind = "divergence" if "hard_bc" in s["model"] or "diffusivity" in s["model"] else "elementwise"
    m = VPINNNonlinear(s["layers"], LR=LR, seed=seed, backend=backend, device=device, strong_form=kind if adapt_every else None,
                       residual_norm=residual_norm, **s["model"])
    his, rows = None, []
    if adapt_every:
        rows = m.train_adaptive(int(n_iter), int(adapt_every), max_elements=max_elements)
        if verbose:
            for it, ne, loss in rows:
                print("It: %d, adapted to %d elements, loss on the new mesh: %.3e" % (it, ne, loss))
    elif validate_every:
        m.set_validation(s["X_test"], s["u_test"])
        his = m.train_validated(int(n_iter), int(validate_every))
        if verbose:
            for it, e2, emax in zip(*his):
                print("It: %d, relative L2 error %.4e, max error %.4e" % (it, e2, emax))
    else:
        m.train(int(n_iter), verbose=verbose)
    from . import lbfgs_stage
    lbfgs_stage(m, lbfgs, lambda: m.rel_l2_error(s["X_test"], s["u_test"]), verbose=verbose)
    err = m.rel_l2_error(s["X_test"], s["u_test"])
    if verbose:
        print("relative L2 error %.4e after %d iterations (%s)" % (err, n_iter, m.h.kernel_variant()))
        # (the test solutions of this driver come without gradients: sqrt(lossv) stands beside the error that is known)
        print("sqrt(lossv) %.4e (residual norm %s)" % (np.sqrt(float(np.asarray(m.loss())[2])), m.residual_norm))
    return dict(model=m, rel_l2=err, history=his, loss_his=np.asarray(m.loss_his), adapt_rows=rows)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("problem", choices=["bratu", "burgers", "allen-cahn", "heat-ku", "p-laplace", "minimal-surface"])
    ap.add_argument("--lam", type=float, default=1.0)
    ap.add_argument("--nu", type=float, default=0.05)
    ap.add_argument("--eps", type=float, default=None, help="allen-cahn: the front width (default 0.2); p-laplace: the regularisation (default 0.1)")
    ap.add_argument("--p", type=float, default=3.0, help="p-laplace: the exponent p > 1")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--width", type=int, default=20)
    ap.add_argument("--validate-every", type=int, default=0)
    ap.add_argument("--adapt-every", type=int, default=None, help="one local hp-refinement round after every K-th update (not together with --validate-every)")
    ap.add_argument("--max-elements", type=int, default=None)
    ap.add_argument("--hard-bc", action="store_true", help="burgers: initial and boundary conditions by ansatz instead of data points")
    ap.add_argument("--residual-norm", choices=["l2", "dual"], default="l2", help="dual: each element's residual in the dual norm of its test space (robust VPINNs)")
    ap.add_argument("--gram-mass", type=float, default=0.0, help="weight of the L2 part of the dual norm's inner product")
    ap.add_argument("--lbfgs", type=int, default=0, help="L-BFGS iterations after the Adam iterations")
    a = ap.parse_args(argv)
    if a.eps is None:
        a.eps = 0.1 if a.problem == "p-laplace" else 0.2
    run(setup(a.problem, lam=a.lam, nu=a.nu, eps=a.eps, width=a.width, hard_bc=a.hard_bc, p=a.p), n_iter=a.iters, validate_every=a.validate_every,
        adapt_every=a.adapt_every, max_elements=a.max_elements,
        residual_norm="l2" if a.residual_norm == "l2" else dict(kind="dual", mass=a.gram_mass), lbfgs=a.lbfgs)


if __name__ == "__main__":
    main()
