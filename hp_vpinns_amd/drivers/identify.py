"""Two coefficient-identification problems on the variable-coefficient class (VPINNLinear / VPINNNonlinear with `trainable=`), each
with a manufactured solution and observations from it: the network and the unknown coefficients are trained together, and the run
prints the recovered values beside the true ones.

  conductivity   (kappa u')' = f on [-1, 1] with kappa piecewise constant, kappa = k1 for x < 0 and k2 for x >= 0 (the interface is
                 an element boundary): two unknowns whose directions are the indicator functions of the two subdomains; u = cos(pi x)
                 manufactured -- its flux kappa u' is continuous (zero) across the interface, so the quadrature node x = 0 that both
                 neighbours own may carry either value --, f = kappa u'' from the true values, interior observations of u through
                 X_u_train.
  burgers-nu     u_t + u u_x - nu u_xx = f in space-time, (x, t) in [-1, 1] x [0, 1] with y = t: beta = (0, 1), advection = (1, 0) and
                 the unknown viscosity nu with the direction kappa = (-1, 0); u = exp(-t) sin(pi x) manufactured, f from the true nu;
                 observations on t = 0, x = +-1 and at interior points.

    python -m hp_vpinns_amd.drivers.identify conductivity --k1 1.0 --k2 2.0
    python -m hp_vpinns_amd.drivers.identify burgers-nu --nu 0.1

`setup(problem, ...)` builds everything a run needs on the host (no GPU); `run(s, ...)` creates the model from it and trains.
"""
import argparse

import numpy as np

# the smallest setting of each run (tests/test_gpu_ident.py trains them once); STEPS: the number of Adam steps at LR = 1e-2 after
# which the CPU reference's own trajectory (tests/ident_reference.py) has the coefficients' errors below their initial ones by a
# factor of more than ten -- conductivity 0.5, 0.5 -> 0.023, 0.037 after 800; viscosity 0.2 -> 0.006 after 400
SMALLEST = {
    "conductivity": dict(problem="conductivity", k1=1.0, k2=2.0, n_elements=2, n_quad=8, n_test=4, width=8, depth=2, n_obs=9),
    "burgers-nu": dict(problem="burgers-nu", nu=0.3, n_elements=2, n_quad=6, n_test=3, width=8, depth=2, n_obs=5, n_bound=9),
}
SMALLEST_LR = 1e-2
SMALLEST_STEPS = {"conductivity": 800, "burgers-nu": 400}


def _left(P):
    return (P[:, 0] < 0.0).astype(np.float64)


def _right(P):
    return (P[:, 0] >= 0.0).astype(np.float64)


def setup(problem, k1=1.0, k2=2.0, nu=0.1, init=None, n_elements=None, n_quad=10, n_test=5, width=20, depth=3, n_obs=21, n_bound=40,
          lossb_weight=10.0):
    """dict(layers, nonlinear, model = the keyword arguments of the class, true = {name: value}, X_test, u_test) of one problem;
    init: the initial value of every unknown (default: 1.5 for the conductivities, 0.5 for the viscosity)"""
    hidden = [int(width)] * int(depth)
    if problem == "conductivity":
        ne = 4 if n_elements is None else int(n_elements)
        if ne % 2:
            raise ValueError("the interface x = 0 must be an element boundary: an even number of elements")
        k1, k2, c0 = float(k1), float(k2), 1.5 if init is None else float(init)

        def f(P):
            return -(k1 * _left(P) + k2 * _right(P)) * np.pi ** 2 * np.cos(np.pi * P[:, 0])      # kappa u''
        Xo = np.linspace(-1.0, 1.0, int(n_obs))[:, None]
        X = np.linspace(-1.0, 1.0, 401)[:, None]
        return dict(layers=[1] + hidden + [1], nonlinear=False, true=dict(k1=k1, k2=k2), X_test=X, u_test=np.cos(np.pi * X),
                    model=dict(grid_x=np.linspace(-1.0, 1.0, ne + 1), n_quad=int(n_quad), n_test=int(n_test), kappa=0.0, f=f, X_u_train=Xo,
                               u_train=np.cos(np.pi * Xo[:, 0]), lossb_weight=lossb_weight, activation="sin",
                               trainable=[dict(name="k1", init=c0, kappa=_left), dict(name="k2", init=c0, kappa=_right)]))
    if problem == "burgers-nu":
        ne = 4 if n_elements is None else int(n_elements)
        nu, c0 = float(nu), 0.5 if init is None else float(init)

        def exact(P):
            return np.exp(-P[:, 1]) * np.sin(np.pi * P[:, 0])

        def f(P):
            u = exact(P)
            ux = np.pi * np.exp(-P[:, 1]) * np.cos(np.pi * P[:, 0])
            return -u + u * ux + nu * np.pi ** 2 * u               # u_t + u u_x - nu u_xx
        t = np.linspace(-1.0, 1.0, int(n_bound))
        s = (t + 1.0) / 2.0
        gi = np.stack([v.reshape(-1) for v in np.meshgrid(np.linspace(-0.8, 0.8, int(n_obs)), np.linspace(0.2, 1.0, int(n_obs)))], 1)
        Xo = np.concatenate([np.stack([t, 0 * t], 1), np.stack([0 * s - 1.0, s], 1), np.stack([0 * s + 1.0, s], 1), gi])
        g = np.stack([v.reshape(-1) for v in np.meshgrid(np.linspace(-1.0, 1.0, 81), np.linspace(0.0, 1.0, 41))], 1)
        return dict(layers=[2] + hidden + [1], nonlinear=True, true=dict(nu=nu), X_test=g, u_test=exact(g)[:, None],
                    model=dict(grid_x=np.linspace(-1.0, 1.0, ne + 1), grid_y=np.linspace(0.0, 1.0, ne + 1), n_quad=int(n_quad), n_test=int(n_test),
                               kappa=np.array([0.0, 0.0]), beta=np.array([0.0, 1.0]), advection=np.array([1.0, 0.0]), f=f, X_u_train=Xo,
                               u_train=exact(Xo), lossb_weight=lossb_weight,
                               trainable=[dict(name="nu", init=c0, kappa=np.array([-1.0, 0.0]))]))
    raise ValueError("problem is one of conductivity, burgers-nu")


def run(s, n_iter=5000, LR=1e-3, seed=1234, backend="auto", device=None, verbose=True, lbfgs=0):
    """Train the problem of `setup`'s dict (lbfgs=N: N L-BFGS iterations after the Adam iterations; the coefficients move with the network); returns dict(model, coefficients, true, rel_l2, loss_his)"""
    from ..vpinn import VPINNLinear, VPINNNonlinear
    m = (VPINNNonlinear if s["nonlinear"] else VPINNLinear)(s["layers"], LR=LR, seed=seed, backend=backend, device=device, **s["model"])
    m.train(int(n_iter), verbose=verbose)
    from . import lbfgs_stage
    lbfgs_stage(m, lbfgs, lambda: max(abs(v - s["true"][k]) / abs(s["true"][k]) for k, v in m.coefficients().items()),
                what="largest relative coefficient error", verbose=verbose)
    c = m.coefficients()
    err = m.rel_l2_error(s["X_test"], s["u_test"])
    if verbose:
        for k, v in c.items():
            print("%s = %.6f (true %.6f)" % (k, v, s["true"][k]))
        print("relative L2 error of u %.4e after %d iterations (%s)" % (err, n_iter, m.h.kernel_variant()))
    return dict(model=m, coefficients=c, true=dict(s["true"]), rel_l2=err, loss_his=np.asarray(m.loss_his))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("problem", choices=["conductivity", "burgers-nu"])
    ap.add_argument("--k1", type=float, default=1.0)
    ap.add_argument("--k2", type=float, default=2.0)
    ap.add_argument("--nu", type=float, default=0.1)
    ap.add_argument("--init", type=float, default=None)
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--width", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--lbfgs", type=int, default=0, help="L-BFGS iterations after the Adam iterations")
    a = ap.parse_args(argv)
    run(setup(a.problem, k1=a.k1, k2=a.k2, nu=a.nu, init=a.init, width=a.width), n_iter=a.iters, LR=a.lr, lbfgs=a.lbfgs)


if __name__ == "__main__":
    main()
