"""Poisson 2-D driver: the `__main__` block of the reference script restated (P2:265-435).

u = (0.1 sin(2 pi x) + tanh(10 x)) sin(2 pi y) on [-1,1]^2, Laplace(u) = f (P2:296-310);
N_el_x x N_el_y elements, tensor GLL rule with N_quad points per direction, N_test_x x N_test_y
Legendre-difference test functions per element; F_ext[ex,ey][k][r] (P2:381-414); 4 x N_bound
boundary points by LHS (P2:314-347).  Plotting (P2:443-534) is not restated.
"""
import argparse

import numpy as np

from ..quadrature import GaussLobattoJacobiWeights
from ..sampling import lhs
from ..testfcn import Test_fcn

omegax = omegay = 2 * np.pi
r1 = 10


def u_ext(x, y):                                                 # P2:300-302
    return (0.1 * np.sin(omegax * x) + np.tanh(r1 * x)) * np.sin(omegay * (y))


def f_ext(x, y):                                                 # P2:304-307
    return (-0.1 * (omegax ** 2) * np.sin(omegax * x) - (2 * r1 ** 2) * (np.tanh(r1 * x)) / ((np.cosh(r1 * x)) ** 2)) \
        * np.sin(omegay * (y)) + (0.1 * np.sin(omegax * x) + np.tanh(r1 * x)) * (-omegay ** 2 * np.sin(omegay * (y)))


def grad_u_ext(x, y):
    """(u_x, u_y) of u_ext: what a Neumann side prescribes"""
    return ((0.1 * omegax * np.cos(omegax * x) + r1 / np.cosh(r1 * x) ** 2) * np.sin(omegay * y),
            (0.1 * np.sin(omegax * x) + np.tanh(r1 * x)) * omegay * np.cos(omegay * y))


# the boundary points of `setup` come side by side in this order (P2:314-347), N_bound rows each, with these outward normals
SIDES = {"top": (0, (0.0, 1.0)), "bottom": (1, (0.0, -1.0)), "right": (2, (1.0, 0.0)), "left": (3, (-1.0, 0.0))}


def split_neumann(s, sides):
    """(setup dict without the boundary points of `sides`, flux data dict(X, g, b) for `set_flux_data`): the points of those sides
    leave X_u_train / u_train and carry the exact normal derivative g = n . grad u_ext instead of the value."""
    sides = [v.strip() for v in sides.split(",")] if isinstance(sides, str) else list(sides)
    bad = [v for v in sides if v not in SIDES]
    if bad or len(set(sides)) != len(sides) or not 0 < len(sides) < 4:
        raise ValueError("neumann sides: one to three of left,right,bottom,top (a Dirichlet side must remain); got %r" % (sides,))
    nb = s["X_u_train"].shape[0] // 4
    keep = np.ones(4 * nb, dtype=bool)
    X, g, b = [], [], []
    for side in sides:
        k, n = SIDES[side]
        rows = slice(k * nb, (k + 1) * nb)
        keep[rows] = False
        Xs = s["X_u_train"][rows]
        ux, uy = grad_u_ext(Xs[:, 0], Xs[:, 1])
        X.append(Xs); g.append(n[0] * ux + n[1] * uy); b.append(np.tile(n, (nb, 1)))
    s = dict(s, X_u_train=s["X_u_train"][keep], u_train=s["u_train"][keep])
    return s, dict(X=np.concatenate(X), g=np.concatenate(g), b=np.concatenate(b))


def setup(N_el_x=4, N_el_y=4, N_test_x=5, N_test_y=5, N_quad=10, N_bound=80, N_residual=100, seed=1234,
          with_test_grid=True, assemble="host", device=0):
    np.random.seed(seed)                                         # P2:23
    ones = lambda a, v: np.full((len(a), 1), float(v))           # noqa: E731
    x_up = 2 * lhs(1, N_bound) - 1                               # P2:314-320
    x_up_train, u_up_train = np.hstack((x_up, ones(x_up, 1))), u_ext(x_up, ones(x_up, 1))
    x_lo = 2 * lhs(1, N_bound) - 1                               # P2:322-328
    x_lo_train, u_lo_train = np.hstack((x_lo, ones(x_lo, -1))), u_ext(x_lo, ones(x_lo, -1))
    y_ri = 2 * lhs(1, N_bound) - 1                               # P2:330-336
    x_ri_train, u_ri_train = np.hstack((ones(y_ri, 1), y_ri)), u_ext(ones(y_ri, 1), y_ri)
    y_le = 2 * lhs(1, N_bound) - 1                               # P2:338-344
    x_le_train, u_le_train = np.hstack((ones(y_le, -1), y_le)), u_ext(ones(y_le, -1), y_le)
    X_u_train = np.concatenate((x_up_train, x_lo_train, x_ri_train, x_le_train))
    u_train = np.concatenate((u_up_train, u_lo_train, u_ri_train, u_le_train))
    grid_pt = lhs(2, N_residual)                                 # P2:349-354 (PINN residual points)
    xf, yf = 2 * grid_pt[:, 0] - 1, 2 * grid_pt[:, 1] - 1
    X_f_train = np.hstack((xf[:, None], yf[:, None]))
    f_train = f_ext(xf, yf)[:, None]
    X_quad, WX_quad = GaussLobattoJacobiWeights(N_quad, 0, 0)    # P2:357-364
    xx, yy = np.meshgrid(X_quad, X_quad)
    wxx, wyy = np.meshgrid(WX_quad, WX_quad)
    XY_quad_train = np.hstack((xx.flatten()[:, None], yy.flatten()[:, None]))
    WXY_quad_train = np.hstack((wxx.flatten()[:, None], wyy.flatten()[:, None]))
    NE_x, NE_y = N_el_x, N_el_y                                  # P2:368-376
    delta_x, delta_y = 2 / NE_x, 2 / NE_y
    grid_x = np.asarray([-1 + i * delta_x for i in range(NE_x + 1)])
    grid_y = np.asarray([-1 + i * delta_y for i in range(NE_y + 1)])
    # N_test_x / N_test_y: an integer (the reference, P2:283-286) or one entry per element column / row -- the p-refinement the
    # class bodies read per element (P2:72-73) and the commented-out list of P2:377 hints at
    ragged = not (np.isscalar(N_test_x) and np.isscalar(N_test_y))
    nax = [int(N_test_x)] * NE_x if np.isscalar(N_test_x) else [int(v) for v in N_test_x]
    nay = [int(N_test_y)] * NE_y if np.isscalar(N_test_y) else [int(v) for v in N_test_y]
    if len(nax) != NE_x or len(nay) != NE_y:
        raise ValueError("N_test_x / N_test_y given as lists need one entry per element column / row")
    N_testfcn_total = [nax, nay]
    N_test_x, N_test_y = max(nax), max(nay)                      # (the family is nested: every element's block is a corner of this one)
    tx, ty = Test_fcn(N_test_x, X_quad), Test_fcn(N_test_y, X_quad)      # (Nt, Q)
    ax, by = tx * WX_quad, ty * WX_quad
    F_ext_total = np.empty((NE_x, NE_y, N_test_y, N_test_x))
    if assemble == "device":                                     # same numbers from the projection kernel
        from ..rhs import assemble_F_ext_2d
        F_ext_total = assemble_F_ext_2d(f_ext, grid_x, grid_y, N_test_x, N_test_y, N_quad, device=device)
    for ex in range(NE_x if assemble != "device" else 0):        # P2:386-411
        xq = grid_x[ex] + (grid_x[ex + 1] - grid_x[ex]) / 2 * (X_quad + 1)
        for ey in range(NE_y):
            yq = grid_y[ey] + (grid_y[ey + 1] - grid_y[ey]) / 2 * (X_quad + 1)
            jacobian = ((grid_x[ex + 1] - grid_x[ex]) / 2) * ((grid_y[ey + 1] - grid_y[ey]) / 2)
            fq = f_ext(xq[None, :], yq[:, None])                 # [j (y)][i (x)]
            F_ext_total[ex, ey] = jacobian * (by @ fq @ ax.T)    # [k][r]
    if ragged:      # what the reference class indexes with [ex, ey]: an (NE_x, NE_y) array of (N_test_y[ey], N_test_x[ex]) blocks
        blocks = np.empty((NE_x, NE_y), dtype=object)
        for ex in range(NE_x):
            for ey in range(NE_y):
                blocks[ex, ey] = F_ext_total[ex, ey][:nay[ey], :nax[ex]].copy()
        F_ext_total = blocks
    out = dict(X_u_train=X_u_train, u_train=u_train, X_f_train=X_f_train, f_train=f_train,
               XY_quad_train=XY_quad_train, WXY_quad_train=WXY_quad_train, F_ext_total=F_ext_total,
               grid_x=grid_x, grid_y=grid_y, N_testfcn_total=N_testfcn_total)
    if with_test_grid:
        delta_test = 0.01                                        # P2:418-426
        xtest = np.arange(-1, 1 + delta_test, delta_test)
        ytest = np.arange(-1, 1 + delta_test, delta_test)
        Xg, Yg = np.meshgrid(xtest, ytest)                       # x fastest, like the reference's nested list
        out["X_test"] = np.hstack((Xg.flatten()[:, None], Yg.flatten()[:, None]))
        out["u_test"] = u_ext(out["X_test"][:, 0:1], out["X_test"][:, 1:2])
    return out


def build_model(s, Net_layer, var_form=1, init_params=None, backend="auto", loss_his=None, **kw):
    from ..vpinn import VPINN2D
    X_test = s.get("X_test", s["X_u_train"])
    u_test = s.get("u_test", s["u_train"])
    return VPINN2D(s["X_u_train"], s["u_train"], s["X_f_train"], s["f_train"], s["XY_quad_train"], s["WXY_quad_train"],
                   None, s["F_ext_total"], s["grid_x"], s["grid_y"], s["N_testfcn_total"], X_test, u_test, Net_layer,
                   var_form=var_form, init_params=init_params, backend=backend, loss_his=loss_his, **kw)   # P2:430-431


def run(scheme="VPINNs", Net_layer=None, var_form=1, N_el_x=4, N_el_y=4, N_test_x=5, N_test_y=5, N_quad=10,
        N_bound=80, N_residual=100, n_iter=10000 + 1, init_params=None, backend="auto", record_every=1, verbose=True,
        validate_every=None, adapt_every=None, max_elements=None, neumann_sides=None, flux_weight=1.0, lbfgs=0):
    """lbfgs=N: an L-BFGS stage of N iterations after the Adam iterations (`train_lbfgs`; loss and error before and after are printed).
    neumann_sides: a comma list out of left,right,bottom,top -- those sides carry the flux n . grad u of the exact solution
    (`set_flux_data`, weight flux_weight) instead of its value.  adapt_every=K: local hp-refinement (`train_adaptive`, right-hand side f_ext) after every K-th update, at most max_elements
    elements.  P2:279-288 hyper-parameters (reference defaults) -> trained model, prediction and L2 error.  validate_every=K trains
    through `train_validated` instead of `train`: the error on the test grid after every K-th update, reduced on the device."""
    Net_layer = [2] + [5] * 3 + [1] if Net_layer is None else Net_layer        # P2:280
    s = setup(N_el_x, N_el_y, N_test_x, N_test_y, N_quad, N_bound, N_residual)
    flux = None
    if neumann_sides:
        s, flux = split_neumann(s, neumann_sides)
    loss_his = []
    model = build_model(s, Net_layer, var_form, init_params, backend, loss_his, scheme=scheme)
    if flux is not None:
        model.set_flux_data(flux["X"], flux["g"], a=0.0, b=flux["b"], weight=flux_weight)
    curve = None
    if validate_every:
        model.set_validation()                                   # the test grid of P2:418-426, uploaded once
        curve = model.train_validated(n_iter, validate_every)
        loss_his.append(float(model.loss()[0]))
        if verbose:
            for it, l2, mx in zip(*curve):
                print("It: %d, rel L2 error: %.3e, max error: %.3e" % (it, l2, mx))
    elif adapt_every:
        rounds = model.train_adaptive(n_iter, adapt_every, f_ext, max_elements)
        if verbose:
            for it, ne, loss in rounds:
                print("It: %d, adapted to %d elements, loss on the new mesh: %.3e" % (it, ne, loss))
    else:
        model.train(n_iter, record_every=record_every)           # P2:434
    from . import lbfgs_stage
    stage = lbfgs_stage(model, lbfgs, lambda: np.linalg.norm(s["u_test"] - model.predict(), 2) / np.linalg.norm(s["u_test"], 2), verbose=verbose)
    u_pred = model.predict()                                     # P2:435
    err = np.linalg.norm(s["u_test"] - u_pred, 2) / np.linalg.norm(s["u_test"], 2)
    if verbose:
        print("relative L2 error of u: %.3e   final loss: %.3e" % (err, loss_his[-1]))
    out = dict(model=model, u_pred=u_pred, rel_l2=err, loss_his=loss_his, setup=s)
    if curve is not None:
        out["error_curve"] = curve
    if stage is not None:
        out["lbfgs"] = stage
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10001)
    ap.add_argument("--elements", type=int, default=4)
    ap.add_argument("--var-form", type=int, default=1)
    ap.add_argument("--width", type=int, default=5)
    ap.add_argument("--record-every", type=int, default=1)
    ap.add_argument("--validate-every", type=int, default=None,
                    help="print the error on the test grid after every K-th update (device-side validation history)")
    ap.add_argument("--adapt-every", type=int, default=None, help="one local hp-refinement round after every K-th update")
    ap.add_argument("--max-elements", type=int, default=None, help="never refine beyond this many elements")
    ap.add_argument("--lbfgs", type=int, default=0, help="L-BFGS iterations after the Adam iterations")
    ap.add_argument("--neumann-sides", default=None,
                    help="comma list out of left,right,bottom,top: sides that prescribe the flux n . grad u instead of u")
    a = ap.parse_args()
    run(n_iter=a.iters, N_el_x=a.elements, N_el_y=a.elements, var_form=a.var_form,
        Net_layer=[2] + [a.width] * 3 + [1], record_every=a.record_every, validate_every=a.validate_every,
        adapt_every=a.adapt_every, max_elements=a.max_elements, neumann_sides=a.neumann_sides, lbfgs=a.lbfgs)
