"""Expected values of the device-side validation (hpv_eval_points / hpv_residual_points / hpv_validate): the channel list, the
strong residual and the six norm numbers from the oracle classes' own net_u / net_du / net_dxu / net_dyu / net_dtu / net_f (torch
autograd, fp64) and numpy.  A plain helper module like cases.py and pinn_reference.py; no GPU needed.
tests/test_validation_host.py checks it against central finite differences of `neural_net`.

The oracle classes are created WITHOUT their problem data (quadrature, grids, right-hand sides): the methods used here read the
network alone -- layers, parameters, activation (and V for the AdvDiff residual)."""
import numpy as np
import torch

from oracle import vpinn_oracle as O

NAMES = {"p1": ("u", "u_x", "u_xx"), "p2": ("u", "u_x", "u_y", "u_xx", "u_yy"), "adv": ("u", "u_x", "u_t", "u_xx", "u_tt")}
_CLS = {"p1": O.OracleVPINN1D, "p2": O.OracleVPINN2D, "adv": O.OracleVPINNAdvDiff}


def bare_oracle(prob, layers, theta):
    """the oracle class of the problem holding a network only"""
    o = object.__new__(_CLS[prob])
    o._init_common([int(v) for v in layers], np.asarray(theta, dtype=np.float64), 0.001)
    return o


def _cols(X):
    X = np.asarray(X, dtype=np.float64)
    return [torch.tensor(X[:, c:c + 1].copy(), requires_grad=True) for c in range(X.shape[1])]


def _np(t):
    return t.detach().numpy().copy()


def channels(prob, layers, theta, X):
    """{name: (n, 1) array} in the order of NAMES[prob]"""
    o = bare_oracle(prob, layers, theta)
    c = _cols(X)
    if prob == "p1":
        d1, d2 = o.net_du(c[0])
        out = (o.net_u(c[0]), d1, d2)
    elif prob == "p2":
        (dx, dxx), (dy, dyy) = o.net_dxu(*c), o.net_dyu(*c)
        out = (o.net_u(*c), dx, dy, dxx, dyy)
    else:
        dx, dxx = o.net_dxu(*c)
        dt = o.net_dtu(*c)
        out = (o.net_u(*c), dx, dt, dxx, o._grad(dt, c[1]))
    return {k: _np(v) for k, v in zip(NAMES[prob], out)}


def residual(prob, layers, theta, X, f=None, V=1.0):
    """(n, 1): -u_xx - f (P1:150-155), u_xx + u_yy - f (net_f, P2:187-194), u_t + V u_x - epsilon u_xx - f (P3:247-253)"""
    o = bare_oracle(prob, layers, theta)
    c = _cols(X)
    f = 0.0 if f is None else np.asarray(f, dtype=np.float64).reshape(-1, 1)
    if prob == "p1":
        return -_np(o.net_du(c[0])[1]) - f
    if prob == "p2":
        return _np(o.net_f(*c)) - f
    dx, dxx = o.net_dxu(*c)
    eps = float(o.epsilon.detach()[0])
    return _np(o.net_dtu(*c)) + V * _np(dx) - eps * _np(dxx) - f


def norms(u_hat, u, du_hat=None, du=None):
    """{sum (u^-u)^2, sum u^2, max |u^-u|, sum |grad u^ - grad u|^2, sum |grad u|^2, n} (numpy, fp64)"""
    u_hat, u = np.asarray(u_hat, dtype=np.float64).reshape(-1), np.asarray(u, dtype=np.float64).reshape(-1)
    e = u_hat - u
    out = [float(np.sum(e * e)), float(np.sum(u * u)), float(np.max(np.abs(e))), 0.0, 0.0, float(u.size)]
    if du is not None:
        g = np.asarray(du_hat, dtype=np.float64) - np.asarray(du, dtype=np.float64)
        out[3], out[4] = float(np.sum(g * g)), float(np.sum(np.asarray(du, dtype=np.float64) ** 2))
    return np.array(out)
