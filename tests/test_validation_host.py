"""tests/validation_reference.py (the expected values of the device-side validation tests) against central finite differences of
the oracle's `neural_net`, on the CPU: a [2, 5, 5, 1] tanh network (Poisson-2D and AdvDiff naming) and a [1, 5, 1] sin network
(Poisson-1D) at 10 seeded points inside the domain, every weight and bias generic (generic_point.generic_theta).

Step size and bound.  With fp64 unit round-off eps = 2^-53 and |u| <= U near the point,
    (u(x+h) - u(x-h)) / 2h         = u_x  + h^2 u_xxx(xi) / 6   + rounding <= eps U / h
    (u(x+h) - 2u(x) + u(x-h)) / h^2 = u_xx + h^2 u_xxxx(xi) / 12 + rounding <= 4 eps U / h^2
so at h = 1e-3 the truncation terms are 1.7e-7 M3 and 8.3e-8 M4 and the rounding terms 1.1e-13 U and 4.4e-10 U.  M3, M4 are the largest
third / fourth derivatives along the coordinate at the ten points (autograd of `neural_net` itself), doubled: across [x-h, x+h] a
derivative of these networks moves by O(h) of itself, far inside the factor two.  U is the largest |u| at the points, doubled
likewise, and the network's own evaluation error (a few eps U per value) is covered by doubling the rounding terms.  Bounds:
    first derivatives   h^2 M3 / 6  + 2 eps U / h
    second derivatives  h^2 M4 / 12 + 8 eps U / h^2
The residuals and the norms are checked against their definitions on the finite-difference channels with the same bounds
propagated (the residual is a fixed linear combination of the channels)."""
import numpy as np
import pytest
import torch

import generic_point as gp
import validation_reference as vr

H = 1e-3
EPS = 2.0 ** -53
N = 10


def _points(prob, seed):
    rng = np.random.default_rng(seed)
    if prob == "p1":
        return rng.uniform(-0.95, 0.95, (N, 1))
    lo, hi = (np.array([-0.95, 0.05]), np.array([0.95, 0.95])) if prob == "adv" else (np.array([-0.95, -0.95]), np.array([0.95, 0.95]))
    return lo + (hi - lo) * rng.uniform(size=(N, 2))


def _case(prob):
    layers = [1, 5, 1] if prob == "p1" else [2, 5, 5, 1]
    th = gp.generic_theta(layers, 4100 + len(prob), extra=[0.8] if prob == "adv" else ())
    return layers, th, _points(prob, 4200 + len(prob))


def _u(o, X):
    with torch.no_grad():
        return o.neural_net(torch.tensor(X)).numpy().reshape(-1)


def _high_derivatives(o, X, c):
    """(max |d^3 u / dx_c^3|, max |d^4 u / dx_c^4|) at the points"""
    x = torch.tensor(X, requires_grad=True)
    d = o.neural_net(x)
    out = []
    for k in range(4):
        d = torch.autograd.grad(d.sum(), x, create_graph=True)[0][:, c:c + 1]
        out.append(float(d.detach().abs().max()))
    return out[2], out[3]


def _fd(o, X, c):
    e = np.zeros(X.shape[1]); e[c] = H
    up, u0, um = _u(o, X + e), _u(o, X), _u(o, X - e)
    return (up - um) / (2 * H), (up - 2 * u0 + um) / H ** 2


def _bounds(o, X, c):
    U = 2.0 * np.abs(_u(o, X)).max()
    m3, m4 = (2.0 * v for v in _high_derivatives(o, X, c))
    return H ** 2 * m3 / 6 + 2 * EPS * U / H, H ** 2 * m4 / 12 + 8 * EPS * U / H ** 2


@pytest.mark.parametrize("prob", ["p1", "p2", "adv"])
def test_channels_against_central_differences(prob):
    layers, th, X = _case(prob)
    o = vr.bare_oracle(prob, layers, th)
    ch = vr.channels(prob, layers, th, X)
    names = vr.NAMES[prob]
    assert tuple(ch) == names and all(v.shape == (N, 1) for v in ch.values())
    assert np.array_equal(ch["u"].reshape(-1), _u(o, X))
    d = X.shape[1]
    for c in range(d):
        b1, b2 = _bounds(o, X, c)
        f1, f2 = _fd(o, X, c)
        e1 = np.abs(ch[names[1 + c]].reshape(-1) - f1).max()
        e2 = np.abs(ch[names[1 + d + c]].reshape(-1) - f2).max()
        print("%s coordinate %d: first %.2e (bound %.2e), second %.2e (bound %.2e)" % (prob, c, e1, b1, e2, b2))
        assert b1 < 1e-4 and b2 < 1e-4          # (the bounds themselves say something: the derivatives are O(1))
        assert e1 <= b1, (prob, c, e1, b1)
        assert e2 <= b2, (prob, c, e2, b2)


@pytest.mark.parametrize("prob", ["p1", "p2", "adv"])
def test_residual_against_central_differences(prob):
    layers, th, X = _case(prob)
    o = vr.bare_oracle(prob, layers, th)
    f = np.random.default_rng(5).standard_normal((N, 1))
    V = 0.6
    d = X.shape[1]
    fd = [_fd(o, X, c) for c in range(d)]
    bd = [_bounds(o, X, c) for c in range(d)]
    if prob == "p1":
        want, bound = -fd[0][1], bd[0][1]
    elif prob == "p2":
        want, bound = fd[0][1] + fd[1][1], bd[0][1] + bd[1][1]
    else:
        eps = th[-1]
        want, bound = fd[1][0] + V * fd[0][0] - eps * fd[0][1], bd[1][0] + V * bd[0][0] + abs(eps) * bd[0][1]
    for ff in (f, None):
        got = vr.residual(prob, layers, th, X, ff, V=V)
        assert got.shape == (N, 1)
        err = np.abs(got.reshape(-1) - (want - (0.0 if ff is None else ff.reshape(-1)))).max()
        print("%s residual (f %s): %.2e (bound %.2e)" % (prob, "given" if ff is not None else "None", err, bound))
        assert err <= bound, (prob, err, bound)


def test_norms_are_the_definitions():
    rng = np.random.default_rng(11)
    uh, u = rng.standard_normal(37), rng.standard_normal(37)
    dh, du = rng.standard_normal((37, 2)), rng.standard_normal((37, 2))
    r = vr.norms(uh, u, dh, du)
    assert r[5] == 37 and r[2] == max(abs(a - b) for a, b in zip(uh, u))
    assert abs(r[0] - sum((a - b) ** 2 for a, b in zip(uh, u))) < 1e-12 * r[0]
    assert abs(r[1] - sum(b * b for b in u)) < 1e-12 * r[1]
    assert abs(r[3] - sum(((a - b) ** 2).sum() for a, b in zip(dh, du))) < 1e-12 * r[3]
    assert abs(r[4] - (du ** 2).sum()) < 1e-12 * r[4]
    r0 = vr.norms(uh[:, None], u[:, None])
    assert np.array_equal(r0[:3], r[:3]) and r0[3] == 0.0 and r0[4] == 0.0
