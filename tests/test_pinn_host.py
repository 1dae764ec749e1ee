"""Host-side checks of the strong-form PINN scheme for Poisson-1D and AdvDiff: the expected-value helper itself
(tests/pinn_reference.py) against finite differences, the sign of net_f against reference-produced data, the AdvDiff residual on
a manufactured solution, and the constructor errors that are raised before any library call.  No GPU."""
import types

import numpy as np
import pytest
import torch

from cases import gold, p1_args, p3_args, rel, theta0
from pinn_reference import PinnRef1D, PinnRefAdvDiff, residual_1d, residual_advdiff


def _fd_grad(ref, h=1e-5):
    th0 = ref.get_params()
    g = np.empty_like(th0)
    for i in range(th0.size):
        vals = []
        for s in (1.0, -1.0):
            th = th0.copy()
            th[i] += s * h
            ref.theta = torch.tensor(th, requires_grad=True)
            vals.append(float(ref.loss_parts()[0].detach()))
        g[i] = (vals[0] - vals[1]) / (2 * h)
    ref.theta = torch.tensor(th0, requires_grad=True)
    return g


# Central differences with step h on a smooth fp64 loss: truncation ~ h^2 |f'''| / 6 ~ 1e-10, rounding ~ 1e-16 |f| / h ~ 1e-11
# per entry, against gradient norms of order 1 and more -- 1e-6 relative leaves three orders to both.
FD_TOL = 1e-6


def test_helper_gradient_equals_finite_differences_1d():
    rng = np.random.default_rng(3)
    layers = [1, 7, 5, 1]
    x = rng.uniform(-1, 1, (9, 1))
    th = theta0(layers, 21)
    th[7:14] = 0.1 * np.arange(7)         # non-zero first bias
    ref = PinnRef1D(np.array([[-1.0], [1.0]]), np.array([[0.3], [-0.2]]), x, np.sin(3 * x) + 0.5, layers, lossb_weight=3,
                    init_params=th)
    _, g = ref.loss_and_grad()
    assert rel(_fd_grad(ref), g) < FD_TOL


def test_helper_gradient_equals_finite_differences_advdiff_with_epsilon():
    rng = np.random.default_rng(4)
    layers = [2, 6, 4, 1]
    xt = np.stack([rng.uniform(-1, 1, 11), rng.uniform(0, 1, 11)], 1)
    xb = np.stack([rng.uniform(-1, 1, 5), np.zeros(5)], 1)
    th = theta0(layers, 22, extra=[0.4])
    ref = PinnRefAdvDiff(xb, -np.sin(np.pi * xb[:, :1]), xt, layers, V=0.7, init_params=th)
    _, g = ref.loss_and_grad()
    fd = _fd_grad(ref)
    assert rel(fd[:-1], g[:-1]) < FD_TOL
    assert abs(g[-1]) > 1e-3 and abs(fd[-1] - g[-1]) < FD_TOL * abs(g[-1])      # d loss / d epsilon on its own


def test_f_train_of_the_reference_fixture_is_minus_u_xx():
    """The sign of net_f (P1:150-155: -u_xx against f_train): `f_train` of the reference-generated fixture equals -u'' of the
    driver's exact solution at X_f_train, i.e. the 1-D strong-form residual of the exact solution vanishes."""
    from hp_vpinns_amd.drivers import poisson1d
    g = gold("poisson1d_small")
    x, f = torch.tensor(g["X_f_train"]), torch.tensor(g["f_train"])
    u = lambda z: poisson1d.amp * (0.1 * torch.sin(poisson1d.omega * z) + torch.tanh(poisson1d.r1 * z))    # noqa: E731  (P1:248-250)
    r = residual_1d(u, x, f).detach().numpy()
    # fp64 autograd of tanh(80 x): |f| reaches 2 r1^2 ~ 1e4, its rounding error ~ 1e-12 relative
    assert np.abs(r).max() < 1e-9 * np.abs(g["f_train"]).max()
    assert np.abs(g["f_train"]).max() > 1e3      # (the wrong sign would miss by twice that)


@pytest.mark.parametrize("V,eps,k", [(1.0, 0.1 / np.pi, np.pi), (0.7, 0.25, 2.0)])
def test_advdiff_residual_vanishes_on_a_manufactured_solution(V, eps, k):
    rng = np.random.default_rng(5)
    x, t = torch.tensor(rng.uniform(-1, 1, (40, 1))), torch.tensor(rng.uniform(0, 1, (40, 1)))
    u = lambda x, t: torch.exp(-eps * k * k * t) * torch.sin(k * (x - V * t))      # noqa: E731
    r = residual_advdiff(u, x, t, V, eps).detach().numpy()
    assert np.abs(r).max() < 1e-13 * k * k      # every term is O(k^2) at most
    # and each term matters: another V or epsilon leaves a residual of the size of that term
    assert np.abs(residual_advdiff(u, x, t, V + 0.1, eps).detach().numpy()).max() > 1e-2
    assert np.abs(residual_advdiff(u, x, t, V, eps + 0.1).detach().numpy()).max() > 1e-2


def test_scheme_argument_errors_are_raised_before_any_library_call(monkeypatch):
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.vpinn import VPINN1D, VPINNAdvDiff

    def no_library(*a, **k):
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    a1 = p1_args(gold("poisson1d_small"))
    a3 = p3_args(gold("advdiff_small"))
    with pytest.raises(ValueError, match="scheme"):
        VPINN1D(*a1, scheme="pinns")
    with pytest.raises(ValueError, match="collocation"):
        VPINN1D(*a1[:9], scheme="PINNs")
    with pytest.raises(ValueError, match="f_train"):
        VPINN1D(*a1[:10], scheme="PINNs")
    with pytest.raises(ValueError, match="scheme"):
        VPINNAdvDiff(*a3, scheme="strong")
    with pytest.raises(ValueError, match="collocation"):
        VPINNAdvDiff(*a3[:2], None, *a3[3:], scheme="PINNs")
    # the switch is a keyword of its own: a module global `scheme` (what P2 reads, P2:279) does not reach these two classes
    with pytest.raises(AssertionError, match="library was reached"):
        VPINN1D(*a1, module_globals={"scheme": "no such scheme"})


def test_collocation_shard_with_fewer_points_than_ranks():
    from hp_vpinns_amd.vpinn import _VPINNBase
    stub = types.SimpleNamespace(world=4, rank=1, h=None)
    with pytest.raises(ValueError, match="fewer collocation points than ranks"):
        _VPINNBase._set_collocation_shard(stub, np.zeros((3, 2)), None)
