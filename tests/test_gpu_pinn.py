"""scheme='PINNs' on Poisson-1D and AdvDiff (trainable epsilon) against tests/pinn_reference.py, the torch-fp64 restatement of
the strong-form losses; collocation counts around the tile, block and grid limits of k_pinn_residual; shards; drivers; and the
Poisson-2D branch bit for bit against a result recorded with the library as it was before the kernel took the problem as a
parameter.  Tolerances are those of tests/test_gpu_parity.py."""
import os

import numpy as np
import pytest

from cases import GOLD, gold, p1_args, p2_args, p3_args, rel, theta0
from pinn_reference import PinnRef1D, PinnRefAdvDiff

pytestmark = pytest.mark.gpu

TOL = 1e-9
TRAJ_TOL = 1e-7

GENERIC_1D, MFMA_1D = [1, 7, 5, 1], [1, 20, 20, 20, 1]
GENERIC_ADV, MFMA_ADV = [2, 6, 9, 4, 1], [2, 20, 20, 20, 1]


def _theta(layers, seed, extra=()):
    th = theta0(layers, seed, extra=extra)
    w = layers[0] * layers[1]
    th[w:w + layers[1]] = 0.1 * np.arange(layers[1]) - 0.3      # non-zero first bias
    return th


def _pair_1d(layers, backend, X_f=None, f=None, lossb_weight=3):
    from hp_vpinns_amd.vpinn import VPINN1D
    a = list(p1_args(gold("poisson1d_small"), layers))
    if X_f is not None:
        a[9], a[10] = X_f, f
    th = _theta(layers, 31)
    o = PinnRef1D(a[0], a[1], a[9], a[10], layers, lossb_weight=lossb_weight, init_params=th)
    m = VPINN1D(*a, scheme="PINNs", lossb_weight=lossb_weight, LR=0.001, init_params=th, backend=backend)
    return o, m


def _pair_adv(layers, backend, V=1.0, eps0=0.6, XT_f=None):
    from hp_vpinns_amd.vpinn import VPINNAdvDiff
    a = list(p3_args(gold("advdiff_small"), layers))
    if XT_f is not None:
        a[2] = XT_f
    th = _theta(layers, 32, extra=[eps0])
    o = PinnRefAdvDiff(a[0], a[1], a[2], layers, V=V, init_params=th)
    m = VPINNAdvDiff(*a, scheme="PINNs", V=V, LR=0.001, init_params=th, backend=backend)
    return o, m


def _check_loss_grad(o, m, n_eps=0):
    l3o, go = o.loss_and_grad()
    l3m, gm = m.loss_and_grad()
    print("loss3", l3m, l3o, "grad rel", rel(gm[:gm.size - n_eps], go[:go.size - n_eps]), "d eps", gm[-1], go[-1])
    assert rel(l3m, l3o) < TOL, (l3m, l3o)
    assert rel(gm[:gm.size - n_eps], go[:go.size - n_eps]) < TOL
    if n_eps:      # the epsilon entry on its own: next to thousands of weights its error would vanish in the norm
        assert abs(go[-1]) > 0 and abs(gm[-1] - go[-1]) < TOL * abs(go[-1]), (gm[-1], go[-1])
    assert rel(m.loss(), l3o) < TOL      # forward-only evaluation


def _check_traj(o, m, n=8, n_eps=0):
    lo, lm = [], []
    for _ in range(n):
        o.adam_step()
        lo.append(float(o.loss_parts()[0]))
        lm.append(float(m._step(1, True)[0]))
    print("trajectory rel", rel(lm, lo), "params rel", rel(m.get_params(), o.get_params()))
    assert rel(lm, lo) < TRAJ_TOL, (lm, lo)
    assert rel(m.get_params(), o.get_params()) < TRAJ_TOL
    if n_eps:
        eo, em = o.get_params()[-1], m.get_params()[-1]
        print("epsilon", em, eo)
        assert abs(em - eo) < TRAJ_TOL * abs(eo) and em == float(m.epsilon[0])


@pytest.mark.parametrize("backend,layers", [("generic", GENERIC_1D), ("mfma", MFMA_1D)])
def test_poisson1d_pinn_scheme(backend, layers):
    """loss = lossb_weight * lossb + mean((-u_xx - f_train)^2) at the fixture's 500 collocation points."""
    o, m = _pair_1d(layers, backend)
    _check_loss_grad(o, m)
    _check_traj(o, m)
    assert m.backend() == backend


@pytest.mark.parametrize("V", [1.0, 0.7])
@pytest.mark.parametrize("backend,layers", [("generic", GENERIC_ADV), ("mfma", MFMA_ADV)])
def test_advdiff_pinn_scheme_with_trainable_epsilon(backend, layers, V):
    """loss = 10 lossb + mean((u_t + V u_x - epsilon u_xx)^2); epsilon starts at 0.6 and is trained with the weights."""
    o, m = _pair_adv(layers, backend, V=V)
    _check_loss_grad(o, m, n_eps=1)
    _check_traj(o, m, n_eps=1)
    assert m.backend() == backend


def _points(dim, n):
    """n collocation points: a subset of the fixture's while it has that many, Latin-hypercube points beyond."""
    from hp_vpinns_amd.sampling import lhs
    X = gold("poisson1d_small")["X_f_train"] if dim == 1 else gold("advdiff_small")["XT_f_train"]
    if n <= X.shape[0]:
        return X[:n].copy()
    np.random.seed(99)
    H = lhs(dim, n)
    return 2 * H - 1 if dim == 1 else np.hstack((2 * H[:, :1] - 1, H[:, 1:]))


# the tile tail of the reverse kernels (1, 15, 16, 17), two blocks of the residual kernel (257), its grid-stride loop past the
# 64-block cap (16 385 > 64 * 256)
COUNTS = [1, 15, 16, 17, 257, 16385]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("backend", ["mfma", "generic"])
def test_poisson1d_collocation_counts(backend, n):
    from hp_vpinns_amd.drivers.poisson1d import f_ext
    X = _points(1, n)
    o, m = _pair_1d(MFMA_1D if backend == "mfma" else GENERIC_1D, backend, X, f_ext(X))
    _check_loss_grad(o, m)
    assert m.backend() == backend


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("backend", ["mfma", "generic"])
def test_advdiff_collocation_counts(backend, n):
    o, m = _pair_adv(MFMA_ADV if backend == "mfma" else GENERIC_ADV, backend, V=0.7, XT_f=_points(2, n))
    _check_loss_grad(o, m, n_eps=1)
    assert m.backend() == backend


@pytest.mark.parametrize("n", [15, 17])
@pytest.mark.parametrize("backend", ["mfma", "generic"])
def test_no_stale_adjoints_after_a_larger_collocation_set(backend, n):
    """A reverse pass over 257 points first, then n points through the SAME handle: nothing the first pass left behind (adjoint
    rows, partial sums of the second block) may reach the second result."""
    from hp_vpinns_amd.drivers.poisson1d import f_ext
    X1 = _points(1, n)
    o, m = _pair_1d(MFMA_1D if backend == "mfma" else GENERIC_1D, backend, X1, f_ext(X1))
    big = _points(1, 257)[::-1].copy()
    m.h.set_collocation(big, 50.0 * f_ext(big))
    m.h.loss_and_grad(True)
    m.h.set_collocation(X1, f_ext(X1))
    _check_loss_grad(o, m)
    X2 = _points(2, n)
    o, m = _pair_adv(MFMA_ADV if backend == "mfma" else GENERIC_ADV, backend, V=0.7, XT_f=X2)
    m.h.set_collocation(_points(2, 257)[::-1].copy(), None)
    m.h.loss_and_grad(True)
    m.h.set_collocation(X2, None)
    _check_loss_grad(o, m, n_eps=1)


@pytest.mark.parametrize("problem", ["poisson1d", "advdiff"])
def test_collocation_shards_add_up(problem):
    """Two handles own the two halves of the collocation points (n_total = all of them), only the first has the boundary
    points: their packed losses and gradients, epsilon's included, add up to the single-handle values."""
    from hp_vpinns_amd import _lib
    if problem == "poisson1d":
        g = gold("poisson1d_small")
        X, f, Xd, ud, layers = g["X_f_train"], g["f_train"].reshape(-1), g["X_u_train"], g["u_train"].reshape(-1), MFMA_1D
        th = _theta(layers, 41)
        make = lambda: _lib.Handle(_lib.PDE_POISSON1D, 1, _lib.ACT_SIN, layers, lossb_weight=3, scheme=_lib.SCHEME_PINN)   # noqa: E731
    else:
        g = gold("advdiff_small")
        X, f, Xd, ud, layers = g["XT_f_train"], None, g["XT_u_train"], g["u_train"].reshape(-1), MFMA_ADV
        th = _theta(layers, 42, extra=[0.6])
        make = lambda: _lib.Handle(_lib.PDE_ADVDIFF, 0, _lib.ACT_TANH, layers, lossb_weight=10, V=0.7, scheme=_lib.SCHEME_PINN)   # noqa: E731

    def run(lo, hi, with_data, ff=f):
        h = make()
        h.set_collocation(X[lo:hi], None if ff is None else ff[lo:hi], n_total=X.shape[0])
        if with_data:
            h.set_data(Xd, ud)
        h.set_params(th)
        return h.loss_and_grad(True)
    n, half = X.shape[0], X.shape[0] // 2 + 3      # (253 and 247 points: neither a multiple of the tile)
    l3, gr = run(0, n, True)
    l3a, ga = run(0, half, True)
    l3b, gb = run(half, n, False)
    assert l3b[1] == 0.0 and abs(l3[2]) > 0
    assert np.abs(l3a + l3b - l3).max() < 1e-12 * abs(l3[0])
    assert np.abs(ga + gb - gr).max() < 1e-12 * np.abs(gr).max()
    assert abs(gr[-1]) > 0 and abs(ga[-1] + gb[-1] - gr[-1]) < 1e-12 * abs(gr[-1])
    if problem == "advdiff":      # no right-hand side is a zero right-hand side
        l3z, gz = run(0, n, True, ff=np.zeros(n))
        assert np.array_equal(l3z, l3) and np.array_equal(gz, gr)
    else:                         # ... which only AdvDiff has
        with pytest.raises(_lib.HpvError):
            make().set_collocation(X, None)


def test_drivers_train_on_the_strong_form():
    """poisson1d.run / advdiff.run with scheme='PINNs': the records keep their documented shape ([it, loss] every 10 iterations;
    [it, loss, epsilon, 1]) and lossp falls from its initial value."""
    from hp_vpinns_amd.drivers import advdiff, poisson1d
    from hp_vpinns_amd.vpinn import VPINN1D
    r = poisson1d.run(scheme="PINNs", Opt_Niter=41, verbose=False)
    rec = np.array(r["total_record"])
    assert rec.shape == (5, 2) and list(rec[:, 0]) == [0, 10, 20, 30, 40] and r["model"].scheme == "PINNs"
    s = r["setup"]
    m0 = VPINN1D(s["X_u_train"], s["u_train"], s["X_quad_train"], s["W_quad_train"], s["F_ext_total"], s["grid"], s["X_test"],
                 s["u_test"], r["model"].layers, s["X_f_train"], s["f_train"], var_form=1, lossb_weight=1, LR=0.001, scheme="PINNs")
    l0, l1 = m0.loss(), r["model"].loss()
    print("poisson1d lossp", l0[2], "->", l1[2])
    assert l1[2] < l0[2] and abs(l1[0] - (l1[1] + l1[2])) < 1e-12 * l1[0] and rec[-1, 1] == l1[0]

    r = advdiff.run(scheme="PINNs", Opt_Niter=61, verbose=False)
    rec = r["total_record"]
    assert [int(v[0]) for v in rec] == [0, 10, 20, 30, 40, 50, 60] and all(len(v) == 4 and v[3] == 1 for v in rec)
    eps = [float(np.ravel(v[2])[0]) for v in rec]
    assert eps[-1] != 1.0 and eps[-1] == r["epsilon"] and r["model"].scheme == "PINNs"
    m0 = advdiff.build_model(r["setup"], r["model"].layers, scheme="PINNs")
    l0, l1 = m0.loss(), r["model"].loss()
    print("advdiff lossp", l0[2], "->", l1[2], "epsilon", eps)
    assert l1[2] < l0[2] and abs(l1[0] - (l1[1] + l1[2])) < 1e-12 * l1[0] and float(rec[-1][1]) == l1[0]


@pytest.mark.parametrize("backend", ["generic", "mfma"])
def test_poisson2d_pinn_scheme_is_bit_identical_to_the_recorded_result(backend):
    """The Poisson-2D strong-form loss and gradient, bit for bit, against tests/golden/pinn2d_recorded.npz -- written by
    scripts/record_pinn2d.py with the library of the commit before k_pinn_residual took the problem as a parameter (that script
    builds the same two models as this test and stores what they return)."""
    from hp_vpinns_amd.vpinn import VPINN2D
    rec = np.load(os.path.join(GOLD, "pinn2d_recorded.npz"), allow_pickle=False)
    layers = [int(v) for v in rec["layers_" + backend]]
    a = p2_args(gold("poisson2d_default"), layers)
    m = VPINN2D(*a, scheme="PINNs", init_params=theta0(layers, 44), backend=backend)
    l3, g = m.loss_and_grad()
    assert m.backend() == backend
    assert np.array_equal(l3, rec["loss3_" + backend]) and np.array_equal(g, rec["grad_" + backend])
    assert np.array_equal(m._step(3, True), rec["loss3_after3_" + backend])
