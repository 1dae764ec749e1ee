"""The L-BFGS stage on the GPU: k_lbfgs_direction and k_lbfgs_push through the hooks of libhpvpinn_testhooks.so against the numpy
two-loop recursion, hpv_lbfgs_step end to end against torch.optim.LBFGS driven by a second handle of the same model, and the
properties that hold by construction.  The figures behind DIR_TOL and E2E_TOL: profiles/lbfgs.md."""
import ctypes as C

import numpy as np
import pytest

import lbfgs_reference as lr
from cases import gold, p1_args, p3_args, rel, theta0

pytestmark = pytest.mark.gpu

# k_lbfgs_direction against two_loop (math.fsum dots): the largest relative difference max|d - d_ref| / max|d_ref| measured over the
# twelve cases below was 2.2e-16; ten times that (reduction order only, everything fp64)
DIR_TOL = 2.2e-15
# hpv_lbfgs_step against torch after six iterations: the largest relative difference of the final parameters, measured over the six
# problems below at three seeds each (11, 12, 13), was 5.0e-13; a hundred times that (never looser than 1e-6)
E2E_TOL = 5.0e-11


# ---- the kernels through the hooks -------------------------------------------------------------------------------------------------
def _hooks():
    from hp_vpinns_amd import _lib
    with _lib.library(_lib.TEST_HOOKS_LIB_PATH) as lib:
        return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _direction(P, m, head, n_hist, S, Y, rho, h_diag, g):
    d, scal = np.empty(P), np.empty(4)
    rc = _hooks().hpv_test_lbfgs_direction(P, m, head, n_hist, _dp(S), _dp(Y), _dp(rho), float(h_diag), _dp(g), _dp(d), _dp(scal))
    assert rc == 0
    return d, scal


def _ring_case(P, m, head, n_hist, seed):
    """S, Y [m][P] with the live pairs at head, head + 1, .. (mod m) (y = A s for a diagonal SPD A: y . s > 0) and garbage in the
    dead slots; the pairs oldest first for the reference."""
    rng = np.random.default_rng(seed)
    a = 0.5 + rng.random(P)
    S, Y = rng.standard_normal((m, P)), 1e30 * rng.standard_normal((m, P))
    slots = [(head + k) % m for k in range(n_hist)]
    for s in slots:
        Y[s] = a * S[s] + 0.05 * rng.standard_normal(P) * np.abs(S[s])
    So, Yo = S[slots], Y[slots]
    rho_o, h_diag = lr.pair_scalars(So, Yo)
    rho = np.full(m, np.nan)
    rho[slots] = rho_o
    return S, Y, rho, h_diag, So, Yo, rho_o, rng.standard_normal(P)


M_RING = 5
DIR_CASES = [(P, n, head) for P in (16, 921, 4417) for n, head in ((0, 2), (1, 4), (3, 3), (M_RING, 2))]      # (3, 3): slots 3, 4, 0


@pytest.mark.parametrize("P,n_hist,head", DIR_CASES)
def test_direction_kernel_against_the_two_loop_recursion(P, n_hist, head):
    S, Y, rho, h_diag, So, Yo, rho_o, g = _ring_case(P, M_RING, head, n_hist, 1000 + P + n_hist)
    d1, s1 = _direction(P, M_RING, head, n_hist, S, Y, rho, h_diag, g)
    d2, s2 = _direction(P, M_RING, head, n_hist, S, Y, rho, h_diag, g)
    assert np.array_equal(d1, d2) and np.array_equal(s1, s2)                    # bitwise, call to call
    ref = lr.two_loop(So, Yo, g, rho_o, h_diag)
    err = float(np.abs(d1 - ref).max() / np.abs(ref).max())
    gtd = float(np.dot(g, ref))
    print("direction P=%d n_hist=%d head=%d: rel err %.3e, gtd %.6e (ref %.6e)" % (P, n_hist, head, err, s1[0], gtd))
    assert err <= DIR_TOL
    assert abs(s1[0] - gtd) <= DIR_TOL * float(np.abs(g * ref).sum()) * 10      # (a dot product: relative to the sum of its terms' sizes)
    assert s1[1] == np.abs(g).max() and s1[3] == np.abs(d1).max() and abs(s1[2] - np.abs(g).sum()) <= 1e-14 * np.abs(g).sum()
    if n_hist == 0:
        assert np.array_equal(d1, -g)


def _push(P, m, ring, S, Y, rho, h_diag, t, d, g_new, g, theta, theta0_):
    ring3 = (C.c_int * 3)(*ring)
    hd = np.array([h_diag])
    rc = _hooks().hpv_test_lbfgs_push(P, m, ring3, _dp(S), _dp(Y), _dp(rho), _dp(hd), float(t), _dp(d), _dp(g_new), _dp(g), _dp(theta), _dp(theta0_))
    assert rc == 0
    return list(ring3), float(hd[0])


@pytest.mark.parametrize("P", [16, 921])
def test_push_applies_the_curvature_test(P):
    """y . s <= 1e-10: the pair is skipped, the counter rises, rings and H_diag stay; just above: stored at the ring's end.  Either
    way g = g_new and theta0 = theta afterwards, and d is read only."""
    rng = np.random.default_rng(5 + P)
    m, t = 4, 0.5
    d = rng.standard_normal(P)
    g = rng.standard_normal(P)
    theta, th0 = rng.standard_normal(P), rng.standard_normal(P)
    s = d * t
    for ys_target, stored in ((0.5e-10, False), (-1.0, False), (2.0e-10, True), (3.0, True)):
        y = ys_target * s / float(s @ s)                 # y . s = ys_target up to rounding (far from the threshold)
        g_new = g + y
        S, Y = rng.standard_normal((m, P)), rng.standard_normal((m, P))
        rho, S0, Y0 = rng.standard_normal(m), S.copy(), Y.copy()
        rho0, gk, t0k, dk = rho.copy(), g.copy(), th0.copy(), d.copy()
        ring, hd = _push(P, m, [1, 2, 7], S, Y, rho, 0.25, t, dk, g_new, gk, theta, t0k)
        assert np.array_equal(gk, g_new) and np.array_equal(t0k, theta) and np.array_equal(dk, d)
        if not stored:
            assert ring == [1, 2, 8] and hd == 0.25 and np.array_equal(S, S0) and np.array_equal(Y, Y0) and np.array_equal(rho, rho0)
        else:
            yk = g_new - g
            assert ring == [1, 3, 7] and np.array_equal(S[3], s) and np.array_equal(Y[3], yk)
            assert abs(rho[3] * float(yk @ s) - 1.0) < 1e-12 and abs(hd - float(yk @ s) / float(yk @ yk)) < 1e-12 * hd
            keep = [0, 1, 2]
            assert np.array_equal(S[keep], S0[keep]) and np.array_equal(Y[keep], Y0[keep]) and np.array_equal(rho[keep], rho0[keep])
    # a full ring drops its oldest pair: the new one takes the head's slot and the head moves on
    S, Y, rho = rng.standard_normal((m, P)), rng.standard_normal((m, P)), rng.standard_normal(m)
    g_new = g + 3.0 * s / float(s @ s)
    ring, _ = _push(P, m, [3, 4, 0], S, Y, rho, 1.0, t, d.copy(), g_new, g.copy(), theta, th0.copy())
    assert ring == [0, 4, 0] and np.array_equal(S[3], s)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _vpinn1d(seed):
    from hp_vpinns_amd.vpinn import VPINN1D
    a = p1_args(gold("poisson1d_small"))
    return VPINN1D(*a, init_params=theta0(a[8], seed))


def _vpinn2d(seed, scheme="VPINNs"):
    from hp_vpinns_amd.drivers.poisson2d import build_model, setup
    s = setup(N_el_x=2, N_el_y=2, N_test_x=5, N_test_y=5, N_quad=10, N_bound=20, N_residual=64)
    L = [2, 20, 20, 20, 1]
    return build_model(s, L, 1, theta0(L, seed), "auto", [], scheme=scheme)


def _advdiff(seed):
    from hp_vpinns_amd.vpinn import VPINNAdvDiff
    a = p3_args(gold("advdiff_small"))
    return VPINNAdvDiff(*a, init_params=theta0(a[12], seed, extra=[0.6]))


def _linear1d(seed):
    from hp_vpinns_amd.vpinn import VPINNLinear
    return VPINNLinear([1, 5, 1], grid_x=np.linspace(0.0, 1.0, 3), n_quad=8, n_test=4, kappa=1.0, beta=0.5, sigma=-1.0,
                       f=lambda P: np.sin(3.0 * P[:, 0]), X_u_train=np.array([[0.0], [1.0]]), u_train=np.array([0.0, 0.3]), lossb_weight=5.0,
                       backend="generic", init_params=theta0([1, 5, 1], seed))


def _nonlinear_dual(seed):
    from hp_vpinns_amd.vpinn import VPINNNonlinear
    Xb = np.stack([np.linspace(-1.0, 1.0, 9), np.zeros(9)], 1)
    return VPINNNonlinear([2, 8, 8, 1], grid_x=np.linspace(-1.0, 1.0, 3), grid_y=np.linspace(0.0, 1.0, 2), n_quad=(6, 5), n_test=(4, 3),
                          kappa=1.0, sigma=0.0, cubic=0.5, f=lambda P: np.sin(P[:, 0]) * P[:, 1], X_u_train=Xb,
                          u_train=np.sin(np.pi * Xb[:, 0]), lossb_weight=3.0, trainable=[dict(name="c", init=0.7, sigma=1.0)],
                          residual_norm="dual", init_params=theta0([2, 8, 8, 1], seed, extra=[0.7]))


# problem -> (builder, seed).  The seeds are ones at which every decision of the reference's line searches -- sufficient decrease,
# curvature, sign of the directional derivative -- stands more than 1e-6 (relative) away from its threshold (asserted below): the
# two implementations then cannot take different branches over a rounding difference.  (Smallest margins measured at these seeds:
# 1.2e-5, 5.0e-5, 7.7e-4, 6.6e-4, 1.7e-2, 3.7e-3; seed 11 of the first problem came within 1.4e-6 and was not taken.)
PROBLEMS = {
    "vpinn1d": (_vpinn1d, 12), "vpinn2d": (_vpinn2d, 11), "vpinn2d_pinns": (lambda s: _vpinn2d(s, "PINNs"), 11),
    "advdiff": (_advdiff, 11), "linear1d": (_linear1d, 11), "nonlinear_dual": (_nonlinear_dual, 11),
}
E2E_OPTS = dict(max_iter=6, history=3, max_eval=40)      # (40: no search of the six is cut short by the evaluation budget)


def run_pair(name, seed=None):
    """hpv_lbfgs_step on one handle, torch.optim.LBFGS around a SECOND handle of the same model (the same function bits)."""
    build, s0 = PROBLEMS[name]
    seed = s0 if seed is None else seed
    m, m2 = build(seed), build(seed)

    def closure(th):
        m2.set_params(th)
        l3, g = m2.loss_and_grad()
        return float(l3[0]), g
    ref = lr.torch_lbfgs(closure, m.get_params(), **E2E_OPTS)
    info = m.train_lbfgs(**E2E_OPTS)
    return m, info, ref


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_stage_follows_torch(name):
    m, info, ref = run_pair(name)
    th, tr = m.get_params(), ref["theta"]
    err = float(np.abs(th - tr).max() / np.abs(tr).max())
    print("%s: iters %d (torch %d), func_evals %d (torch %d), reason %s, margin %.2e, params rel err %.3e, loss %.6e -> %.6e"
          % (name, info["iters"], len(ref["losses"]) - 1, info["func_evals"], ref["func_evals"], info["reason"], ref["margin"], err,
             info["loss"][0, 0], info["loss"][-1, 0]))
    assert ref["margin"] > 1e-6                                   # the seed's check
    assert info["iters"] == len(ref["losses"]) - 1 == 6 and info["func_evals"] == ref["func_evals"]
    assert err <= E2E_TOL
    assert rel(info["loss"][:, 0], ref["losses"]) < 1e-9
    assert np.all(np.diff(info["loss"][:, 0]) <= 0.0)             # Armijo
    if name == "advdiff":
        assert th[-1] != 0.6 and abs(th[-1] - tr[-1]) <= E2E_TOL * abs(tr[-1])      # epsilon moves with the network
    if name == "nonlinear_dual":
        assert m.coefficients()["c"] != 0.7 and abs(th[-1] - tr[-1]) <= E2E_TOL * abs(tr[-1])


def test_properties_by_construction():
    from hp_vpinns_amd import _lib
    a, b = _vpinn2d(3), _vpinn2d(3)
    a.train(5)
    b.train(5)
    st = a.h.get_state()
    P = a.h.num_params()
    n0 = a.h.updates_applied()
    ia, ib = a.train_lbfgs(4, history=3, max_eval=30), b.train_lbfgs(4, history=3, max_eval=30)
    assert ia["iters"] >= 2 and np.array_equal(a.h.get_params(), b.h.get_params()) and np.array_equal(ia["loss"], ib["loss"])      # bitwise, run to run
    assert np.all(np.diff(ia["loss"][:, 0]) <= 0.0)
    assert len(a.loss_his) == 5 + ia["iters"] and a.loss_his[-1] == ia["loss"][-1, 0]
    st2 = a.h.get_state()
    assert np.array_equal(st2[P:], st[P:]) and not np.array_equal(st2[:P], st[:P]) and a.h.updates_applied() == n0      # Adam's state is left alone
    # a forced failure: one evaluation allowed, the search cannot start -- the parameters are the last accepted iterate bit for bit
    accepted = a.h.get_params()
    bad = a.train_lbfgs(3, history=3, max_eval=1)
    assert bad["reason"] == "max_eval" and bad["iters"] == 0 and bad["func_evals"] == 1 and np.array_equal(a.h.get_params(), accepted)
    # the history survives a call and is dropped by the reset: the next direction is -g again, so the runs differ
    a.lbfgs_reset()
    ic = a.train_lbfgs(1, history=3, max_eval=30)
    id_ = b.train_lbfgs(1, history=3, max_eval=30)
    assert ic["iters"] == id_["iters"] == 1 and not np.array_equal(a.h.get_params(), b.h.get_params())
    a.train(3)                                                    # Adam goes on
    assert a.h.updates_applied() == n0 + 3 and np.isfinite(a.loss_his[-1])
    # refusals
    for kw, msg in ((dict(history=0), "history"),):
        with pytest.raises(_lib.HpvError, match=msg) as e:
            a.h.lbfgs_step(2, **kw)
        assert e.value.code == -4


def test_sharded_handle_is_refused():
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.quadrature import GaussLobattoJacobiWeights
    from hp_vpinns_amd.testfcn import tables_1d
    h = _lib.Handle(_lib.PDE_POISSON2D, 1, _lib.ACT_TANH, [2, 20, 20, 20, 1])
    x, w = GaussLobattoJacobiWeights(10, 0, 0)
    h.set_quadrature(x, w, x, w)
    h.set_tables(tables_1d(5, x), tables_1d(5, x))
    h.set_elements(np.linspace(-1, 1, 3), np.linspace(-1, 1, 3), 0, 2)       # two of the four elements
    h.set_rhs(np.zeros(4 * 25))
    h.set_params(theta0([2, 20, 20, 20, 1], 1))
    with pytest.raises(_lib.HpvError, match="shard") as e:
        h.lbfgs_step(2)
    assert e.value.code == -4
