"""The reference side of tests/test_gpu_generic_point.py, without a GPU: at generic points -- warped grids, every weight and bias
perturbed, V = 0.6, random right-hand sides, lossb_weight != 10 -- the three CPU restatements (the autograd element loops, the
vectorised autograd oracle, oracle/closed_form.py) agree PER PARAMETER BLOCK to <= 1e-12, so the 1e-9 the GPU file asserts
block-wise leaves three orders of magnitude over the references' own spread.  Also: the helpers themselves."""
import numpy as np
import pytest

import generic_point as gp
from cases import rel
from oracle import closed_form as CF
from oracle import vpinn_oracle as O

L4 = [2, 20, 20, 20, 1]
AGREE = 1e-12
SEED_ADV = {0: 32, 1: 30}      # (d loss / d epsilon must be >= 1e-4 of the gradient norm: generic_point.BLOCK_FLOOR)


def _three_2d(prob, vf, s, th, lbw=10, V=0.6):
    """(loss3, grad) of the element loop, the vectorised oracle and the closed form on the setup dict `s`"""
    if prob == "p2":
        a = gp.p2_tuple(s, L4)
        mk = lambda: O.OracleVPINN2D(*a, var_form=vf, lossb_weight=lbw, init_params=th)
        q = int(round(np.sqrt(a[4].shape[0])))
        cf = CF.loss_and_grad_2d(th, L4, "poisson2d", vf, a[4][:q, 0], a[5][:q, 0], a[8], a[9], a[10][0][0], a[10][1][0],
                                 np.asarray(a[7], dtype=np.float64), a[0], a[1], float(lbw))
    else:
        a = gp.p3_tuple(s, L4)
        mk = lambda: O.OracleVPINNAdvDiff(*a, var_form=vf, V=V, lossb_weight=lbw, init_params=th)
        q = int(a[5].size)
        cf = CF.loss_and_grad_2d(th, L4, "advdiff", vf, a[3][:q, 0], a[4][:q, 0], a[7], a[8], a[9][0][0], a[9][1][0], None,
                                 a[0], a[1], float(lbw), V=V)
    loop, vec = mk(), mk()
    vec.vectorized = True
    return loop.loss_and_grad(), vec.loss_and_grad(), cf


def _agree(res, layers, n_extra):
    (l3a, ga), (l3b, gb), (l3c, gc) = res
    for l3, g, what in ((l3b, gb, "vectorised"), (l3c, gc, "closed form")):
        k, e = gp.worst_block(g, ga, layers, n_extra)
        print("%s vs element loop: loss rel %.2e, worst block %s %.2e" % (what, rel(l3, l3a), k, e))
        assert rel(l3, l3a) < AGREE, (what, l3, l3a)
        assert e < AGREE, (what, k, e)
    assert gp.block_rel(gc, gb, layers, n_extra) < AGREE


@pytest.mark.parametrize("F", ["recomputed", "random"])
@pytest.mark.parametrize("vf", [0, 1, 2])
def test_three_oracles_agree_blockwise_poisson2d(vf, F):
    from hp_vpinns_amd.drivers import poisson2d
    s = gp.warp_poisson2d(poisson2d.setup(N_el_x=3, N_el_y=4, N_test_x=4, N_test_y=3, N_quad=8, N_bound=9, with_test_grid=False), 11 + vf, F=F)
    assert s["F_ext_total"].shape == (3, 4, 3, 4)
    _agree(_three_2d("p2", vf, s, gp.generic_theta(L4, 20 + vf), lbw=3 if F == "random" else 10), L4, 0)


@pytest.mark.parametrize("vf", [0, 1])
def test_three_oracles_agree_blockwise_advdiff(vf):
    from hp_vpinns_amd.drivers import advdiff
    s = gp.warp_advdiff(advdiff.setup(N_el_x=3, N_el_t=2, N_test_x=4, N_test_t=3, N_quad=8, N_bound=9, with_test_grid=False), 31 + vf)
    th = gp.generic_theta(L4, SEED_ADV[vf], extra=[0.9])
    assert th[-1] == 0.9
    res = _three_2d("adv", vf, s, th, lbw=3 if vf else 10)
    _agree(res, L4, 1)
    # V = 0.6 is visible: the same point under V = 1 is another loss and another d/d eps
    other = _three_2d("adv", vf, s, th, lbw=3 if vf else 10, V=1.0)[1]
    assert abs(other[0][2] - res[1][0][2]) > 1e-3 * abs(res[1][0][2])


@pytest.mark.parametrize("vf", [1, 2, 3])
def test_three_oracles_agree_blockwise_poisson1d(vf):
    """On the shape of the suite's small 1-D fixture (4 elements, 12 points, 6 test functions), warped.  Why not more test functions:
    under var_form 3 a shift of u leaves every U_k unchanged (the rule integrates phi_k'' exactly: sum_q w_q phi_k''(xi_q) =
    phi_k'(1) - phi_k'(-1)), so the variational part of d loss / d b_out is a sum that is analytically zero and its computed value
    is round-off that grows with sum_q |w_q phi_k''|.  Measured spread of the b_out block between the three restatements: 3.5e-13
    (5 test functions, 10 points), 1.1e-12 (12 / 20), 1.4e-12 (60 / 80, the GPU file's 1-D shape; every other block <= 4e-15
    there) -- all three orders below the 1e-9 the GPU file asserts."""
    from hp_vpinns_amd.drivers import poisson1d
    L = [1, 20, 20, 20, 1]
    s = gp.warp_poisson1d(poisson1d.setup(N_Element=4, N_testfcn=6, N_Quad=12), 41)
    a = gp.p1_tuple(s, L)
    th = gp.generic_theta(L, 40 + vf)
    loop, vec = O.OracleVPINN1D(*a, var_form=vf, init_params=th), O.OracleVPINN1D(*a, var_form=vf, init_params=th)
    vec.vectorized = True
    cf = CF.loss_and_grad_1d(th, L, vf, a[2][:, 0], a[3][:, 0], a[5], 6, np.asarray(a[4]), a[0], a[1], 1.0)
    _agree((loop.loss_and_grad(), vec.loss_and_grad(), cf), L, 0)


def test_numpy_rhs_equals_the_drivers_loops():
    """poisson2d_F is the driver's loop: on the driver's own grid against setup(), on a warped grid against the loop of
    poisson2d.setup restated here; warp_poisson1d on the driver's own NON-uniform grid (the published 3-element run) against setup()."""
    from hp_vpinns_amd import GaussLobattoJacobiWeights, Test_fcn
    from hp_vpinns_amd.drivers import poisson1d, poisson2d
    s = poisson2d.setup(N_el_x=3, N_el_y=2, N_test_x=5, N_test_y=4, N_quad=10, N_bound=5, with_test_grid=False)
    assert rel(gp.poisson2d_F(s["grid_x"], s["grid_y"], 5, 4, 10), s["F_ext_total"]) < 1e-13
    w = gp.warp_poisson2d(s, 3)
    gx, gy = w["grid_x"], w["grid_y"]
    X, W = GaussLobattoJacobiWeights(10, 0, 0)
    ax, by = Test_fcn(5, X) * W, Test_fcn(4, X) * W
    F = np.empty((3, 2, 4, 5))
    for ex in range(3):
        xq = gx[ex] + (gx[ex + 1] - gx[ex]) / 2 * (X + 1)
        for ey in range(2):
            yq = gy[ey] + (gy[ey + 1] - gy[ey]) / 2 * (X + 1)
            jac = ((gx[ex + 1] - gx[ex]) / 2) * ((gy[ey + 1] - gy[ey]) / 2)
            F[ex, ey] = jac * (by @ poisson2d.f_ext(xq[None, :], yq[:, None]) @ ax.T)
    assert rel(w["F_ext_total"], F) < 1e-13
    for e in range(6):
        assert rel(w["F_ext_total"].reshape(6, -1)[e], F.reshape(6, -1)[e]) < 1e-12, e
    s1 = poisson1d.setup(N_Element=3, N_testfcn=15, N_Quad=30)
    assert np.allclose(s1["grid"], [-1, -0.1, 0.1, 1])

    w1 = gp.warp_poisson1d(s1, 0, grid=s1["grid"])
    assert rel(w1["F_ext_total"], s1["F_ext_total"]) < 1e-13


def test_warp_generic_theta_and_blocks():
    rng = np.random.default_rng(5)
    g = gp.warp(np.linspace(-1, 1, 17), rng)
    d = np.diff(g)
    assert g[0] == -1 and g[-1] == 1 and g.size == 17 and d.min() > 0 and len(set(d)) == 16 and d.max() / d.min() < 3.0001
    assert d.max() / d.min() > 1.5                                   # (a seeded draw: far from uniform)
    assert np.array_equal(gp.warp(np.array([0.0, 1.0]), rng), [0.0, 1.0])
    th = gp.generic_theta(L4, 7, extra=[0.9])
    from hp_vpinns_amd.init import xavier_init
    x0 = xavier_init(L4, 7, extra=[0.9])
    assert th.size == x0.size == 922 and th[-1] == 0.9 and np.all(th[:-1] != x0[:-1])
    bl = gp.blocks(L4, 1)
    assert [b[0] for b in bl] == ["W0", "b0", "W1", "b1", "W2", "b2", "W3", "b3", "eps"]
    assert bl[0][1] == 0 and bl[-1][2] == 922 and all(bl[i][2] == bl[i + 1][1] for i in range(len(bl) - 1))
    for name, lo, hi in bl[:-2]:                                     # (b3 is one number)
        assert abs(np.std(th[lo:hi] - x0[lo:hi]) - 0.3) < (0.2 if hi - lo < 30 else 0.05), name
    # block_rel sees an error a global norm hides, and refuses a case with a negligible block
    gref = np.concatenate([np.full(921, 10.0), [0.05]])
    gbad = gref.copy()
    gbad[-1] *= 1 + 1e-6
    assert rel(gbad, gref) < 1e-9 and gp.block_rel(gbad, gref, L4, 1) > 9e-7
    gref[-1] = 1e-3
    with pytest.raises(AssertionError, match="ill-posed"):
        gp.block_rel(gref, gref, L4, 1)
