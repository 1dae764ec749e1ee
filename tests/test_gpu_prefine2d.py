"""Per-element test-function counts of the 2-D problems (p-refinement: the reference classes read N_testfcn[0][ex] / N_testfcn[1][ey]
per element, P2:72-73 / P3:112-113) through hpv_set_active_tests_2d, the general projections and the whole-iteration kernel
k_iter_fused.  Against the oracle's element loops (`vectorized=False`: they read the same lists and take F_ext_total[ex, ey]) on
identical inputs and initial parameters; larger grids against the generic backend (k_project).  Tolerances: the project's own,
1e-9 on loss / gradient, 1e-7 on trajectories (test_gpu_parity.py); shard additivity 1e-12 / 1e-11 as in the 1-D shard test.

Time of this file on one MI355X: see profiles/p_refine_2d.md."""
import os
import socket

import numpy as np
import pytest

from cases import rel, theta0

pytestmark = pytest.mark.gpu

TOL = 1e-9
TRAJ_TOL = 1e-7
L4 = [2, 20, 20, 20, 1]
NAX, NAY = [5, 3, 4], [2, 5]            # the small grid: 3 x 2 elements


def _p2(nex, ney, nax, nay, q, nb=13):
    from hp_vpinns_amd.drivers import poisson2d
    s = poisson2d.setup(N_el_x=nex, N_el_y=ney, N_test_x=nax, N_test_y=nay, N_quad=q, N_bound=nb, with_test_grid=False)
    return (s["X_u_train"], s["u_train"], s["X_f_train"], s["f_train"], s["XY_quad_train"], s["WXY_quad_train"], None,
            s["F_ext_total"], s["grid_x"], s["grid_y"], s["N_testfcn_total"], s["X_u_train"], s["u_train"])


def _p3(nex, net, nax, nat, q, nb=11):
    from hp_vpinns_amd.drivers import advdiff
    s = advdiff.setup(N_el_x=nex, N_el_t=net, N_test_x=nax, N_test_t=nat, N_quad=q, N_bound=nb, with_test_grid=False)
    return (s["XT_u_train"], s["u_train"], s["XT_f_train"], s["XT_quad_train"], s["WXT_quad_train"], s["T_quad"], s["WT_quad"],
            s["grid_x"], s["grid_t"], s["N_testfcn_total"], s["XT_u_train"], s["u_train"])


def _env(env):
    """context manager: environment switches the library reads when a model is built / a pass is launched"""
    class _E:
        def __enter__(self):
            self.saved = {k: os.environ.get(k) for k in env}
            os.environ.update(env)

        def __exit__(self, *a):
            for k, v in self.saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _E()


def _pair(prob, vf, args, th, backend="auto", oracle=True):
    if prob == "p2":
        from hp_vpinns_amd.vpinn import VPINN2D as M
        from oracle.vpinn_oracle import OracleVPINN2D as O
        a = args + (L4,)
    else:
        from hp_vpinns_amd.vpinn import VPINNAdvDiff as M
        from oracle.vpinn_oracle import OracleVPINNAdvDiff as O
        a = args + (L4, None, None)
    o = O(*a, var_form=vf, init_params=th) if oracle else None
    if o is not None:
        o.vectorized = False                 # the reference-structured element loops: they read the counts per element
    return o, M(*a, var_form=vf, init_params=th, backend=backend)


def _residual_blocks(m, nax_e, nay_e, ntx, nty, lossv):
    """zero outside each element's block, at most a handful of exact zeros inside, lossv = sum_e mean over ITS block"""
    ne = len(nax_e)
    r = m.h.residuals(ne * nty * ntx).reshape(ne, nty, ntx)
    s = 0.0
    for e in range(ne):
        ax, ay = int(nax_e[e]), int(nay_e[e])
        assert np.all(r[e, ay:, :] == 0.0) and np.all(r[e, :, ax:] == 0.0), e
        assert np.count_nonzero(r[e, :ay, :ax]) >= ax * ay - 3, e      # (a high-order row can round to exactly 0)
        s += float(np.mean(r[e, :ay, :ax] ** 2))
    print("lossv %.17e  sum_e mean(R_e^2) %.17e" % (lossv, s))
    assert abs(lossv - s) < 1e-10 * abs(lossv)
    return r


def _check_loss_grad(o, m, adv):
    l3o, go = o.loss_and_grad()
    l3m, gm = m.loss_and_grad()
    print("variant", m.h.kernel_variant(), "| loss", l3m, l3o, "| grad rel", rel(gm, go), "| lossv rel", rel(l3m[2], l3o[2]))
    assert rel(l3m, l3o) < TOL, (l3m, l3o)
    assert rel(gm, go) < TOL, (rel(gm, go), np.abs(gm - go).max())
    assert rel(m.loss(), l3o) < TOL                    # forward-only evaluation
    # lossv on its own: in the AdvDiff problem it is 1e-5 of lossb, a relative error on the triple cannot see the counts
    assert rel(l3m[2], l3o[2]) < TOL, (l3m[2], l3o[2])
    assert rel(m.loss()[2], l3o[2]) < TOL
    if adv:
        print("d eps", gm[-1], go[-1])
        assert rel(gm[-1], go[-1]) < TOL, (gm[-1], go[-1])
    return l3m


def _check_variational_grad(o, m, adv):
    """the gradient of the variational term alone: data term off on both sides"""
    m.h.set_data(None, None)
    o.use_data = False
    try:
        l3o, go = o.loss_and_grad()
        l3m, gm = m.loss_and_grad()
        print("no data term: lossv", l3m[2], l3o[2], "| grad rel", rel(gm, go), "| d eps", gm[-1], go[-1])
        assert l3m[1] == 0.0 and rel(l3m[2], l3o[2]) < TOL
        assert rel(gm, go) < TOL, (rel(gm, go), np.abs(gm - go).max())
        if adv:
            assert rel(gm[-1], go[-1]) < TOL, (gm[-1], go[-1])
    finally:
        o.use_data = True


def _check_traj(o, m, n=8):
    lo, lm = [], []
    for _ in range(n):
        o.adam_step()
        lo.append(float(o.loss_parts()[0]))
        lm.append(float(m._step(1, True)[0]))
    assert rel(lm, lo) < TRAJ_TOL, (lm, lo)
    assert rel(m.get_params(), o.get_params()) < TRAJ_TOL


def _fused_built(m, gen=False):
    bi = m.h.build_info()
    return bi["k_iter_fused"] != "absent" and (not gen or bi.get("k_iter_fused_gen", "ok") != "absent")


# ---- 1. small grids: every form, both backends ---------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["auto", "generic"])
@pytest.mark.parametrize("prob,vf", [("p2", 0), ("p2", 1), ("p2", 2), ("adv", 0), ("adv", 1)])
def test_small_grid_every_form_against_the_oracle_element_loop(prob, vf, backend):
    adv = prob == "adv"
    args = _p3(3, 2, NAX, NAY, 12) if adv else _p2(3, 2, NAX, NAY, 12)
    th = theta0(L4, 21, extra=[0.7] if adv else ())
    o, m = _pair(prob, vf, args, th, backend)
    l3 = _check_loss_grad(o, m, adv)
    nax_e, nay_e = np.repeat(NAX, 2), np.tile(NAY, 3)
    _residual_blocks(m, nax_e, nay_e, 5, 5, float(l3[2]))
    _check_traj(o, m, n=8)
    # the variational gradient on its own (a fresh pair: the trajectory moved the parameters)
    o2, m2 = _pair(prob, vf, args, th, backend)
    _check_variational_grad(o2, m2, adv)
    # the same problem WITHOUT the counts (dense F, padded with zeros) is a different loss
    if not adv:
        from hp_vpinns_amd.vpinn import VPINN2D
        a = list(args + (L4,))
        a[7] = m.F_ext_total
        a[10] = [[5, 5, 5], [5, 5]]
        m3 = VPINN2D(*a, var_form=vf, init_params=th, backend=backend)
        assert abs(m3.loss_and_grad()[0][2] - l3[2]) > 1e-6 * abs(l3[2])


# ---- 2. the hot path -----------------------------------------------------------------------------------------------------------
def _pattern(nex, ney, ntmax):
    """counts that vary by column and by row, at most ntmax"""
    nax = [max(1, ntmax - 6 + (3 * ex) % 7) for ex in range(nex)]
    nay = [ntmax - (ey % 5) for ey in range(ney)]
    return nax, nay


def _assert_counted_fused(m, gen=False, split=None, loop=False):
    v = m.h.kernel_variant()
    print("variant:", v, "| structure:", m.h.pass_structure())
    if not _fused_built(m, gen):
        return
    assert m.h.pass_structure() in (("whole-iteration-split",) if split else ("whole-iteration",)), (m.h.pass_structure(), v)
    assert v.startswith("k_iter_fused<") and ",NACT>" in v, v
    if loop:
        assert v.endswith("elements-per-workgroup>1"), v


def test_config4_shape_counted_runs_the_whole_iteration_kernel_against_the_oracle():
    """16 x 16 elements of 20 x 20 points, at most 10 x 10 test functions: nax[ex] = 4 + (3 ex) % 7, nay[ey] = 10 - ey % 5; Poisson-2D
    var_form 1 (the one-hot headline instantiation).  Loss triple and gradient against the oracle's element loop at full size."""
    nax, nay = _pattern(16, 16, 10)
    assert nax[:4] == [4, 7, 10, 6] and max(nax) == 10 and nay[:6] == [10, 9, 8, 7, 6, 10]
    args = _p2(16, 16, nax, nay, 20)
    th = theta0(L4, 22)
    o, m = _pair("p2", 1, args, th)
    l3 = _check_loss_grad(o, m, False)
    _assert_counted_fused(m)
    assert m.h.kernel_variant().startswith("k_iter_fused<L=3,SPLIT=false,") or not _fused_built(m)
    _residual_blocks(m, np.repeat(nax, 16), np.tile(nay, 16), 10, 10, float(l3[2]))


@pytest.mark.parametrize("case", ["no-quarter-tile", "16x16", "12x12", "p2-vf0-16x16", "adv-vf0-16x16", "adv-vf1-12x12"])
def test_counted_whole_iteration_kernel_other_plans_shapes_and_forms_against_the_generic_backend(case):
    """One round of elements (16 x 16) on: whole tiles only (HPV_NO_QUARTER_TILE=1), the 16 x 16- and 12 x 12-point shapes (one-hot),
    and the general instantiations (GEN / NT2: Poisson-2D var_form 0, AdvDiff var_form 0 / 1).  Reference: the generic backend
    (k_project), itself checked against the oracle on the small grids above."""
    env = {}
    prob, vf, q = "p2", 1, 20
    if case == "no-quarter-tile":
        env = {"HPV_NO_QUARTER_TILE": "1"}
    elif case in ("16x16", "12x12"):
        q = int(case[:2])
    else:
        prob, vf, q = case.split("-")[0], int(case.split("-")[1][2:]), int(case[-2:])
    adv = prob == "adv"
    nax, nay = _pattern(16, 16, q // 2)
    args = _p3(16, 16, nax, nay, q) if adv else _p2(16, 16, nax, nay, q)
    th = theta0(L4, 23, extra=[0.6] if adv else ())
    with _env(env):
        _, m = _pair(prob, vf, args, th, oracle=False)
        l3m, gm = m.loss_and_grad()
        _assert_counted_fused(m, gen=not (prob == "p2" and vf == 1))
        v = m.h.kernel_variant()
    if _fused_built(m, gen=not (prob == "p2" and vf == 1)):
        if case == "no-quarter-tile":
            assert "QT=false" in v, v
        if prob != "p2" or vf != 1:
            assert ",GEN" in v and ("NT2=1" in v) == (vf == 0), v
    _, g = _pair(prob, vf, args, th, backend="generic", oracle=False)
    l3g, gg = g.loss_and_grad()
    print("loss", l3m, l3g, "grad rel", rel(gm, gg))
    assert rel(l3m, l3g) < TOL and rel(l3m[2], l3g[2]) < TOL and rel(gm, gg) < TOL, (l3m, l3g, rel(gm, gg))
    nt = q // 2
    assert rel(m.h.residuals(256 * nt * nt), g.h.residuals(256 * nt * nt)) < TOL
    _residual_blocks(m, np.repeat(nax, 16), np.tile(nay, 16), nt, nt, float(l3m[2]))
    if adv:
        assert rel(gm[-1], gg[-1]) < TOL, (gm[-1], gg[-1])
        m.h.set_data(None, None)
        g.h.set_data(None, None)
        (l3a, ga), (l3b, gb) = m.loss_and_grad(), g.loss_and_grad()
        print("no data term: grad rel", rel(ga, gb), "d eps", ga[-1], gb[-1])
        assert rel(l3a[2], l3b[2]) < TOL and rel(ga, gb) < TOL and rel(ga[-1], gb[-1]) < TOL
    else:
        m._step(3, False)
        g._step(3, False)
        assert rel(m.get_params(), g.get_params()) < TRAJ_TOL


def test_counted_element_loop_on_full_rounds_against_the_separate_launches():
    """32 x 24 = 768 elements of 12 x 12 points: three full rounds on a 256-CU chip, walked by the element loop (HPV_FUSE=m);
    the same problem on the separate launches (HPV_FUSE=n: general projection) is the reference."""
    nax, nay = _pattern(32, 24, 6)
    args = _p2(32, 24, nax, nay, 12)
    th = theta0(L4, 24)
    assert "HPV_FUSE" not in os.environ
    with _env({"HPV_FUSE": "m"}):
        _, m = _pair("p2", 1, args, th, oracle=False)
    with _env({"HPV_FUSE": "n"}):
        _, s = _pair("p2", 1, args, th, oracle=False)
    l3m, gm = m.loss_and_grad()
    l3s, gs = s.loss_and_grad()
    v = m.h.kernel_variant()
    print("variant:", v, "| reference:", s.h.kernel_variant())
    assert "k_iter_fused" not in s.h.kernel_variant()
    if _fused_built(m) and v.startswith("k_iter_fused"):
        assert ",NACT>" in v, v
    if _fused_built(m) and "elements-per-workgroup>1" not in v:
        pytest.fail("the element loop did not take a grid of three full rounds under HPV_FUSE=m: " + v)
    assert rel(l3m, l3s) < TOL and rel(gm, gs) < TOL, (l3m, l3s, rel(gm, gs))
    assert rel(m.h.residuals(768 * 36), s.h.residuals(768 * 36)) < TOL
    _residual_blocks(m, np.repeat(nax, 24), np.tile(nay, 32), 6, 6, float(l3m[2]))
    m._step(3, False)
    s._step(3, False)
    assert rel(m.get_params(), s.get_params()) < TRAJ_TOL


# ---- 3. small shards -----------------------------------------------------------------------------------------------------------
def test_small_shard_shared_elements():
    """8 x 8 elements of 20 x 20 points: 64 elements on 256 CUs, an element is shared by several workgroups (SPLIT).  Whatever runs is
    correct against the generic backend, a counted SPLIT run says so in its name, and training steps go through (no exchange error)."""
    nax, nay = _pattern(8, 8, 10)
    args = _p2(8, 8, nax, nay, 20)
    th = theta0(L4, 25)
    _, m = _pair("p2", 1, args, th, oracle=False)
    _, g = _pair("p2", 1, args, th, backend="generic", oracle=False)
    l3m, gm = m.loss_and_grad()
    l3g, gg = g.loss_and_grad()
    v = m.h.kernel_variant()
    print("variant:", v, "| structure:", m.h.pass_structure())
    if "SPLIT=true" in v:
        assert ",NACT>" in v and m.h.pass_structure() == "whole-iteration-split", v
    assert rel(l3m, l3g) < TOL and rel(gm, gg) < TOL, (l3m, l3g, rel(gm, gg))
    _residual_blocks(m, np.repeat(nax, 8), np.tile(nay, 8), 10, 10, float(l3m[2]))
    m._step(4, True)                       # (an HpvError -7 would raise)
    g._step(4, True)
    assert rel(m.get_params(), g.get_params()) < TRAJ_TOL


# ---- 4. pairs that are no column x row product ---------------------------------------------------------------------------------
PAIRS_X, PAIRS_Y = [5, 1, 3, 4, 2, 5], [2, 5, 1, 3, 4, 5]


@pytest.mark.parametrize("backend", ["auto", "generic"])
@pytest.mark.parametrize("prob,vf", [("p2", 1), ("p2", 0), ("adv", 1)])
def test_arbitrary_pairs_through_the_c_abi_add_up_element_by_element(prob, vf, backend):
    """Six arbitrary (nax, nay) pairs on a 3 x 2 grid -- the oracle cannot express them.  One handle per element (its pair, no data
    term) + one handle with the data term alone add up to the whole problem's loss and gradient."""
    adv = prob == "adv"
    args = _p3(3, 2, 5, 5, 12) if adv else _p2(3, 2, 5, 5, 12)
    th = theta0(L4, 26, extra=[0.8] if adv else ())
    gx, gy = args[7:9] if adv else args[8:10]

    def model():
        m = _pair(prob, vf, args, th, backend, oracle=False)[1]
        m.h.set_active_tests_2d(PAIRS_X, PAIRS_Y)
        return m
    full = model()
    l3, g = full.h.loss_and_grad()
    print("variant:", full.h.kernel_variant())
    _residual_blocks(full, PAIRS_X, PAIRS_Y, 5, 5, float(l3[2]))
    lv, gsum = 0.0, np.zeros_like(g)
    for e in range(6):
        m = model()
        m.h.set_elements(gx, gy, e, e + 1)           # the counts survive and are sliced
        m.h.set_data(None, None)
        le, ge = m.h.loss_and_grad()
        r = m.h.residuals(25).reshape(5, 5)
        assert np.all(r[PAIRS_Y[e]:, :] == 0.0) and np.all(r[:, PAIRS_X[e]:] == 0.0)
        assert le[1] == 0.0 and abs(le[2] - np.mean(r[:PAIRS_Y[e], :PAIRS_X[e]] ** 2)) < 1e-10 * abs(le[2])
        lv += le[2]
        gsum += ge
    d = model()
    d.h.set_elements(gx, gy, 0, 0)                   # no element: the data term alone
    ld, gd = d.h.loss_and_grad()
    assert ld[2] == 0.0 and rel(ld[1], l3[1]) < 1e-13
    print("lossv", l3[2], lv, "grad rel", rel(gsum + gd, g))
    assert rel(lv, l3[2]) < 1e-12 and rel(gsum + gd, g) < 1e-11


# ---- 5. shards -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["auto", "generic"])
def test_shards_of_a_counted_problem_add_up(backend):
    """Two element ranges of one counted problem -- [0, 3) ends in the middle of element column 1 -- with the boundary term on the
    first: variational losses and gradients add up to the whole problem's (F and the counts are sliced inside the library)."""
    args = _p2(3, 2, NAX, NAY, 12)
    th = theta0(L4, 27)
    nax_e, nay_e = np.repeat(NAX, 2), np.tile(NAY, 3)
    full = _pair("p2", 1, args, th, backend, oracle=False)[1]
    l3, g = full.h.loss_and_grad()
    parts = []
    for eb, ee, with_data in ((0, 3, True), (3, 6, False)):
        m = _pair("p2", 1, args, th, backend, oracle=False)[1]
        m.h.set_elements(args[8], args[9], eb, ee)
        if not with_data:
            m.h.set_data(None, None)
        parts.append(m.h.loss_and_grad())
        print("shard", eb, ee, m.h.kernel_variant())
        _residual_blocks(m, nax_e[eb:ee], nay_e[eb:ee], 5, 5, float(parts[-1][0][2]))
    (la, ga), (lb, gb) = parts
    assert lb[1] == 0.0 and rel(la[1], l3[1]) < 1e-13
    assert rel(la[2] + lb[2], l3[2]) < 1e-12 and rel(ga + gb, g) < 1e-11


# ---- 6. argument checks and reset ----------------------------------------------------------------------------------------------
def test_argument_checks_and_reset():
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.drivers import poisson1d, poisson2d
    from hp_vpinns_amd.init import xavier_init
    from hp_vpinns_amd.vpinn import VPINN1D, VPINN2D
    args = _p2(3, 2, 5, 5, 12)
    th = theta0(L4, 28)
    m = _pair("p2", 1, args, th, oracle=False)[1]
    l0, g0 = m.h.loss_and_grad()
    ok_x, ok_y = np.repeat(NAX, 2), np.tile(NAY, 3)
    for bx, by in (([0, 5, 5, 5, 5, 5], [5] * 6), ([5] * 6, [5, 5, 0, 5, 5, 5]), ([6, 5, 5, 5, 5, 5], [5] * 6), ([5] * 6, [5, 5, 5, 5, 5, 6]),
                   ([5] * 5, [5] * 5), ([5] * 7, [5] * 7)):
        with pytest.raises(_lib.HpvError):
            m.h.set_active_tests_2d(bx, by)
    with pytest.raises(ValueError):
        m.h.set_active_tests_2d(ok_x, None)
    l0b, g0b = m.h.loss_and_grad()
    assert np.array_equal(l0b, l0) and np.array_equal(g0b, g0)         # a refused call changes nothing
    m.h.set_active_tests_2d(ok_x, ok_y)
    l1, g1 = m.h.loss_and_grad()
    assert abs(l1[2] - l0[2]) > 1e-9 * abs(l0[2])
    m.h.set_elements(args[8], args[9], 0, 6)                           # the counts survive a following set_elements
    l1b, g1b = m.h.loss_and_grad()
    assert np.array_equal(l1b, l1) and np.array_equal(g1b, g1)
    with pytest.raises(_lib.HpvError):
        m.h.set_active_tests([5] * 6)                                  # the 1-D entry point still refuses 2-D handles
    m.h.set_active_tests_2d(None, None)
    l2, g2 = m.h.loss_and_grad()
    assert np.array_equal(l2, l0) and np.array_equal(g2, g0)           # bit for bit
    # a 1-D handle
    s = poisson1d.setup(N_Element=3)
    L1 = [1, 20, 20, 1]
    t1 = xavier_init(L1, 2)
    t1[20:40] = 0.1
    m1 = VPINN1D(s["X_u_train"], s["u_train"], s["X_quad_train"], s["W_quad_train"], s["F_ext_total"], s["grid"], s["X_test"],
                 s["u_test"], L1, s["X_f_train"], s["f_train"], init_params=t1)
    with pytest.raises(_lib.HpvError):
        m1.h.set_active_tests_2d([5, 5, 5], [1, 1, 1])
    # the strong-form PINN scheme
    s2 = poisson2d.setup(N_el_x=2, N_el_y=2, with_test_grid=False)
    mp = poisson2d.build_model(s2, [2, 20, 20, 1], init_params=xavier_init([2, 20, 20, 1], 2), scheme="PINNs")
    with pytest.raises(_lib.HpvError):
        mp.h.set_active_tests_2d([5] * 4, [5] * 4)
    # a block whose shape contradicts the counts
    a = list(_p2(3, 2, NAX, NAY, 12) + (L4,))
    F = a[7].copy()
    F[2, 1] = np.zeros((5, 5))
    a[7] = F
    with pytest.raises(ValueError):
        VPINN2D(*a, init_params=th)
    # uniform counts given as lists make no call to the new entry point: same bits as the integer set-up
    mu = _pair("p2", 1, _p2(3, 2, [5, 5, 5], [5, 5], 12), th, oracle=False)[1]
    lu, gu = mu.h.loss_and_grad()
    assert np.array_equal(lu, l0) and np.array_equal(gu, g0) and "NACT" not in mu.h.kernel_variant()


# ---- 7. graphs and the deferred update -----------------------------------------------------------------------------------------
def test_counted_training_through_graphs_eager_launches_and_the_deferred_update():
    """A counted config-4-shape model trained 20 steps through hpv_step (captured graphs), with HPV_NO_GRAPH=1 (eager launches) and
    under HPV_FORCE_DIST=1 with a one-rank group (the in-library exchange: the TF1-Adam update rides in the iteration kernel's
    prologue): the same parameters."""
    import torch
    import torch.distributed as dist
    nax, nay = _pattern(16, 16, 10)
    args = _p2(16, 16, nax, nay, 20)
    th = theta0(L4, 29)

    def train(env):
        with _env(env):
            m = _pair("p2", 1, args, th, oracle=False)[1]
            m._step(20, False)
            l3 = m.loss()
            return m, m.get_params(), l3
    m0, p0, l0 = train({})
    assert m0.h.graphs_in_use()
    _assert_counted_fused(m0)
    m1, p1, l1 = train({"HPV_NO_GRAPH": "1"})
    assert not m1.h.graphs_in_use()
    print("graphs vs eager: params rel", rel(p1, p0))
    assert rel(p1, p0) < TRAJ_TOL and rel(l1, l0) < TRAJ_TOL
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        m2, p2, l2 = train({"HPV_FORCE_DIST": "1"})
        assert m2._dist and m2.exchange() == "rccl", m2.exchange()
        v = m2.h.kernel_variant()
        print("deferred update:", v, "| params rel", rel(p2, p0))
        if _fused_built(m2):
            assert v.startswith("k_iter_fused<") and ",NACT>" in v, v
        assert rel(p2, p0) < TRAJ_TOL and rel(l2, l0) < TRAJ_TOL
    finally:
        dist.destroy_process_group()
