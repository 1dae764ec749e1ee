"""Local hp-refinement on the GPU: element boxes (hpv_set_element_boxes), the device-side refinement indicators
(hpv_element_indicators, k_elem_indicators) and the refine-and-continue loop (set_mesh / adapt / train_adaptive).

References: the tensor grid itself (bit for bit), the oracle classes summed box by box (tests/adapt_reference.py), known answers
for a zero network.  Tolerances: 1e-9 on loss / gradient / d epsilon as tests/test_gpu_parity.py holds them; 1e-8 of the column norm
on each indicator column (r per point is held to 1e-9, tests/test_gpu_headline.py, and the sums are quadratic in it).

Shapes: 2 x 2 grids and the 7-box list (a 2 x 2 grid with one element split in four, unequal counts); rules of 5 x 5 and 12 x 12
points (6 x 6 test functions on the latter); [2, 5, 5, 1] on the generic backend and [2, 20, 20, 20, 1] on the default dispatch; a
3-interval 1-D problem."""
import ctypes as C
import os

import numpy as np
import pytest

import adapt_reference as ar
from cases import rel, theta0
from test_adapt_host import seven_boxes

pytestmark = pytest.mark.gpu

TOL = 1e-9
L4, L2 = [2, 20, 20, 20, 1], [2, 5, 5, 1]
# (network, backend, rule points, table size): the generic kernels on the small rule, the default dispatch on 12 x 12 / 6 x 6
SHAPES = {"generic5": (L2, "generic", 5, 5), "auto12": (L4, "auto", 12, 6)}


def _setup(prob, q, nt, nb=11):
    if prob == "p2":
        from hp_vpinns_amd.drivers import poisson2d
        s = poisson2d.setup(N_el_x=2, N_el_y=2, N_test_x=nt, N_test_y=nt, N_quad=q, N_bound=nb, with_test_grid=False)
        return s, (s["X_u_train"], s["u_train"], s["X_f_train"], s["f_train"], s["XY_quad_train"], s["WXY_quad_train"], None,
                   s["F_ext_total"], s["grid_x"], s["grid_y"], s["N_testfcn_total"], s["X_u_train"], s["u_train"])
    from hp_vpinns_amd.drivers import advdiff
    s = advdiff.setup(N_el_x=2, N_el_t=2, N_test_x=nt, N_test_t=nt, N_quad=q, N_bound=nb, with_test_grid=False)
    return s, (s["XT_u_train"], s["u_train"], s["XT_f_train"], s["XT_quad_train"], s["WXT_quad_train"], s["T_quad"], s["WT_quad"],
               s["grid_x"], s["grid_t"], s["N_testfcn_total"], s["XT_u_train"], s["u_train"])


def _model(prob, vf, shape, th=None, seed=21, **kw):
    layers, backend, q, nt = SHAPES[shape]
    s, args = _setup(prob, q, nt)
    if th is None:
        th = theta0(layers, seed, extra=[0.7] if prob == "adv" else ())
    if prob == "p2":
        from hp_vpinns_amd.vpinn import VPINN2D
        m = VPINN2D(*args, layers, var_form=vf, init_params=th, backend=backend, **kw)
    else:
        from hp_vpinns_amd.vpinn import VPINNAdvDiff
        m = VPINNAdvDiff(*args, layers, None, None, var_form=vf, init_params=th, backend=backend, V=0.8, **kw)
    return m, s, th


def _rule(q):
    from hp_vpinns_amd.quadrature import GaussLobattoJacobiWeights
    x, w = GaussLobattoJacobiWeights(q, 0, 0)
    return x, w, x.copy(), w.copy()


def _f(prob):
    from hp_vpinns_amd.drivers import poisson2d
    return poisson2d.f_ext if prob == "p2" else (lambda x, t: np.sin(2.0 * x + 0.3) * np.cos(1.5 * t) + 0.5 * x * t)


def _data(prob, s):
    return (s["X_u_train"], s["u_train"]) if prob == "p2" else (s["XT_u_train"], s["u_train"])


def _mesh7(shape):
    """the 7-box list on the problem's domain with counts that fit the shape's tables"""
    m = seven_boxes()
    nt = SHAPES[shape][3]
    m.nax[:] = np.minimum(m.nax + (nt - 5), nt)
    m.nay[:] = np.minimum(m.nay + (nt - 5), nt)
    return m


def _mesh7_for(prob, shape):
    m = _mesh7(shape)
    if prob == "adv":       # AdvDiff's domain is [-1, 1] x [0, 1]
        m.boxes[:, 2:] = (m.boxes[:, 2:] + 1) / 2
    return m


def _need_fused(m, shape, prob, vf):
    """At the start of every 12 x 12 case: the default dispatch must have taken k_iter_fused (hpv_kernel_variant after one reverse-mode
    pass), or the case skips with the build's reason before doing any work.  Poisson-2D var_form 2 is a one-channel form, which the
    dispatch gives to the generic element-resident kernel k_iter_elem or, with per-element counts, to the per-layer MFMA kernels +
    k_project_wg (README.md, 'element shapes'): there the MFMA backend is asserted."""
    if shape != "auto12":
        return
    bi = m.h.build_info()
    if bi["k_iter_fused"] == "absent" or bi.get("k_iter_fused_gen", "ok") == "absent":
        pytest.skip("this build has no k_iter_fused: %s" % bi)
    m.loss_and_grad()
    if (prob, vf) == ("p2", 2):
        assert m.backend() == "mfma" and "generic" not in m.h.kernel_variant(), m.h.kernel_variant()
    else:
        assert "k_iter_fused" in m.h.kernel_variant(), m.h.kernel_variant()


# ---- 1. grid = boxes, bit for bit ----------------------------------------------------------------------------------------------------
def _twin_check(m1, m2, nres):
    l1, g1 = m1.loss_and_grad()
    l2, g2 = m2.loss_and_grad()
    assert m1.h.kernel_variant() == m2.h.kernel_variant(), (m1.h.kernel_variant(), m2.h.kernel_variant())
    assert np.array_equal(l1, l2) and np.array_equal(g1, g2)
    assert np.array_equal(m1.h.residuals(nres), m2.h.residuals(nres))
    m1._step(20, False)
    m2._step(20, False)
    assert np.array_equal(m1.h.get_state(), m2.h.get_state())
    assert m1.h.kernel_variant() == m2.h.kernel_variant()


@pytest.mark.parametrize("shape", ["generic5", "auto12"])
@pytest.mark.parametrize("prob,vf", [("p2", 0), ("p2", 1), ("p2", 2), ("adv", 0), ("adv", 1)])
def test_grid_and_its_box_list_agree_bit_for_bit_2d(prob, vf, shape):
    from hp_vpinns_amd.adapt import ElementMesh
    m1, s, th = _model(prob, vf, shape)
    _need_fused(m1, shape, prob, vf)
    m2, _, _ = _model(prob, vf, shape, th=th)
    gy = s["grid_y"] if prob == "p2" else s["grid_t"]
    m2.h.set_element_boxes(ElementMesh.from_grid(s["grid_x"], gy).boxes)
    m2.h.backend_in_use()
    nt = SHAPES[shape][3]
    _twin_check(m1, m2, 4 * nt * nt)


@pytest.mark.parametrize("vf", [1, 3])
@pytest.mark.parametrize("backend,layers", [("generic", [1, 5, 5, 1]), ("auto", [1, 20, 20, 20, 1])])
def test_grid_and_its_box_list_agree_bit_for_bit_1d(vf, backend, layers):
    from hp_vpinns_amd.adapt import ElementMesh
    from hp_vpinns_amd.drivers import poisson1d
    from hp_vpinns_amd.vpinn import VPINN1D
    s = poisson1d.setup(N_Element=3, N_testfcn=5, N_Quad=10)
    a = (s["X_u_train"], s["u_train"], s["X_quad_train"], s["W_quad_train"], s["F_ext_total"], s["grid"], s["X_u_train"], s["u_train"], layers)
    th = theta0(layers, 5)
    with_env = {"HPV_NO_RULE_PADDING": "1"}      # (both twins on the rule as it is: the boxes replace the elements, not the rule)
    old = {k: os.environ.get(k) for k in with_env}
    os.environ.update(with_env)
    try:
        m1 = VPINN1D(*a, var_form=vf, init_params=th, backend=backend)
        m2 = VPINN1D(*a, var_form=vf, init_params=th, backend=backend)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    m2.h.set_element_boxes(ElementMesh.from_grid(s["grid"]).boxes)
    m2.h.backend_in_use()
    _twin_check(m1, m2, 3 * 5)


# ---- 2. a non-tensor list against the oracle, summed box by box -------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["generic5", "auto12"])
@pytest.mark.parametrize("prob,vf", [("p2", 0), ("p2", 1), ("p2", 2), ("adv", 0), ("adv", 1)])
def test_seven_boxes_loss_gradient_and_d_epsilon_against_the_oracle(prob, vf, shape):
    layers, _, q, _ = SHAPES[shape]
    m, s, th = _model(prob, vf, shape)
    mesh = _mesh7_for(prob, shape)
    f = _f(prob) if prob == "p2" else None              # (the oracle's AdvDiff class has a zero right-hand side)
    m.set_mesh(mesh, f)
    _need_fused(m, shape, prob, vf)
    rule = _rule(q)
    F = ar.f_blocks(mesh, f, *rule)
    l3o, go = ar.box_loss_and_grad(prob, vf, mesh, F, rule, _data(prob, s), layers, th, V=0.8)
    l3m, gm = m.loss_and_grad()
    print("variant", m.h.kernel_variant(), "| loss", l3m, l3o, "| grad rel", rel(gm, go))
    assert rel(l3m, l3o) < TOL, (l3m, l3o)
    assert rel(l3m[2], l3o[2]) < TOL, (l3m[2], l3o[2])
    assert rel(gm, go) < TOL, (rel(gm, go), np.abs(gm - go).max())
    assert rel(m.loss(), l3o) < TOL
    if prob == "adv":
        print("d eps", gm[-1], go[-1])
        assert rel(gm[-1], go[-1]) < TOL, (gm[-1], go[-1])


def test_seven_boxes_on_two_handles_add_up_to_the_whole():
    """[0, 3) + [3, 7) of the list on two handles: partial sums add up (tolerances of the 1-D shard test of test_gpu_parity.py)"""
    from hp_vpinns_amd import _lib
    m, s, th = _model("p2", 1, "generic5")
    mesh = _mesh7_for("p2", "generic5")
    m.set_mesh(mesh, _f("p2"))
    l3, g = m.loss_and_grad()
    xi, yi = m._dev_rule
    F = np.zeros((7, 25))
    F[:] = m.h.assemble_rhs(m._f_at_quad(mesh, _f("p2"), 0, 7), 7 * 25).reshape(7, 25)
    parts = []
    for (eb, ee), data in (((0, 3), True), ((3, 7), False)):
        h = _lib.Handle(*m._handle_args[0], **m._handle_args[1])
        from hp_vpinns_amd.testfcn import tables_1d
        x, w = _rule(5)[:2]
        h.set_quadrature(x, w, x, w)
        h.set_tables(tables_1d(5, x), tables_1d(5, x))
        h.set_element_boxes(mesh.boxes, eb, ee)
        h.set_rhs(F.reshape(-1))
        h.set_active_tests_2d(mesh.nax, mesh.nay)
        if data:
            h.set_data(s["X_u_train"], s["u_train"].reshape(-1))
        h.set_params(m._to_dev(th))
        parts.append(h.loss_and_grad(True))
        ind = h.element_indicators(m._f_at_quad(mesh, _f("p2"), eb, ee))
        assert np.array_equal(ind, m.element_indicators(_f("p2"))[eb:ee])          # the shard's rows of the whole table, bit for bit
        h.close()
    (la, ga), (lb, gb) = parts
    assert lb[1] == 0.0 and rel(la[1], l3[1]) < 1e-13
    assert rel(la[2] + lb[2], l3[2]) < 1e-12 and rel(m._from_dev(ga + gb), g) < 1e-11


# ---- 3. indicators against the reference at a generic point -----------------------------------------------------------------------
def _check_columns(ind, ref):
    for c in range(5):
        n = np.linalg.norm(ref[:, c])
        err = np.linalg.norm(ind[:, c] - ref[:, c])
        print("column %d: |err| %.3e, |ref| %.3e" % (c, err, n))
        assert err <= 1e-8 * n, (c, err, n, ind[:, c], ref[:, c])


@pytest.mark.parametrize("shape", ["generic5", "auto12"])
@pytest.mark.parametrize("prob,vf", [("p2", 0), ("p2", 1), ("p2", 2), ("adv", 0), ("adv", 1)])
def test_indicators_against_the_reference_on_seven_boxes(prob, vf, shape):
    layers, _, q, _ = SHAPES[shape]
    rng = np.random.default_rng(100 + vf)
    th = theta0(layers, 31, extra=[0.7] if prob == "adv" else ())
    npar = th.size - (1 if prob == "adv" else 0)
    th[:npar] += 0.2 * rng.standard_normal(npar)        # a random network: every bias non-zero (Xavier starts them at 0)
    m, s, _ = _model(prob, vf, shape, th=th)
    mesh = _mesh7_for(prob, shape)                        # unequal counts: columns 3 and 4 differ from column 2 and from each other
    f = _f(prob)
    m.set_mesh(mesh, f)
    _need_fused(m, shape, prob, vf)
    ind = m.element_indicators(f)
    ref = ar.indicators(prob, vf, mesh, f, _rule(q), _data(prob, s), layers, th, V=0.8)
    assert ind.shape == (7, 5) and np.all(ref[:, 1:4] > 0)
    _check_columns(ind, ref)
    # column 0 is the term the training pass sums into lossv
    assert abs(ind[:, 0].sum() - m.loss()[2]) <= 1e-12 * m.loss()[2]


@pytest.mark.parametrize("vf", [1, 3])
def test_indicators_against_the_reference_1d(vf):
    from hp_vpinns_amd.adapt import ElementMesh
    from hp_vpinns_amd.drivers import poisson1d
    from hp_vpinns_amd.vpinn import VPINN1D
    layers = [1, 20, 20, 20, 1]
    s = poisson1d.setup(N_Element=3, N_testfcn=5, N_Quad=10)
    th = theta0(layers, 5) + 0.1 * np.random.default_rng(4).standard_normal(theta0(layers, 5).size)
    m = VPINN1D(s["X_u_train"], s["u_train"], s["X_quad_train"], s["W_quad_train"], s["F_ext_total"], s["grid"], s["X_u_train"],
                s["u_train"], layers, var_form=vf, init_params=th)
    mesh = ElementMesh.from_grid(s["grid"], None, [5, 3, 4])
    m.set_mesh(mesh, poisson1d.f_ext)
    ind = m.element_indicators(poisson1d.f_ext)
    rule = (s["X_quad_train"].reshape(-1), s["W_quad_train"].reshape(-1))
    ref = ar.indicators("p1", vf, mesh, poisson1d.f_ext, rule, (s["X_u_train"], s["u_train"]), layers, th)
    assert np.all(ind[:, 4] == 0.0)
    for c in range(4):
        n = np.linalg.norm(ref[:, c])
        print("column %d: |err| %.3e, |ref| %.3e" % (c, np.linalg.norm(ind[:, c] - ref[:, c]), n))
        assert np.linalg.norm(ind[:, c] - ref[:, c]) <= 1e-8 * n, (c, ind[:, c], ref[:, c])


# ---- 4. zero network: known answers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["generic5", "auto12"])
@pytest.mark.parametrize("prob", ["p2", "adv"])
def test_zero_network_known_answers_on_seven_boxes(prob, shape):
    layers, _, q, _ = SHAPES[shape]
    th = np.zeros_like(theta0(layers, 1, extra=[0.7] if prob == "adv" else ()))
    if prob == "adv":
        th[-1] = 0.7
    m, s, _ = _model(prob, 1 if prob == "p2" else 0, shape, th=th)
    mesh, f = _mesh7_for(prob, shape), _f(prob)
    m.set_mesh(mesh, f)
    _need_fused(m, shape, prob, 1 if prob == "p2" else 0)
    ind = m.element_indicators(f)
    known = ar.zero_network_indicators(mesh, f, _rule(q))         # eta2 = J sum w f^2, R = -F
    for c in range(5):
        assert np.linalg.norm(ind[:, c] - known[:, c]) <= 1e-12 * np.linalg.norm(known[:, c]), (c, ind[:, c], known[:, c])


# ---- 5. bitwise reproducibility ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["generic5", "auto12"])
def test_indicators_are_bitwise_reproducible(shape):
    m, s, th = _model("p2", 1, shape)
    mesh, f = _mesh7_for("p2", shape), _f("p2")
    m.set_mesh(mesh, f)
    _need_fused(m, shape, "p2", 1)
    a = m.element_indicators(f)
    b = m.element_indicators(f)
    assert a.tobytes() == b.tobytes()
    st = m.h.get_state()
    m._step(10, False)
    c = m.element_indicators(f)
    assert c.tobytes() != a.tobytes()
    m.h.set_state(st)
    assert m.element_indicators(f).tobytes() == a.tobytes()


# ---- 6. padded rule ---------------------------------------------------------------------------------------------------------------
def test_indicators_of_a_padded_rule_equal_those_of_the_rule_itself():
    from hp_vpinns_amd.drivers import poisson2d
    from hp_vpinns_amd.vpinn import VPINN2D
    s = poisson2d.setup(N_el_x=2, N_el_y=2, N_test_x=8, N_test_y=8, N_quad=14, N_bound=11, with_test_grid=False)
    a = (s["X_u_train"], s["u_train"], s["X_f_train"], s["f_train"], s["XY_quad_train"], s["WXY_quad_train"], None,
         s["F_ext_total"], s["grid_x"], s["grid_y"], s["N_testfcn_total"], s["X_u_train"], s["u_train"], L4)
    th = theta0(L4, 9)
    m = VPINN2D(*a, var_form=1, init_params=th)
    if m._dev_rule[0].size != 16:
        pytest.skip("the rule advice does not pad a 14 x 14 rule on this device (device rule: %d points)" % m._dev_rule[0].size)
    ind = m.element_indicators(poisson2d.f_ext)
    os.environ["HPV_NO_RULE_PADDING"] = "1"
    try:
        m0 = VPINN2D(*a, var_form=1, init_params=th)
    finally:
        os.environ.pop("HPV_NO_RULE_PADDING", None)
    assert m0._dev_rule[0].size == 14
    ind0 = m0.element_indicators(poisson2d.f_ext)
    for c in range(5):
        assert np.linalg.norm(ind[:, c] - ind0[:, c]) <= 1e-12 * np.linalg.norm(ind0[:, c]), (c, ind[:, c], ind0[:, c])


# ---- 7. set_mesh / adapt / train_adaptive -----------------------------------------------------------------------------------------
def test_set_mesh_keeps_the_state_and_a_grid_mesh_gives_the_identical_loss():
    m, s, th = _model("p2", 1, "auto12")
    from hp_vpinns_amd.drivers import poisson2d
    _need_fused(m, "auto12", "p2", 1)
    m._step(5, False)
    st, l3 = m.h.get_state(), m.loss()
    # set_mesh assembles F on the device from f; the constructor was handed the driver's host-assembled F.  For the IDENTICAL loss the
    # grid model gets that same device-assembled F through the old interface first (set_rhs; elements still from set_elements) ...
    xi, yi = m._dev_rule
    grid_mesh = m.mesh
    Fdev = m.h.assemble_rhs(m._f_at_quad(grid_mesh, poisson2d.f_ext, 0, 4), 4 * 36)
    m.h.set_rhs(Fdev)
    l3_grid, g_grid = m.loss_and_grad()
    # ... (the two assemblies agree to 1e-13, test_gpu_parity.py; the loss is quadratic in R = U - F with |F| ~ |R| this early)
    assert rel(l3_grid, l3) < 1e-11
    # ... and then the mesh equal to the constructor's grid, through set_mesh: bit for bit
    m.set_mesh(grid_mesh, poisson2d.f_ext)
    assert np.array_equal(m.h.get_state(), st)
    l3_mesh, g_mesh = m.loss_and_grad()
    assert np.array_equal(l3_mesh, l3_grid) and np.array_equal(g_mesh, g_grid)
    m.set_mesh(grid_mesh, poisson2d.f_ext)                 # a second set_mesh of the same mesh changes nothing either
    assert np.array_equal(m.loss_and_grad()[0], l3_grid) and np.array_equal(m.h.get_state(), st)
    m.set_mesh(_mesh7_for("p2", "auto12"), poisson2d.f_ext)
    assert np.array_equal(m.h.get_state(), st) and len(m.mesh) == 7


def test_indicator_buffers_follow_the_rule_when_the_padded_batch_size_stays():
    """Two rules with the same owned count whose point counts pad to the same 16-point batch: 2 elements on 5 x 5 points (50 -> 64),
    then on 6 x 5 points (60 -> 64) on the same handle.  The right-hand-side buffer of the indicators is sized by the point count."""
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.adapt import ElementMesh
    from hp_vpinns_amd.quadrature import GaussLobattoJacobiWeights
    from hp_vpinns_amd.testfcn import tables_1d
    mesh = ElementMesh([[-1.0, 0.1, -1.0, 1.0], [0.1, 1.0, -0.5, 0.5]], [4, 3], [3, 4])
    th = theta0(L4, 17) + 0.1 * np.random.default_rng(8).standard_normal(theta0(L4, 17).size)
    f = _f("p2")
    data = (np.zeros((1, 2)), np.zeros((1, 1)))
    h = _lib.Handle(_lib.PDE_POISSON2D, 1, _lib.ACT_TANH, L4)
    h.set_params(th)
    x5, w5 = GaussLobattoJacobiWeights(5, 0, 0)
    x6, w6 = GaussLobattoJacobiWeights(6, 0, 0)
    for xi, wx in ((x5, w5), (x6, w6)):
        rule = (xi, wx, x5, w5)
        h.set_active_tests_2d(None, None)
        h.set_rhs(None)
        h.set_quadrature(*rule)
        h.set_tables(tables_1d(4, xi), tables_1d(4, x5))
        h.set_element_boxes(mesh.boxes)
        P = mesh.quad_points(xi, x5)
        fq = f(P[:, 0], P[:, 1])
        h.set_rhs(h.assemble_rhs(fq, 2 * 16))
        h.set_active_tests_2d(mesh.nax, mesh.nay)
        assert h.backend_in_use() == _lib.BACKEND_MFMA
        ind = h.element_indicators(fq)
        ref = ar.indicators("p2", 1, mesh, f, rule, data, L4, th)
        _check_columns(ind, ref)
    h.close()


def test_adapt_bisects_what_mark_predicts_and_training_continues():
    from hp_vpinns_amd.adapt import mark, refine
    layers = L2
    th = np.zeros_like(theta0(layers, 1))
    loss_his = []
    m, s, _ = _model("p2", 1, "generic5", th=th, loss_his=loss_his)

    def f(x, y):      # concentrated in the quadrant x > 0, y > 0
        return 50.0 * np.exp(-40.0 * ((x - 0.5) ** 2 + (y - 0.5) ** 2))
    m.set_mesh(m.mesh, f)
    mesh = m.mesh
    known = ar.zero_network_indicators(mesh, f, _rule(5))
    want = mark(known, mesh, smooth=0.0)                  # smooth = 0: bisections only
    assert [a[0] for a in want] == [3] and want[0][1:] == ("h", "h")
    st = m.h.get_state()
    new = m.adapt(f, smooth=0.0)
    assert np.array_equal(new.boxes, refine(mesh, want).boxes) and len(new) == 7
    assert np.array_equal(m.mesh.boxes, new.boxes) and np.array_equal(m.h.get_state(), st)
    n0 = len(m.loss_his)
    rounds = m.train_adaptive(50, 25, f, max_elements=12, smooth=0.0)
    assert len(m.loss_his) == n0 + 50 and np.all(np.isfinite(m.loss_his[n0:]))
    assert len(rounds) == 1 and rounds[0][0] == 25 and 7 <= rounds[0][1] <= 12 and np.isfinite(rounds[0][2])
    assert len(m.mesh) == rounds[0][1]


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from hp_vpinns_amd._lib import HpvError
    m, s, th = _model("p2", 1, "generic5")
    l3 = m.loss_and_grad()[0]

    def refused(fn):
        with pytest.raises(HpvError) as ei:
            fn()
        assert ei.value.code < 0 and len(str(ei.value)) > len("libhpvpinn error -1: "), str(ei.value)
        assert np.array_equal(m.loss_and_grad()[0], l3)
    refused(lambda: m.h.element_indicators(np.zeros(4 * 25 - 1)))                    # wrong n
    out = np.empty(3 * 5)                                                             # wrong n_out (the binding always passes the right one)
    refused(lambda: m.h._chk(m.h.lib.hpv_element_indicators(m.h._h, None, 0, out.ctypes.data_as(C.POINTER(C.c_double)), out.size)))
    boxes = m.mesh.boxes
    bad = boxes.copy()
    bad[2, 1] = bad[2, 0]
    refused(lambda: m.h.set_element_boxes(bad))                                      # x0 >= x1
    bad = boxes.copy()
    bad[1, 3] = np.inf
    refused(lambda: m.h.set_element_boxes(bad))                                      # not finite
    refused(lambda: m.h.set_element_boxes(_mesh7("generic5").boxes))                 # F of the constructor's 4 elements, 7 boxes
    refused(lambda: m.h.set_rhs(np.zeros(7 * 25)))                                   # F of the wrong size for the list
    refused(lambda: m.h.set_active_tests_2d(np.full(7, 3), np.full(7, 3)))           # counts of the wrong length
    # the strong-form scheme
    mp, _, _ = _model("p2", 1, "generic5", scheme="PINNs")
    lp = mp.loss_and_grad()[0]
    with pytest.raises(HpvError) as ei:
        mp.h.element_indicators()
    assert ei.value.code < 0 and "variational" in str(ei.value)
    assert np.array_equal(mp.loss_and_grad()[0], lp)
