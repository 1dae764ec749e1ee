"""Host half of the local hp-refinement (hp_vpinns_amd/adapt.py) and of its reference (tests/adapt_reference.py): no GPU."""
import numpy as np
import pytest

import adapt_reference as ar
from cases import rel, theta0
from hp_vpinns_amd.adapt import ETA2, ElementMesh, mark, refine
from hp_vpinns_amd.quadrature import GaussLobattoJacobiWeights


def seven_boxes():
    """a 2 x 2 grid on [-1, 1]^2 whose element 1 (left-upper) is split in four, with unequal counts"""
    m = ElementMesh.from_grid([-1.0, 0.0, 1.0], [-1.0, 0.0, 1.0], [4, 5], [3, 5])
    m.split(1, None)
    m.nax[:] = [4, 3, 5, 2, 4, 5, 5]
    m.nay[:] = [3, 5, 2, 4, 3, 3, 5]
    return m


# ---- ElementMesh ------------------------------------------------------------------------------------------------------------------
def test_from_grid_order_is_ex_times_ney_plus_ey():
    m = ElementMesh.from_grid([0.0, 1.0, 3.0], [10.0, 11.0, 12.0, 14.0], [2, 3], [4, 5, 6])
    assert len(m) == 6 and m.dim == 2
    for ex in range(2):
        for ey in range(3):
            e = ex * 3 + ey
            assert list(m.boxes[e]) == [[0.0, 1.0, 3.0][ex], [0.0, 1.0, 3.0][ex + 1], [10.0, 11.0, 12.0, 14.0][ey], [10.0, 11.0, 12.0, 14.0][ey + 1]]
            assert m.nax[e] == [2, 3][ex] and m.nay[e] == [4, 5, 6][ey]
    m1 = ElementMesh.from_grid([0.0, 1.0, 3.0], None, 7)
    assert m1.dim == 1 and list(m1.nax) == [7, 7] and list(m1.nay) == [1, 1] and m1.boxes.tolist() == [[0.0, 1.0], [1.0, 3.0]]


def test_splits_conserve_area_and_children_replace_the_parent_in_order():
    m = ElementMesh.from_grid([-1.0, 0.0, 1.0], [-1.0, 0.0, 1.0], [4, 5], [3, 5])
    a0 = m.area()
    assert m.split(1, None) == 4 and len(m) == 7 and m.area() == a0
    # left-lower, left-upper, right-lower, right-upper of the parent [-1, 0] x [0, 1]; the later elements moved up
    assert m.boxes[1:5].tolist() == [[-1, -0.5, 0, 0.5], [-1, -0.5, 0.5, 1], [-0.5, 0, 0, 0.5], [-0.5, 0, 0.5, 1]]
    assert m.boxes[0].tolist() == [-1, 0, -1, 0] and m.boxes[5].tolist() == [0, 1, -1, 0] and m.boxes[6].tolist() == [0, 1, 0, 1]
    assert list(m.nax) == [4, 4, 4, 4, 4, 5, 5] and list(m.nay) == [3, 5, 5, 5, 5, 3, 5]      # children inherit
    assert m.split(0, 0) == 2 and m.boxes[0:2].tolist() == [[-1, -0.5, -1, 0], [-0.5, 0, -1, 0]] and m.area() == a0
    assert m.split(7, 1) == 2 and m.boxes[7:9].tolist() == [[0, 1, 0, 0.5], [0, 1, 0.5, 1]] and m.area() == a0
    m1 = ElementMesh.from_grid([0.0, 1.0, 3.0], None, 7)
    assert m1.split(1, None) == 2 and m1.boxes.tolist() == [[0, 1], [1, 2], [2, 3]] and m1.area() == 3.0
    with pytest.raises(ValueError):
        m1.split(0, 1)


def test_raise_p_clamps():
    m = seven_boxes()
    assert m.raise_p(0, 0, 5) and m.nax[0] == 5
    assert not m.raise_p(0, 0, 5) and m.nax[0] == 5
    assert not m.raise_p(2, 0, 5) and m.raise_p(2, 1, 3) and m.nay[2] == 3 and not m.raise_p(2, 1, 3)


def test_quad_points_layout_and_expression():
    m = seven_boxes()
    xi, _ = GaussLobattoJacobiWeights(5, 0, 0)
    yi, _ = GaussLobattoJacobiWeights(4, 0, 0)
    P = m.quad_points(xi, yi).reshape(7, 4, 5, 2)            # [e][j][i]
    for e in (0, 3, 6):
        b = m.boxes[e]
        for j in range(4):
            for i in range(5):
                assert P[e, j, i, 0] == b[0] + (b[1] - b[0]) / 2 * (xi[i] + 1) and P[e, j, i, 1] == b[2] + (b[3] - b[2]) / 2 * (yi[j] + 1)
    assert np.array_equal(m.quad_points(xi, yi, 2, 5), P[2:5].reshape(-1, 2))


# ---- mark: hand-made tables with known answers ------------------------------------------------------------------------------------
def _table(eta, topx=0.5, topy=0.5):
    t = np.zeros((len(eta), 5))
    t[:, ETA2] = eta
    t[:, 2] = 1.0
    t[:, 3], t[:, 4] = topx, topy
    return t


def test_mark_prefix_rule_and_tie_order():
    m = seven_boxes()
    # total 20; theta 0.5 needs 10: 6 (e 2) + 4 = 10 -- of the two 4s the lower index (e 1) is taken, e 5 is not
    t = _table([1, 4, 6, 2, 2, 4, 1])
    assert [a[0] for a in mark(t, m, theta=0.5)] == [1, 2]
    assert [a[0] for a in mark(t, m, theta=0.51)] == [1, 2, 5]
    assert [a[0] for a in mark(t, m, theta=0.3)] == [2]
    assert [a[0] for a in mark(t, m, theta=1.0)] == [0, 1, 2, 3, 4, 5, 6]
    assert mark(_table([0] * 7), m) == []
    assert all(a[1:] == ("h", "h") for a in mark(t, m, theta=1.0))          # top / sumR2 = 0.5 >= smooth everywhere


def test_mark_smooth_switch_per_axis_and_p_max():
    m = seven_boxes()                       # nax [4 3 5 2 4 5 5], nay [3 5 2 4 3 3 5]
    t = _table([9, 8, 7, 0, 0, 0, 0], topx=[0.01, 0.5, 0.01, 0, 0, 0, 0], topy=[0.5, 0.01, 0.01, 0, 0, 0, 0])
    got = mark(t, m, theta=1.0, smooth=0.1, p_max=5)
    # e 0: x decayed, room (4 < 5) -> p; y not decayed -> h.  e 1: x not decayed -> h; y decayed but nay = 5 = p_max -> h.
    # e 2: x decayed but nax = 5 = p_max -> h; y decayed, room -> p
    assert got == [(0, "p", "h"), (1, "h", "h"), (2, "h", "p")]
    assert mark(t, m, theta=1.0, smooth=0.001, p_max=5) == [(0, "h", "h"), (1, "h", "h"), (2, "h", "h")]
    new = refine(m, got, p_max=5)
    assert len(new) == 7 + 1 + 3 + 1 and new.area() == m.area()
    assert list(new.nax[0:2]) == [5, 5] and list(new.nay[0:2]) == [3, 3]           # e 0 bisected in y, both children raised in x
    assert list(new.nax[2:6]) == [3] * 4 and list(new.nay[2:6]) == [5] * 4         # e 1 in four
    assert list(new.nax[6:8]) == [5, 5] and list(new.nay[6:8]) == [3, 3]           # e 2 bisected in x, raised in y
    assert len(m) == 7                                                             # the input mesh is left alone


def test_mark_never_exceeds_max_elements():
    m = seven_boxes()
    t = _table([9, 8, 7, 1, 1, 1, 1])
    for cap in (7, 8, 9, 10, 11, 13, 16, 100):
        got = mark(t, m, theta=0.85, max_elements=cap)
        assert len(refine(m, got)) <= cap, cap
    assert mark(t, m, theta=0.85, max_elements=7) == []
    assert mark(t, m, theta=0.85, max_elements=8) == [(0, "h", None)]               # one bisection fits, in x
    assert mark(t, m, theta=0.85, max_elements=11) == [(0, "h", "h"), (1, "h", None)]
    assert len(refine(m, mark(t, m, theta=0.85))) == 7 + 9


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _f2(x, y):
    return np.sin(2.0 * x + 0.3) * np.cos(1.5 * y) + 0.5 * x * y


def _rule(q):
    x, w = GaussLobattoJacobiWeights(q, 0, 0)
    return x, w, x.copy(), w.copy()


def _data2(n=9, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, 2))
    return X, np.sin(X[:, 0:1]) * X[:, 1:2]


@pytest.mark.parametrize("prob,vf", [("p2", 0), ("p2", 1), ("p2", 2), ("adv", 0), ("adv", 1)])
def test_reference_of_one_box_is_the_oracle_on_a_1x1_grid(prob, vf):
    from oracle.vpinn_oracle import OracleVPINN2D, OracleVPINNAdvDiff
    layers, rule, data = [2, 5, 5, 1], _rule(5), _data2()
    mesh = ElementMesh([[-0.5, 0.25, 0.0, 1.0]], 4, 3)
    th = theta0(layers, 11, extra=[0.7] if prob == "adv" else ())
    F = ar.f_blocks(mesh, _f2 if prob == "p2" else None, *rule)
    l3, g = ar.box_loss_and_grad(prob, vf, mesh, F, rule, data, layers, th, V=0.8)
    XY, W = ar._rule2d(*rule)
    if prob == "p2":
        o = OracleVPINN2D(data[0], data[1], np.zeros((1, 2)), np.zeros((1, 1)), XY, W, None, F[0].reshape(1, 1, 3, 4), [-0.5, 0.25],
                          [0.0, 1.0], [[4], [3]], None, None, layers, var_form=vf, init_params=th)
    else:
        o = OracleVPINNAdvDiff(data[0], data[1], None, XY, W, None, None, [-0.5, 0.25], [0.0, 1.0], [[4], [3]], None, None, layers,
                               None, None, var_form=vf, V=0.8, init_params=th)
    l3o, go = o.loss_and_grad()                  # the reference-structured element loop
    assert rel(l3, l3o) < 1e-12 and rel(g, go) < 1e-12, (l3, l3o, rel(g, go))


def test_reference_box_list_of_a_grid_is_the_oracle_on_that_grid():
    from oracle.vpinn_oracle import OracleVPINN2D
    layers, rule, data = [2, 5, 5, 1], _rule(5), _data2()
    gx, gy = [-1.0, 0.2, 1.0], [-1.0, -0.1, 1.0]
    mesh = ElementMesh.from_grid(gx, gy, [4, 3], [2, 3])
    th = theta0(layers, 12)
    F = ar.f_blocks(mesh, _f2, *rule)
    blocks = np.empty((2, 2), dtype=object)
    for e in range(4):
        blocks[e // 2, e % 2] = F[e]
    XY, W = ar._rule2d(*rule)
    o = OracleVPINN2D(data[0], data[1], np.zeros((1, 2)), np.zeros((1, 1)), XY, W, None, blocks, gx, gy, [[4, 3], [2, 3]], None, None,
                      layers, var_form=1, init_params=th)
    l3o, go = o.loss_and_grad()
    l3, g = ar.box_loss_and_grad("p2", 1, mesh, F, rule, data, layers, th)
    assert rel(l3, l3o) < 1e-12 and rel(g, go) < 1e-12
    # shard additivity of the reference itself
    la, ga = ar.box_loss_and_grad("p2", 1, mesh, F, rule, data, layers, th, e_range=(0, 1))
    lb, gb = ar.box_loss_and_grad("p2", 1, mesh, F, rule, data, layers, th, e_range=(1, 4), use_data=False)
    assert rel(la[2] + lb[2], l3[2]) < 1e-13 and rel(ga + gb, g) < 1e-13 and lb[1] == 0.0


@pytest.mark.parametrize("prob", ["p1", "p2", "adv"])
def test_zero_network_eta2_is_J_sum_w_f_squared(prob):
    if prob == "p1":
        layers, mesh = [1, 5, 5, 1], ElementMesh.from_grid([-1.0, -0.2, 0.3, 1.0], None, [4, 5, 3])
        x, w = GaussLobattoJacobiWeights(6, 0, 0)
        rule, f = (x, w), (lambda x: np.cos(3.0 * x) + x)
        data = (np.array([[-1.0], [1.0]]), np.zeros((2, 1)))
    else:
        layers, mesh, rule, f, data = [2, 5, 5, 1], seven_boxes(), _rule(5), _f2, _data2()
    th = np.zeros_like(theta0(layers, 1, extra=[0.7] if prob == "adv" else ()))
    if prob == "adv":
        th[-1] = 0.7
    vf = 1 if prob != "adv" else 0
    ind = ar.indicators(prob, vf, mesh, f, rule, data, layers, th)
    known = ar.zero_network_indicators(mesh, f, rule)
    # eta2 computed directly: J sum_q w_q f(x_q)^2
    for e in range(len(mesh)):
        P = mesh.quad_points(rule[0], rule[2] if mesh.dim == 2 else None, e, e + 1)
        wq = rule[1] if mesh.dim == 1 else (rule[1][None, :] * rule[3][:, None]).reshape(-1)
        direct = mesh.jacobians()[e] * float((wq * f(*[P[:, c] for c in range(mesh.dim)]) ** 2).sum())
        assert abs(ind[e, ETA2] - direct) <= 1e-14 * direct, (e, ind[e, ETA2], direct)
    assert rel(ind, known) < 1e-13
    assert np.all(ind[:, 4] == 0.0) if prob == "p1" else np.all(ind[:, 4] > 0.0)
