"""tests/data_term_reference.py (the expected values of tests/test_gpu_data_term.py) on the CPU:

  * var_part + data_part equals the oracle's own full loss_and_grad -- on the three small fixtures and on one generic-point handle per
    problem, with a NEW data set of 37 interior points -- within the bound at which tests/test_oracle.py holds two evaluations of the
    oracle equal (`_same` there: the triple within 1e-12 |loss|, the gradient within 1e-11 max |g|);
  * data_part's gradient against central differences in every parameter, step and bound as tests/test_validation_host.py derives
    them for its channels:  (f(t + h) - f(t - h)) / 2h = f' + h^2 f'''(xi) / 6 + rounding <= eps F / h, with f''' from autograd at
    the point (doubled: it moves by O(h) of itself across the step) and F = 2 |f|, the rounding term doubled for the evaluation error;
  * conditions (a) - (c) of the reference module hold for every launch structure of the GPU file at every point count of its sweep
    (static workgroup counts; the GPU file reads them from the device and asserts the conditions again)."""
import numpy as np
import pytest
import torch

import data_term_reference as dr
import generic_point as gp
import validation_reference as vr
from cases import gold, p1_args, p2_args, p3_args

H = 1e-3
EPS = 2.0 ** -53
LOSS_EQ, GRAD_EQ = 1e-12, 1e-11          # tests/test_oracle.py::_same
TOL = 1e-9                               # the gradient-block bound of tests/test_gpu_generic_point.py (asserted equal below)


def _oracle(prob):
    from oracle import vpinn_oracle as O
    return {"p1": O.OracleVPINN1D, "p2": O.OracleVPINN2D, "adv": O.OracleVPINNAdvDiff}[prob]


def _fixture(prob):
    if prob == "p1":
        a = list(p1_args(gold("poisson1d_small")))
        return a, a[8], dict(var_form=1, lossb_weight=3), 3.0
    if prob == "p2":
        a = list(p2_args(gold("poisson2d_small")))
        return a, a[13], dict(var_form=1, lossb_weight=3), 3.0
    a = list(p3_args(gold("advdiff_small")))
    return a, a[12], dict(var_form=0, V=0.6, lossb_weight=3), 3.0


def _generic_handle(prob):
    import test_gpu_generic_point as T
    c = dr.case_of({"p1": "tile-1d", "p2": "fused-unsplit", "adv": "tile-2d"}[prob])
    s, th = T._setup(c)
    a = list(T._classes(prob)[2](s, c["L"]))
    return a, c["L"], T._kw(c), float(c["lbw"]), th


@pytest.mark.parametrize("where", ["fixture", "generic-point"])
@pytest.mark.parametrize("prob", ["p1", "p2", "adv"])
def test_decomposition_equals_the_oracle(prob, where):
    if where == "fixture":
        a, L, kw, w = _fixture(prob)
        th = gp.generic_theta(L, 7300 + len(prob), extra=[0.9] if prob == "adv" else ())
    else:
        a, L, kw, w, th = _generic_handle(prob)
    a[1] = np.asarray(a[1], dtype=np.float64).reshape(-1, 1)
    o = _oracle(prob)(*a, init_params=th, **kw)
    o.vectorized = True
    var = dr.var_part(o, prob, L, th, a[0], a[1], w)
    assert abs(var["full"][0][0] - (var["lossv"] + var["data_full"]["wmsq"])) < LOSS_EQ * abs(var["full"][0][0])
    X = dr.points(prob, 37, 7400)
    u = dr.targets(prob, L, th, X, 7400)
    l3, g = dr.reference(prob, var, dr.data_part(prob, L, th, X, u, w))
    o2 = _oracle(prob)(*dr.with_data(None, a, X, u), init_params=th, **kw)
    o2.vectorized = True
    l3o, go = o2.loss_and_grad()
    print(prob, where, "triple", l3, l3o, "gradient", np.abs(g - go).max() / np.abs(go).max())
    assert np.abs(l3 - np.array(l3o)).max() < LOSS_EQ * abs(l3o[0]), (l3, l3o)
    assert np.abs(g - go).max() < GRAD_EQ * np.abs(go).max()
    # ... and no data at all is the variational part alone
    l0, g0 = dr.reference(prob, var, dr.data_part(prob, L, th, X[:0], u[:0], w))
    assert l0[1] == 0.0 and l0[0] == l0[2] == var["lossv"] and np.array_equal(g0, var["grad"])


@pytest.mark.parametrize("prob", ["p1", "p2", "adv"])
def test_data_gradient_against_central_differences(prob):
    L = [1, 5, 1] if prob == "p1" else [2, 5, 5, 1]
    th = gp.generic_theta(L, 7500 + len(prob), extra=[0.8] if prob == "adv" else ())
    X = dr.points(prob, 10, 7600)
    u = dr.targets(prob, L, th, X, 7600)
    w = 3.0
    d = dr.data_part(prob, L, th, X, u, w)
    assert abs(d["wmsq"] - w * d["msq"]) <= 1e-15 * d["wmsq"] and 0.25 <= d["msq"] <= 2.25
    Xt, ut = torch.tensor(X), torch.tensor(u)

    def f(theta):
        o = vr.bare_oracle(prob, L, th)
        return w * torch.mean(torch.square(ut - o.neural_net(Xt, theta)))

    P = th.size
    n_net = P - dr.n_extra(prob)
    worst = 0.0
    for i in range(P):
        t = torch.tensor(th, requires_grad=True)
        d1 = torch.autograd.grad(f(t), t, create_graph=True)[0][i]
        if i >= n_net:                                   # epsilon: the data term does not know it
            assert d["grad"][i] == 0.0 and float(d1.detach()) == 0.0
            continue
        d2 = torch.autograd.grad(d1, t, create_graph=True)[0][i]
        m3 = 2.0 * abs(float(torch.autograd.grad(d2, t)[0][i]))
        e = np.zeros(P); e[i] = H
        with torch.no_grad():
            fp, fm, f0 = float(f(torch.tensor(th + e))), float(f(torch.tensor(th - e))), float(f(torch.tensor(th)))
        bound = H ** 2 * m3 / 6 + 2 * EPS * (2.0 * abs(f0)) / H
        err = abs((fp - fm) / (2 * H) - d["grad"][i])
        worst = max(worst, err / bound)
        assert bound < 1e-4 * max(1.0, abs(d["grad"][i])) and err <= bound, (prob, i, err, bound, d["grad"][i])
    print(prob, "data gradient against central differences: worst error / bound %.3f" % worst)


def _var_gradient(name):
    """the variational gradient of a structure's case from the CPU oracle (the 80x80-point elements included: once, vectorised)"""
    import test_gpu_generic_point as T
    c = dr.case_of(name)
    s, th = T._setup(c)
    a = list(T._classes(c["prob"])[2](s, c["L"]))
    a[1] = np.asarray(a[1], dtype=np.float64).reshape(-1, 1)
    o = _oracle(c["prob"])(*a, init_params=th, **T._kw(c))
    o.vectorized = True
    X0, u0 = dr.start_data(c, s)
    return c, th, dr.var_part(o, c["prob"], c["L"], th, X0, u0, float(c["lbw"]))


@pytest.mark.parametrize("name", sorted(dr.STRUCTURES))
def test_conditions_hold_for_every_case(name):
    import test_gpu_generic_point as T
    assert T.TOL == TOL
    spec = dr.STRUCTURES[name]
    c, th, var = _var_gradient(name)
    counts = sorted({n for n, _ in dr.sweep_counts(spec) if n > 0})
    X = dr.points(c["prob"], max(counts), spec["seed"])
    u = dr.targets(c["prob"], c["L"], th, X, spec["seed"])
    for n in counts:
        f = dr.conditions(c["prob"], c["L"], th, X[:n], u[:n], float(c["lbw"]), var["grad"], TOL)
        # the TOTAL gradient's blocks (epsilon's among them) stand above the floor: block_errors asserts it
        gt = var["grad"] + dr.data_part(c["prob"], c["L"], th, X[:n], u[:n], float(c["lbw"]))["grad"]
        gp.block_errors(gt, gt, c["L"], dr.n_extra(c["prob"]))
        print("%s n = %d: smallest data block %.2e of the gradient, data share %.2e, leave-one-out %s"
              % (name, n, f["block_share"], f["share"], "%.2e" % f["loo"] if f["loo"] is not None else "(loss: 1/(9n) = %.1e)" % (1 / (9.0 * n))))
    # no data: a block the variational gradient does not have (the output bias, where the form holds derivatives of u only) is
    # compared absolutely
    e = dr.without_data_errors(var["grad"], var["grad"], c["L"], dr.n_extra(c["prob"]))
    assert e and max(e.values()) == 0.0


@pytest.mark.parametrize("backend", ["generic", "mfma"])
@pytest.mark.parametrize("prob", ["p1", "p2", "adv"])
def test_conditions_hold_for_the_pinn_scheme_cases(prob, backend):
    o, a, L, th = dr.pinn_case(prob, backend)
    var = dr.var_part(o, prob, L, th, a[0], a[1], dr.PINN_W[prob])
    counts = dr.DATA_LOSS_COUNTS if backend == "generic" else dr.PINN_MFMA_COUNTS
    X = dr.points(prob, max(counts), 9400)
    u = dr.targets(prob, L, th, X, 9400)
    for n in counts:
        f = dr.conditions(prob, L, th, X[:n], u[:n], dr.PINN_W[prob], var["grad"], TOL)
        gt = var["grad"] + dr.data_part(prob, L, th, X[:n], u[:n], dr.PINN_W[prob])["grad"]
        gp.block_errors(gt, gt, L, dr.n_extra(prob))
        print(prob, backend, n, f)


def test_conditions_hold_for_the_small_generic_case():
    import test_gpu_generic_point as T
    c = dr.small_generic_case()
    s, th = T._setup(c)
    a = list(T._classes("p2")[2](s, c["L"]))
    o = _oracle("p2")(*a, init_params=th, **T._kw(c))
    o.vectorized = True
    var = dr.var_part(o, "p2", c["L"], th, a[0], a[1], 3.0)
    X = dr.points("p2", max(dr.DATA_LOSS_COUNTS), c["seed"])
    u = dr.targets("p2", c["L"], th, X, c["seed"])
    for n in dr.DATA_LOSS_COUNTS:
        f = dr.conditions("p2", c["L"], th, X[:n], u[:n], 3.0, var["grad"], TOL)
        gt = var["grad"] + dr.data_part("p2", c["L"], th, X[:n], u[:n], 3.0)["grad"]
        gp.block_errors(gt, gt, c["L"], 0)
        print("generic-small", n, f)
