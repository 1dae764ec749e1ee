"""tests/flux_reference.py proved on the CPU (no GPU): the conditions every case of tests/test_gpu_flux.py rests on, asserted on the
reference alone; flux_part's gradient against central differences of flux_part's loss (step and bound of
tests/test_data_term_host.py); and a = 1, b = 0, g = u_d, w_f = lossb_weight reproducing data_term_reference.data_part."""
import numpy as np
import pytest
import torch

import data_term_reference as dr
import flux_reference as fr
import generic_point as gp
import validation_reference as vr
from test_data_term_host import EPS, H, TOL


def _check_counts(prob, L, th, g_rest_with, g_rest_without, f, counts):
    for n in sorted(set(counts)):
        for g_rest, what in ((g_rest_with, "with Dirichlet data"), (g_rest_without, "without")):
            fig = fr.conditions(prob, L, th, fr.head(f, n), g_rest, TOL)
            print("%s n = %d %s: %s" % (prob, n, what, fig))


@pytest.mark.parametrize("name", list(fr.STRUCTURES))
def test_conditions_hold_for_every_structure(name):
    import test_gpu_generic_point as T
    assert T.TOL == TOL
    c = fr.STRUCTURES[name]
    o, a, th = fr.oracle_of(c)
    var = dr.var_part(o, c["prob"], c["L"], th, a[0], a[1], float(c["lbw"]))
    _check_counts(c["prob"], c["L"], th, var["full"][1], var["grad"], fr.sweep_data(c["prob"], c["L"], th), fr.SWEEP)
    if name == "generic":      # the grid-stride case runs on this handle
        f = fr.flux_data(c["prob"], c["L"], th, fr.LARGE_N, fr.LARGE_SEED)
        _check_counts(c["prob"], c["L"], th, var["full"][1], var["grad"], f, [fr.LARGE_N])


@pytest.mark.parametrize("prob", fr.PINN)
def test_conditions_hold_for_the_strong_form_cases(prob):
    o, a, L, th = dr.pinn_case(prob, "mfma")
    var = dr.var_part(o, prob, L, th, a[0], a[1], dr.PINN_W[prob])
    _check_counts(prob, L, th, var["full"][1], var["grad"], fr.sweep_data(prob, L, th), fr.SWEEP)


@pytest.mark.parametrize("prob", ["p1", "p2", "adv"])
def test_flux_gradient_against_central_differences(prob):
    L = [1, 5, 1] if prob == "p1" else [2, 5, 5, 1]
    th = gp.generic_theta(L, 7500 + len(prob), extra=[0.8] if prob == "adv" else ())
    fd = fr.flux_data(prob, L, th, 10, 7600)
    d = fr.flux_part(prob, L, th, fd)
    assert abs(d["wmsf"] - fr.W_F * d["msf"]) <= 1e-15 * d["wmsf"] and 0.25 <= d["msf"] <= 2.25
    at, bt, gt = torch.tensor(fd["a"]), torch.tensor(fd["b"]), torch.tensor(fd["g"])

    def f(theta):
        o = vr.bare_oracle(prob, L, th)
        Xt = torch.tensor(fd["X"], requires_grad=True)
        u = o.neural_net(Xt, theta)
        du, = torch.autograd.grad(u, Xt, grad_outputs=torch.ones_like(u), create_graph=True)
        return fr.W_F * torch.mean(torch.square(at * u.reshape(-1) + torch.sum(bt * du, dim=1) - gt))

    P = th.size
    n_net = P - dr.n_extra(prob)
    worst = 0.0
    for i in range(P):
        t = torch.tensor(th, requires_grad=True)
        d1 = torch.autograd.grad(f(t), t, create_graph=True)[0][i]
        if i >= n_net:                                   # epsilon: the flux term does not know it
            assert d["grad"][i] == 0.0 and float(d1.detach()) == 0.0
            continue
        d2 = torch.autograd.grad(d1, t, create_graph=True)[0][i]
        m3 = 2.0 * abs(float(torch.autograd.grad(d2, t)[0][i]))
        e = np.zeros(P); e[i] = H
        fp, fm, f0 = float(f(torch.tensor(th + e))), float(f(torch.tensor(th - e))), float(f(torch.tensor(th)))
        bound = H ** 2 * m3 / 6 + 2 * EPS * (2.0 * abs(f0)) / H
        err = abs((fp - fm) / (2 * H) - d["grad"][i])
        worst = max(worst, err / bound)
        assert bound < 1e-4 * max(1.0, abs(d["grad"][i])) and err <= bound, (prob, i, err, bound, d["grad"][i])
    print(prob, "flux gradient against central differences: worst error / bound %.3f" % worst)


@pytest.mark.parametrize("prob", ["p1", "p2", "adv"])
def test_value_only_flux_term_is_the_data_term(prob):
    L = [1, 20, 20, 1] if prob == "p1" else [2, 20, 20, 1]
    th = gp.generic_theta(L, 7700 + len(prob), extra=[0.8] if prob == "adv" else ())
    X = dr.points(prob, 17, 7800)
    u = dr.targets(prob, L, th, X, 7800)
    w = 3.0
    d = dr.data_part(prob, L, th, X, u, w)
    f = dict(X=X, a=np.ones(17), b=np.zeros_like(X), g=u.reshape(-1))
    fp = fr.flux_part(prob, L, th, f, w)
    assert abs(fp["msf"] - d["msq"]) <= 1e-13 * d["msq"] and abs(fp["wmsf"] - d["wmsq"]) <= 1e-13 * d["wmsq"]
    assert np.max(np.abs(fp["grad"] - d["grad"])) <= 1e-13 * np.max(np.abs(d["grad"]))


def test_adam_trajectory_without_flux_data_is_the_oracles_own():
    """the numpy restatement of the update rule in flux_reference.adam_trajectory against oracle.adam_step"""
    c = fr.STRUCTURES["generic"]
    o1, _, th = fr.oracle_of(c)
    o2, _, _ = fr.oracle_of(c)
    for _ in range(4):
        o1.adam_step()
    p = fr.adam_trajectory(o2, c["prob"], c["L"], None, 4)
    assert np.max(np.abs(p - o1.get_params())) <= 1e-14 * np.max(np.abs(p))
