"""tests/linear_reference.py on the CPU alone: it restates the three existing problems exactly, its gradient is the derivative of its
loss, and its cases tell a wrong plane, channel or index apart (the conditions the GPU test asserts again before it reads a device
number).  No GPU needed."""
import numpy as np
import pytest

import generic_point as gp
import linear_reference as lr
from cases import rel

ORACLE_TOL = 1e-12      # what tests/test_oracle.py uses between the oracle and its fixtures


def _oracle(prob):
    import test_gpu_generic_point as T
    c = lr.SPECIAL[prob]
    s, th = T._setup(c)
    Oc, _, tup = T._classes(prob)
    o = Oc(*tup(s, c["L"]), init_params=th, **T._kw(c))
    o.vectorized = True
    return o, lr.from_setup(prob, s, c["L"], th, c["lbw"]), th


@pytest.mark.parametrize("prob", ["p2", "adv", "p1"])
def test_the_reference_restates_the_existing_problems(prob):
    """k = 1 is Poisson-2D var_form 1; kx = -eps, bx = V, by = 1 is AdvDiff var_form 1 at fixed epsilon (network blocks); 1-D k = -1
    is Poisson-1D var_form 2"""
    o, p, th = _oracle(prob)
    l3o, go = o.loss_and_grad()
    l3, g, _ = lr.reference(p)
    n = g.size
    print("%s: loss %.3e lossv %.3e gradient %.3e" % (prob, abs(l3[0] - l3o[0]) / abs(l3o[0]), abs(l3[2] - l3o[2]) / abs(l3o[2]), rel(g, go[:n])))
    assert abs(l3[0] - l3o[0]) < ORACLE_TOL * abs(l3o[0]) and abs(l3[2] - l3o[2]) < ORACLE_TOL * abs(l3o[2])
    if prob != "adv":
        assert abs(l3[1] - l3o[1]) < ORACLE_TOL * abs(l3o[1])
    assert rel(g, go[:n]) < ORACLE_TOL
    assert gp.block_rel(g, go[:n], p["layers"]) < 1e-10


@pytest.mark.parametrize("name", ["2d-h8-flux", "2d-h8-counts", "1d-sin"])
def test_gradient_against_central_differences(name):
    p = lr.problem(lr.CASES[name])
    _, g, _ = lr.reference(p)
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(4):
        d = rng.standard_normal(g.size)
        d /= np.linalg.norm(d)
        h = 1e-5
        fd = (lr.reference(p, p["theta"] + h * d)[0][0] - lr.reference(p, p["theta"] - h * d)[0][0]) / (2 * h)
        worst = max(worst, abs(fd - g @ d) / abs(g @ d))
    print(name, "directional derivative against central differences: %.2e" % worst)
    assert worst < 1e-6       # h^2 |f'''| / 6 ~ 1e-10 plus rounding eps |f| / h ~ 1e-10, relative to |g . d| ~ 1 and above


@pytest.mark.parametrize("name", list(lr.CASES))
def test_conditions_on_the_reference_alone(name):
    p = lr.problem(lr.CASES[name])
    fig = lr.conditions(p)
    print(name, fig)
    R = lr.var_part(p)["R"]
    if p["nax"] is not None:
        nax = p["nax"][p["eb"]:p["ee"]]
        assert all(np.all(R[e][:, nax[e]:] == 0.0) for e in range(R.shape[0]))
    # a zero-weight padding point carries no weight in the reference either: the padded rule integrates what the rule itself does
    assert all(np.isfinite(v) for v in (fig["block_share"], fig["plane"]))


def test_padded_rule_equals_the_rule_itself():
    """21 x 21 with one zero-weight point per direction against the same planes without those points"""
    c = lr.CASES["lds-21x21-padded"]
    p = lr.problem(c)
    q = dict(p, xr=lr.rule(20), yr=lr.rule(20))
    ne = p["ee"] - p["eb"]
    q["planes"] = np.ascontiguousarray(p["planes"].reshape(5, ne, 21, 21)[:, :, :20, :20]).reshape(5, -1)
    a, b = lr.var_part(p), lr.var_part(q)
    assert abs(a["lossv"] - b["lossv"]) < 1e-13 * abs(b["lossv"]) and rel(a["grad"], b["grad"]) < 1e-12
