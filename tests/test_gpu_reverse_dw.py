"""Phase R of k_iter_fused, the weight-gradient operands of the two-channel reverse tile (csrc/kernels_fused.hip, rev_tile without a
second tangent): the inputs h_{i-1} = s and hdot_{i-1} = s'(z_{i-1}) z_d,{i-1} of EVERY hidden layer go into the per-wave transpose
tiles once per tile, behind the tangent recompute (layer 3's and layer 2's side by side: tiles 2..5 of the six), only zbar follows the
adjoint chain (tiles 0, 1), and both channels' operands of a layer are read back in one round trip under the hbar chain.  That text
runs with three hidden layers and one workgroup per element or more (DWE in rev_tile); L = 2 and SPLIT keep the per-layer transposes,
and the cases on them pin that the switch between the two texts selects a complete one.

As tests/test_gpu_forward_adjoint.py: Poisson-2D var_form 1 on warped grids, Xavier + 0.3 N(0,1) on every weight and bias
(tests/generic_point.py), against oracle/vpinn_oracle.py (vectorised): the loss triple, the element losses, the full gradient and every
residual at TOL of test_gpu_parity.py, two calls of loss_and_grad() bit-equal (the order of the sums depends on nothing but the text).
Every case asserts through hpv_pass_structure / hpv_kernel_variant that k_iter_fused ran in the wanted plan.  One oracle evaluation
per problem, shared by the cases that run on it.

What the cases are for:
  L = 3 / L = 2   two layers' inputs side by side in the transpose region / the per-layer text
  quarter-tile    2 x 2 elements of 20 x 20 points, 10 x 10 test functions, one workgroup per element: six whole tiles per wave, the data
                  points ride in the packed quarter tile, whose reverse uses tiles 0, 1 of the same region behind the last whole tile
  whole-tile      2 x 2 elements of 12 x 12 points without the quarter tile: 9 element tiles + a data tile on four waves -- waves with
                  three and with two tiles; the data tile carries an adjoint on the value channel and zeros on the tangent
  split           ONE shard of 2 elements, several workgroups per element: a wave owns one tile or none (the per-layer text)
  trajectory      50 TF1-Adam steps on the quarter-tile case against the oracle's adam_step, final parameters to TRAJ_TOL
  bitwise         two passes from the same parameters in one process: gradient, loss triple and residuals byte-equal"""
import functools

import numpy as np
import pytest

import generic_point as gp
from cases import rel
from test_gpu_parity import TOL, TRAJ_TOL
from test_gpu_proj_phase import _classes, _compare, _compiled_out

pytestmark = pytest.mark.gpu

LAYERS = {2: [2, 20, 20, 1], 3: [2, 20, 20, 20, 1]}
# plan -> (elements in x, in y, points per direction, test functions per direction, seed)
PLANS = {"quarter-tile": (2, 2, 20, 10, 1320), "whole-tile": (2, 2, 12, 6, 1312), "split": (2, 1, 20, 10, 1302)}


@pytest.fixture(autouse=True)
def _plan_environment(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def _problem(plan, nl):
    """(constructor arguments, parameters, the oracle's loss triple, gradient and residuals) of one problem; read-only"""
    from hp_vpinns_amd.drivers import poisson2d
    nex, ney, q, nt, seed = PLANS[plan]
    s = poisson2d.setup(N_el_x=nex, N_el_y=ney, N_test_x=nt, N_test_y=nt, N_quad=q, N_bound=13, with_test_grid=False)
    s = gp.warp_poisson2d(s, seed, F="random")
    a = gp.p2_tuple(s, LAYERS[nl])
    th = gp.generic_theta(LAYERS[nl], seed + nl)
    o = _classes("p2")[0](*a, init_params=th, var_form=1)
    o.vectorized = True
    l3o, go = o.loss_and_grad()
    l3o = np.asarray(l3o, dtype=np.float64)
    R = np.array(o.last["R"], dtype=np.float64)
    for x in (th, l3o, go, R):
        x.setflags(write=False)
    return a, th, l3o, go, R


def _model(monkeypatch, plan, nl):
    """the device model of a problem in its plan, and what its kernel variant must say"""
    nex, ney, q, nt, _ = PLANS[plan]
    a, th, _, _, _ = _problem(plan, nl)
    if plan != "split":
        monkeypatch.setenv("HPV_FUSE", "i")            # one workgroup per element also on the 2 x 2 grid
    if plan == "whole-tile":
        monkeypatch.setenv("HPV_NO_QUARTER_TILE", "1")
    m = _classes("p2")[1](*a, init_params=th.copy(), var_form=1)
    # (no skip: the text under test raised the compiler's register need, and a guard that compiled it out must show here)
    assert not _compiled_out(m, False, False), "the build guard compiled this instantiation out: %s" % (m.h.build_info(),)
    want = ["k_iter_fused<L=%d,SPLIT=%s," % (nl, "true" if plan == "split" else "false")]
    if plan == "whole-tile":
        want += ["QT=false", ",%dx%d/%dx%d>" % (q, q, nt, nt)]
    if plan == "quarter-tile":
        want += ["QT=true"]
    return m, want, "whole-iteration-split" if plan == "split" else "whole-iteration"


@pytest.mark.parametrize("nl", [3, 2], ids=["L3", "L2"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_reverse_dw_one_pass_against_the_oracle(monkeypatch, plan, nl):
    nex, ney, _, nt, _ = PLANS[plan]
    _, _, l3o, go, R = _problem(plan, nl)
    m, want, structure = _model(monkeypatch, plan, nl)
    name = "%s-L%d" % (plan, nl)
    _, gm, _ = _compare(name, m, l3o, go, R, [nt * nt] * (nex * ney), want, structure, 0)
    # the hidden layers' weight blocks on their own: what the transposed operands feed (blocks(): weight, bias per layer)
    worst = gp.worst_block(gm, go, LAYERS[nl])
    print("%s | worst block %s" % (name, (worst,)))
    assert gp.block_rel(gm, go, LAYERS[nl]) < TOL, (name, worst)


def test_reverse_dw_trajectory(monkeypatch):
    a, th, _, _, _ = _problem("quarter-tile", 3)
    m, want, _ = _model(monkeypatch, "quarter-tile", 3)
    o = _classes("p2")[0](*a, init_params=th.copy(), var_form=1)
    o.vectorized = True
    for _ in range(50):
        o.adam_step()
    m._step(50, False)
    v = m.h.kernel_variant()
    assert all(w in v for w in want), v
    print("trajectory | 50 steps | %s | parameters %.2e" % (v, rel(m.get_params(), o.get_params())))
    assert rel(m.get_params(), o.get_params()) < TRAJ_TOL


@pytest.mark.parametrize("plan", list(PLANS))
def test_reverse_dw_two_passes_are_bitwise_equal(monkeypatch, plan):
    nex, ney, _, nt, _ = PLANS[plan]
    m, want, _ = _model(monkeypatch, plan, 3)
    l3a, ga = m.loss_and_grad()
    ra = np.array(m.h.residuals(nex * ney * nt * nt))
    v = m.h.kernel_variant()
    assert all(w in v for w in want), v
    l3b, gb = m.loss_and_grad()
    rb = np.array(m.h.residuals(nex * ney * nt * nt))
    assert np.all(np.isfinite(ga)) and np.abs(ga).max() > 0.0
    assert ga.tobytes() == gb.tobytes() and np.asarray(l3a).tobytes() == np.asarray(l3b).tobytes() and ra.tobytes() == rb.tobytes(), (v, "not reproducible")
