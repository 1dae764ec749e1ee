"""Phase F of k_iter_fused without tangent channels (csrc/kernels_fused.hip, fwd_trip without a second tangent): the forward phase
carries the value channel alone through the hidden layers and forms u_x, u_y of a point by ONE adjoint sweep over it -- abar_L =
s'(z_L) w_o, abar_{i-1} = s'(z_{i-1}) (W_i abar_i), u_x = W1[0,:] . abar_1, u_y = W1[1,:] . abar_1 -- instead of two forward tangents.

As tests/test_gpu_reverse_direction.py: 2 x 2 elements on warped grids (a warped grid separates x from y), Xavier + 0.3 N(0,1) on every
weight and bias (tests/generic_point.py), through the handle of the C ABI, against oracle/vpinn_oracle.py (vectorised): the loss
triple, the element losses, the full gradient, d/d epsilon on its own where the problem has one and EVERY residual -- the residuals
are the direct observable of u_x, u_y -- at TOL of test_gpu_parity.py; two calls of loss_and_grad() bit-equal.  Every case asserts
through hpv_pass_structure / hpv_kernel_variant that k_iter_fused ran in the wanted plan, and skips only when hpv_build_info()
reports the instantiation compiled out.  One oracle evaluation per problem, shared by the cases that run on it.

What the cases are for:
  shapes        zero (L = 2: the head alone), one and two adjoint products past the head; 9 / 16 / 25 tiles per element
  whole tiles   HPV_NO_QUARTER_TILE with N_bound = 13: a boundary / data tile passes through fwd_trip beside element tiles -- its
                u_x, u_y must reach nothing, the data loss and the head-bias gradient (which only the data term feeds) must be right;
                and the default plan on 16 x 16, where the packed quarter tile keeps its three slots beside the new whole tiles
  GEN           AdvDiff var_form 1: both integrated arrays are combinations of u_x, u_y; V = 0.6, epsilon = 0.9
  SPLIT / MULTI several workgroups per element (the default plan on 2 x 2 elements) / several elements per workgroup (17 x 17 elements
                of 12 x 12 points: the smallest shape on the smallest grid of the MULTI test of tests/test_gpu_elem.py)
  counts        per-element test-function counts (10,10), (1,1), (10,10), (10,10): the residuals of the active pairs only
  trajectory    50 TF1-Adam steps against the oracle's adam_step, final parameters to TRAJ_TOL"""
import functools

import numpy as np
import pytest

import generic_point as gp
from cases import rel, theta0
from test_gpu_parity import TOL, TRAJ_TOL
from test_gpu_proj_phase import _classes, _compare, _compiled_out, _setup

pytestmark = pytest.mark.gpu

L2, L3 = [2, 20, 20, 1], [2, 20, 20, 20, 1]
SEED = {12: 912, 16: 916, 20: 920}


@pytest.fixture(autouse=True)
def _one_workgroup_per_element(monkeypatch, request):
    """HPV_FUSE=i: one workgroup per element also on the 2 x 2 grid (the SPLIT and MULTI cases choose their own plan)."""
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)
    if "split" not in request.node.name and "several_elements" not in request.node.name:
        monkeypatch.setenv("HPV_FUSE", "i")


@functools.lru_cache(maxsize=None)
def _problem(prob, q, nt, nl):
    """(constructor arguments, parameters, keywords, the oracle's loss triple, gradient and residuals) of one problem; read-only"""
    L = L3 if nl == 3 else L2
    s = _setup(prob, q, nt, nt, SEED[q] + (1000 if prob == "adv" else 0))
    Oc, _, tup = _classes(prob)
    a = tup(s, L)
    th = gp.generic_theta(L, SEED[q], extra=[0.9] if prob == "adv" else ())
    kw = dict(var_form=1, **({"V": 0.6} if prob == "adv" else {}))
    o = Oc(*a, init_params=th, **kw)
    o.vectorized = True
    l3o, go = o.loss_and_grad()
    l3o = np.asarray(l3o, dtype=np.float64)
    for x in (th, l3o, go):
        x.setflags(write=False)
    R = np.array(o.last["R"], dtype=np.float64)
    R.setflags(write=False)
    return a, th, kw, l3o, go, R


def _case(name, prob, q, nt, nl, want, structure="whole-iteration"):
    a, th, kw, l3o, go, R = _problem(prob, q, nt, nl)
    m = _classes(prob)[1](*a, init_params=th.copy(), **kw)
    if _compiled_out(m, False, False):
        pytest.skip("the build guard compiled this instantiation out: %s" % m.h.build_info())
    l3m, gm, _ = _compare(name, m, l3o, go, R, [nt * nt] * 4, want, structure, 1 if prob == "adv" else 0)
    return m, l3m, gm, l3o, go


# ---- the three rule shapes, two and three hidden layers ----------------------------------------------------------------------------
@pytest.mark.parametrize("q,nt,nl", [(12, 6, 3), (20, 10, 3), (16, 8, 2)], ids=["12x12-L3", "20x20-L3", "16x16-L2"])
def test_forward_adjoint_rule_shapes(q, nt, nl):
    want = ["k_iter_fused<L=%d,SPLIT=false," % nl] + ([",%dx%d/%dx%d>" % (q, q, nt, nt)] if q != 20 else [])
    _case("shape-%d-L%d" % (q, nl), "p2", q, nt, nl, want)


# ---- a boundary / data tile beside element tiles in one forward trip; the quarter tile beside new whole tiles ---------------------
@pytest.mark.parametrize("q,nt,whole", [(20, 10, True), (16, 8, True), (16, 8, False)], ids=["20x20-whole-tiles", "16x16-whole-tiles", "16x16-default"])
def test_forward_adjoint_data_tile(monkeypatch, q, nt, whole):
    if whole:
        monkeypatch.setenv("HPV_NO_QUARTER_TILE", "1")
    want = ["k_iter_fused<L=3,SPLIT=false,"] + (["QT=false"] if whole else []) + ([",%dx%d/%dx%d>" % (q, q, nt, nt)] if q != 20 else [])
    name = "data-tile-%d-%s" % (q, "whole" if whole else "default")
    _, l3m, gm, l3o, go = _case(name, "p2", q, nt, 3, want)
    # the data loss on its own, and the head's bias: element tiles carry no adjoint on the value channel, so only the data term feeds it
    _, b0, b1 = gp.blocks(L3)[-1]
    print("%s | data loss %.15e %.15e | head bias %s %s" % (name, l3m[1], l3o[1], gm[b0:b1], go[b0:b1]))
    assert l3o[1] > 0.0 and abs(l3m[1] - l3o[1]) < TOL * l3o[1], (name, l3m, l3o)
    assert np.abs(go[b0:b1]).max() > 0.0 and rel(gm[b0:b1], go[b0:b1]) < TOL, (name, gm[b0:b1], go[b0:b1])


# ---- both integrated arrays are combinations of u_x, u_y ---------------------------------------------------------------------------
def test_forward_adjoint_general_form_advdiff():
    _case("gen-adv-vf1-16", "adv", 16, 8, 3, ["k_iter_fused<L=3,SPLIT=false,", ",16x16/8x8,GEN>"])


# ---- several workgroups per element ------------------------------------------------------------------------------------------------
def test_forward_adjoint_split():
    _case("split", "p2", 20, 10, 3, ["k_iter_fused<L=3,SPLIT=true,"], structure="whole-iteration-split")


# ---- several elements per workgroup ------------------------------------------------------------------------------------------------
def test_forward_adjoint_several_elements_per_workgroup(monkeypatch):
    """k_iter_fused<.., MULTI>: 17 x 17 elements (289 = 256 + 33: most workgroups own one element, 33 own two) of 12 x 12 points."""
    from hp_vpinns_amd.vpinn import VPINN2D
    from oracle.vpinn_oracle import OracleVPINN2D
    from test_gpu_elem import _p2
    a = _p2(12, 6, 17, 17, nb=40) + (L3,)
    th = theta0(L3, 973)
    monkeypatch.setenv("HPV_FUSE", "m")            # (read when the device batch is assembled)
    m = VPINN2D(*a, init_params=th)
    monkeypatch.delenv("HPV_FUSE")
    if m.h.build_info().get("k_iter_fused", "ok") != "ok":
        pytest.skip("the build guard compiled this instantiation out: %s" % m.h.build_info())
    o = OracleVPINN2D(*a, init_params=th)
    o.vectorized = True
    l3o, go = o.loss_and_grad()
    l3m, gm = m.loss_and_grad()
    v = m.h.kernel_variant()
    assert m.h.pass_structure() == "whole-iteration" and v.startswith("k_iter_fused<L=3,") and v.endswith("elements-per-workgroup>1"), v
    rm, ro = m.h.residuals(17 * 17 * 36), o.last["R"].reshape(-1)
    print("multi | %s | loss3 %.2e | gradient %.2e | residuals %.2e" % (v, rel(l3m, l3o), rel(gm, go), rel(rm, ro)))
    assert rel(l3m, l3o) < TOL and rel(gm, go) < TOL and rel(rm, ro) < TOL, (v, l3m, l3o, rel(gm, go), rel(rm, ro))
    l3b, gb = m.loss_and_grad()
    assert np.array_equal(gb, gm) and np.array_equal(l3b, l3m), (v, "not reproducible")


# ---- per-element test-function counts ----------------------------------------------------------------------------------------------
def test_forward_adjoint_per_element_counts():
    """(10,10), (1,1), (10,10), (10,10) on 20 x 20 points.  Reference: the oracle's own element loop, one element at a time with that
    element's counts (the data term rides with element 0), as test_reverse_direction_zero_adjoints; residuals from the dense
    vectorised oracle, masked."""
    from oracle.vpinn_oracle import OracleVPINN2D
    from hp_vpinns_amd.vpinn import VPINN2D
    pairs = [(10, 10), (1, 1), (10, 10), (10, 10)]
    s = _setup("p2", 20, 10, 10, 921)
    a = gp.p2_tuple(s, L3)
    th = gp.generic_theta(L3, 921)
    m = VPINN2D(*a, var_form=1, init_params=th)
    if _compiled_out(m, False, False):
        pytest.skip("the build guard compiled this instantiation out: %s" % m.h.build_info())
    m.h.set_active_tests_2d([p[0] for p in pairs], [p[1] for p in pairs])
    dense = np.asarray(s["F_ext_total"], dtype=np.float64)
    od = OracleVPINN2D(*a, var_form=1, init_params=th)
    od.loss_parts_vectorized()
    R = od.last["R"].copy().reshape(4, 10, 10)
    loss, lossb, lossv, g = 0.0, 0.0, 0.0, 0.0
    for e, (nx, ny) in enumerate(pairs):
        R[e, ny:, :] = 0.0
        R[e, :, nx:] = 0.0
        ae = list(a)
        ae[7], ae[10] = np.ascontiguousarray(dense[:, :, :ny, :nx]), [[nx, nx], [ny, ny]]
        oe = OracleVPINN2D(*ae, var_form=1, init_params=th)
        oe.e_range, oe.use_data = (e, e + 1), e == 0
        l3e, ge = oe.loss_and_grad()
        loss, lossv, g = loss + l3e[0], lossv + l3e[2], g + ge
        lossb = l3e[1] if e == 0 else lossb
    _compare("per-element-counts", m, np.array([loss, lossb, lossv]), g, R, [p[0] * p[1] for p in pairs], ["SPLIT=false,", ",NACT>"],
             "whole-iteration", 0)


# ---- 50 optimiser steps ------------------------------------------------------------------------------------------------------------
def test_forward_adjoint_trajectory():
    a, th, kw, _, _, _ = _problem("p2", 20, 10, 3)
    m, _, _, _, _ = _case("trajectory", "p2", 20, 10, 3, ["k_iter_fused<L=3,SPLIT=false,"])
    o = _classes("p2")[0](*a, init_params=th.copy(), **kw)
    o.vectorized = True
    for _ in range(50):
        o.adam_step()
    m._step(50, False)
    assert m.h.kernel_variant().startswith("k_iter_fused<L=3,SPLIT=false,"), m.h.kernel_variant()
    print("trajectory | 50 steps | parameters %.2e" % rel(m.get_params(), o.get_params()))
    assert rel(m.get_params(), o.get_params()) < TRAJ_TOL
