"""Phase R of k_iter_fused along ONE directional tangent per point (csrc/kernels_fused.hip, rev_tile without a second tangent): the
adjoints gx, gy of u_x, u_y at a point are plain numbers after the projection phase, so the reverse pass carries the value channel and
the tangent along d = (gx, gy) instead of the three channels (value, d/dx, d/dy).  The direction enters twice -- the first layer's
tangent pre-activation gx W1[0,:] + gy W1[1,:] and the first layer's weight gradient -- and every plan that shares rev_tile takes it.

As tests/test_gpu_proj_phase.py: 2 x 2 elements on warped grids, Xavier + 0.3 N(0,1) on every weight and bias (tests/generic_point.py),
through the handle of the C ABI, against oracle/vpinn_oracle.py (vectorised): the loss triple, the element losses, the full gradient,
d/d epsilon on its own where the problem has one, every residual, at TOL of test_gpu_parity.py; two calls of loss_and_grad() bit-equal.
Every case asserts through hpv_pass_structure / hpv_kernel_variant that k_iter_fused ran in the wanted plan, and skips only when
hpv_build_info() reports the instantiation compiled out.

What the cases are for:
  shapes        the layer loop at L - 1 = 1 and 2 recompute products, 9 / 16 / 25 tiles per element
  zero adjoints an element with the single active pair (1, 1): d tiny or zero at its points
  first layer   N_bound = 13 boundary points (weight 10): value-only tiles (d = 0) and directional tiles add into the same dW1, db and
                dW_o -- on whole tiles (HPV_NO_QUARTER_TILE: the boundary points are a tile of rev_tile) and on the default plan; the
                first-layer and head blocks of the gradient each on their own, where a wrong gx zbar_d term cannot hide behind the
                hidden-layer blocks.  The per-block bound is TOL as well: fp64 sums of at most 1 613 terms per entry, and no block below
                generic_point.BLOCK_FLOOR of the gradient norm (asserted), leave round-off four orders below it.
  GEN           AdvDiff var_form 1 (the direction formed from both integrated arrays' adjoints), V = 0.6, epsilon = 0.9
  SPLIT / MULTI several workgroups per element (the default plan on 2 x 2 elements) / several elements per workgroup (17 x 17 elements
                of 12 x 12 points: the smallest shape on the smallest grid of the MULTI test of tests/test_gpu_elem.py)
  trajectory    50 TF1-Adam steps against the oracle's adam_step, final parameters to TRAJ_TOL"""
import numpy as np
import pytest

import generic_point as gp
from cases import rel, theta0
from test_gpu_parity import TOL, TRAJ_TOL
from test_gpu_proj_phase import _classes, _compare, _compiled_out, _setup

pytestmark = pytest.mark.gpu

L2, L3 = [2, 20, 20, 1], [2, 20, 20, 20, 1]


@pytest.fixture(autouse=True)
def _one_workgroup_per_element(monkeypatch, request):
    """HPV_FUSE=i: one workgroup per element also on the 2 x 2 grid (the SPLIT and MULTI cases choose their own plan)."""
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)
    if "split" not in request.node.name and "several_elements" not in request.node.name:
        monkeypatch.setenv("HPV_FUSE", "i")


def _case(name, prob, q, nt, L, want, seed, structure="whole-iteration"):
    """One evaluation against the oracle (everything _compare of test_gpu_proj_phase.py asserts); returns what the case-specific checks need."""
    s = _setup(prob, q, nt, nt, seed)
    Oc, Mc, tup = _classes(prob)
    a = tup(s, L)
    n_extra = 1 if prob == "adv" else 0
    th = gp.generic_theta(L, seed, extra=[0.9] if n_extra else ())
    kw = dict(var_form=1, **({"V": 0.6} if prob == "adv" else {}))
    m = Mc(*a, init_params=th, **kw)
    if _compiled_out(m, False, False):
        pytest.skip("the build guard compiled this instantiation out: %s" % m.h.build_info())
    o = Oc(*a, init_params=th, **kw)
    o.vectorized = True
    l3o, go = o.loss_and_grad()
    _, gm, _ = _compare(name, m, l3o, go, o.last["R"], [nt * nt] * 4, want, structure, n_extra)
    return m, o, gm, go


def _first_layer_and_head(name, gm, go, L):
    """the blocks the direction enters (W0) or leaves through (the head), and the biases beside them, each against its own norm"""
    e = gp.block_errors(gm, go, L)
    last = len(L) - 2
    print("%s | blocks %s" % (name, {k: "%.2e" % v for k, v in e.items()}))
    for k in ("W0", "b0", "W%d" % last, "b%d" % last):
        assert e[k] < TOL, (name, k, e)


# ---- the three rule shapes, two and three hidden layers ----------------------------------------------------------------------------
@pytest.mark.parametrize("q,nt,L", [(12, 6, L3), (20, 10, L3), (16, 8, L2)], ids=["12x12-L3", "20x20-L3", "16x16-L2"])
def test_reverse_direction_rule_shapes(q, nt, L):
    want = ["k_iter_fused<L=%d,SPLIT=false," % (len(L) - 2)] + ([",%dx%d/%dx%d>" % (q, q, nt, nt)] if q != 20 else [])
    _, _, gm, go = _case("shape-%d-L%d" % (q, len(L) - 2), "p2", q, nt, L, want, 800 + q)
    _first_layer_and_head("shape-%d" % q, gm, go, L)


# ---- an element whose adjoints all but vanish ----------------------------------------------------------------------------------------
def test_reverse_direction_zero_adjoints():
    """Element 1 of (10,10), (1,1), (10,10), (10,10) keeps the single pair (1, 1): its points' gx, gy are the back-projection of ONE
    residual (tiny or zero).  Reference: the oracle's own element loop, one element at a time with that element's counts (the data term
    rides with element 0), as test_projection_phase_per_element_counts; residuals from the dense vectorised oracle, masked."""
    from oracle.vpinn_oracle import OracleVPINN2D
    from hp_vpinns_amd.vpinn import VPINN2D
    pairs = [(10, 10), (1, 1), (10, 10), (10, 10)]
    s = _setup("p2", 20, 10, 10, 820)
    a = gp.p2_tuple(s, L3)
    th = gp.generic_theta(L3, 820)
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
    _, gm, _ = _compare("zero-adjoints", m, np.array([loss, lossb, lossv]), g, R, [p[0] * p[1] for p in pairs], ["SPLIT=false,", ",NACT>"],
                        "whole-iteration", 0)
    _first_layer_and_head("zero-adjoints", gm, g, L3)


# ---- value-only tiles and directional tiles into the same first-layer and head gradient --------------------------------------------
@pytest.mark.parametrize("q,nt,whole", [(20, 10, True), (16, 8, True), (16, 8, False)], ids=["20x20-whole-tiles", "16x16-whole-tiles", "16x16-default"])
def test_reverse_direction_first_layer_gradient(monkeypatch, q, nt, whole):
    if whole:
        monkeypatch.setenv("HPV_NO_QUARTER_TILE", "1")
    want = ["k_iter_fused<L=3,SPLIT=false,"] + (["QT=false"] if whole else []) + ([",%dx%d/%dx%d>" % (q, q, nt, nt)] if q != 20 else [])
    m, o, gm, go = _case("first-layer-%d-%s" % (q, "whole" if whole else "default"), "p2", q, nt, L3, want, 830 + q)
    _first_layer_and_head("first-layer-%d" % q, gm, go, L3)
    # the boundary term is in this gradient: without it the head's bias has no adjoint at all (element tiles carry none on the value channel)
    b_head = gp.blocks(L3)[-1]
    assert np.abs(go[b_head[1]:b_head[2]]).max() > 0.0


# ---- the direction from both integrated arrays' adjoints ---------------------------------------------------------------------------
def test_reverse_direction_general_form_advdiff():
    _case("gen-adv-vf1-16", "adv", 16, 8, L3, ["k_iter_fused<L=3,SPLIT=false,", ",16x16/8x8,GEN>"], 1841)


# ---- several workgroups per element ------------------------------------------------------------------------------------------------
def test_reverse_direction_split():
    _, _, gm, go = _case("split", "p2", 20, 10, L3, ["k_iter_fused<L=3,SPLIT=true,"], 850, structure="whole-iteration-split")
    _first_layer_and_head("split", gm, go, L3)


# ---- several elements per workgroup ------------------------------------------------------------------------------------------------
def test_reverse_direction_several_elements_per_workgroup(monkeypatch):
    """k_iter_fused<.., MULTI>: 17 x 17 elements (289 = 256 + 33: most workgroups own one element, 33 own two) of 12 x 12 points."""
    from hp_vpinns_amd.vpinn import VPINN2D
    from oracle.vpinn_oracle import OracleVPINN2D
    from test_gpu_elem import _p2
    a = _p2(12, 6, 17, 17, nb=40) + (L3,)
    th = theta0(L3, 873)
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


# ---- 50 optimiser steps ------------------------------------------------------------------------------------------------------------
def test_reverse_direction_trajectory():
    m, o, _, _ = _case("trajectory", "p2", 20, 10, L3, ["k_iter_fused<L=3,SPLIT=false,"], 860)
    for _ in range(50):
        o.adam_step()
    m._step(50, False)
    assert m.h.kernel_variant().startswith("k_iter_fused<L=3,SPLIT=false,"), m.h.kernel_variant()
    print("trajectory | 50 steps | parameters %.2e" % rel(m.get_params(), o.get_params()))
    assert rel(m.get_params(), o.get_params()) < TRAJ_TOL
