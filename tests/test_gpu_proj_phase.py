"""Phase P of k_iter_fused -- the element's projection as four small matrix products on the MFMA pipe (csrc/kernels_fused.hip) --
on 2 x 2 elements, the smallest grid on which an element index can go wrong: warped grids (no two elements share a coefficient),
Xavier + 0.3 N(0,1) on every weight and bias (tests/generic_point.py), through the handle of the C ABI as tests/test_gpu_elem.py
drives it.  Against oracle/vpinn_oracle.py: the loss triple, the element losses (the handle returns no loss_e array: each element's
mean square of the residuals the handle returns against the oracle's element), the full gradient, d/d epsilon on its own where the
problem has one, every residual.  Tolerances: those of test_gpu_elem.py for the same quantities (TOL of test_gpu_parity.py).

Every case asserts through hpv_pass_structure / hpv_kernel_variant that the whole-iteration kernel ran, and skips only when
hpv_build_info() reports its instantiation compiled out."""
import numpy as np
import pytest

import generic_point as gp
from cases import rel
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

L2, L3 = [2, 20, 20, 1], [2, 20, 20, 20, 1]


@pytest.fixture(autouse=True)
def _one_workgroup_per_element(monkeypatch, request):
    """HPV_FUSE=i: one workgroup per element also on this small grid (the default there is the SPLIT plan: its own test below)."""
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)
    if "split" not in request.node.name:
        monkeypatch.setenv("HPV_FUSE", "i")


def _setup(prob, q, ntx, nty, seed):
    from hp_vpinns_amd.drivers import advdiff, poisson2d
    if prob == "p2":
        s = poisson2d.setup(N_el_x=2, N_el_y=2, N_test_x=ntx, N_test_y=nty, N_quad=q, N_bound=13, with_test_grid=False)
        return gp.warp_poisson2d(s, seed, F="random")
    s = advdiff.setup(N_el_x=2, N_el_t=2, N_test_x=ntx, N_test_t=nty, N_quad=q, N_bound=11, with_test_grid=False)
    return gp.warp_advdiff(s, seed)


def _classes(prob):
    from hp_vpinns_amd import vpinn
    from oracle import vpinn_oracle as O
    return (O.OracleVPINN2D, vpinn.VPINN2D, gp.p2_tuple) if prob == "p2" else (O.OracleVPINNAdvDiff, vpinn.VPINNAdvDiff, gp.p3_tuple)


def _compiled_out(m, four, tight):
    st = m.h.build_info()
    gen = st.get("k_iter_fused_gen", "ok")
    return (st.get("k_iter_fused", "ok") == "absent" or gen == "absent" or (four and "three-channel" in gen)
            or (tight and "no-tight-plan" in gen))


def _element_losses(r, n_act):
    """mean square of every element's residuals over its active pair"""
    r = np.asarray(r, dtype=np.float64).reshape(len(n_act), -1)
    return (r * r).sum(axis=1) / np.asarray(n_act, dtype=np.float64)


def _compare(name, m, l3o, go, ro, n_act, want, structure, n_extra):
    l3m, gm = m.loss_and_grad()
    v, ps = m.h.kernel_variant(), m.h.pass_structure()
    assert ps == structure and v.startswith("k_iter_fused<"), (name, "the whole-iteration kernel did not run", v, ps)
    for w in want:
        assert w in v, (name, "wanted", w, "ran", v)
    ro = np.asarray(ro, dtype=np.float64).reshape(-1)
    rm = m.h.residuals(ro.size)
    lem, leo = _element_losses(rm, n_act), _element_losses(ro, n_act)
    print("%s | %s | loss3 %.2e | loss_e %.2e | gradient %.2e | residuals %.2e" % (name, v, rel(l3m, l3o), rel(lem, leo), rel(gm, go), rel(rm, ro)))
    assert rel(l3m, l3o) < TOL, (name, v, l3m, l3o)
    assert np.abs(lem - leo).max() <= TOL * np.abs(leo).max() and rel(lem, leo) < TOL, (name, v, lem, leo)
    assert rel(gm, go) < TOL, (name, v, rel(gm, go))
    assert rel(rm, ro) < TOL, (name, v, rel(rm, ro))
    if n_extra:
        print("%s | d/d epsilon %.15e %.15e" % (name, gm[-1], go[-1]))
        assert abs(gm[-1] - go[-1]) <= TOL * max(1.0, np.abs(go).max()), (name, v, gm[-1], go[-1])
    l3b, gb = m.loss_and_grad()
    assert np.array_equal(gb, gm) and np.array_equal(l3b, l3m), (name, v, "not reproducible")
    return l3m, gm, rm


def _run(name, prob, vf, q, ntx, nty, L, want, seed, four=False, tight=False, structure="whole-iteration"):
    s = _setup(prob, q, ntx, nty, seed)
    Oc, Mc, tup = _classes(prob)
    a = tup(s, L)
    n_extra = 1 if prob == "adv" else 0
    th = gp.generic_theta(L, seed, extra=[0.9] if n_extra else ())
    kw = dict(var_form=vf, **({"V": 0.6} if prob == "adv" else {}))
    m = Mc(*a, init_params=th, **kw)
    if _compiled_out(m, four, tight):
        pytest.skip("the build guard compiled this instantiation out: %s" % m.h.build_info())
    o = Oc(*a, init_params=th, **kw)
    o.vectorized = True
    l3o, go = o.loss_and_grad()
    return _compare(name, m, l3o, go, o.last["R"], [ntx * nty] * 4, want, structure, n_extra), (Mc, a, th, kw)


# ---- the three rule shapes at full counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,nt,L", [(20, 10, L3), (16, 8, L3), (12, 6, L3), (16, 8, L2)], ids=["20x20-L3", "16x16-L3", "12x12-L3", "16x16-L2"])
def test_projection_phase_rule_shapes_at_full_counts(q, nt, L):
    _run("shape-%d-L%d" % (q, len(L) - 2), "p2", 1, q, nt, nt, L, ["k_iter_fused<L=%d,SPLIT=false," % (len(L) - 2)] + ([",%dx%d/%dx%d>" % (q, q, nt, nt)] if q != 20 else []), 700 + q)      # (the variant names a shape other than the headline one)


# ---- run-time counts below the instantiated maximum, unequal directions ------------------------------------------------------------
@pytest.mark.parametrize("q,ntx,nty", [(20, 7, 4), (16, 5, 8)], ids=["20x20-7x4", "16x16-5x8"])
def test_projection_phase_run_time_counts(q, ntx, nty):
    _run("counts-%dx%d" % (ntx, nty), "p2", 1, q, ntx, nty, L3, ["SPLIT=false,", ",%dx%d/%dx%d>" % (q, q, ntx, nty)], 710 + q)


# ---- per-element counts: zero masking and the per-element mean ---------------------------------------------------------------------
def test_projection_phase_per_element_counts():
    """Elements e = ex * 2 + ey with the pairs (10,10), (1,1), (7,3), (3,9) -- no product of a per-column and a per-row list, so they
    reach the handle through set_active_tests_2d.  Reference: the oracle's own element loop, one element at a time with that
    element's uniform counts (e_range; the data term rides with element 0); residuals from the dense vectorised oracle, masked."""
    from oracle.vpinn_oracle import OracleVPINN2D
    from hp_vpinns_amd.vpinn import VPINN2D
    pairs = [(10, 10), (1, 1), (7, 3), (3, 9)]
    s = _setup("p2", 20, 10, 10, 720)
    a = gp.p2_tuple(s, L3)
    th = gp.generic_theta(L3, 720)
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
        oe.e_range, oe.use_data = (e, e + 1), e == 0        # (the data term rides with element 0)
        l3e, ge = oe.loss_and_grad()
        loss, lossv, g = loss + l3e[0], lossv + l3e[2], g + ge
        lossb = l3e[1] if e == 0 else lossb
    _compare("per-element-counts", m, np.array([loss, lossb, lossv]), g, R, [p[0] * p[1] for p in pairs], ["SPLIT=false,", ",NACT>"], "whole-iteration", 0)
    rm = m.h.residuals(400).reshape(4, 10, 10)
    for e, (nx, ny) in enumerate(pairs):        # beyond the pair: exact zeros
        assert not rm[e, ny:, :].any() and not rm[e, :, nx:].any(), (e, nx, ny)


# ---- a rule zero-weight padded onto an instantiated one ----------------------------------------------------------------------------
def test_projection_phase_padded_rule():
    _run("padded-18", "p2", 1, 18, 9, 9, L3, ["SPLIT=false,", ",20x20/9x9>"], 730)


# ---- the general forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,vf,q,nt,want,four,tight,seed", [
    ("adv", 1, 16, 8, ",16x16/8x8,GEN>", False, False, 1741),
    ("adv", 0, 16, 8, ",16x16/8x8,NT2=1,GEN>", True, False, 4742),
    ("p2", 0, 16, 8, ",16x16/8x8,NT2=1,GEN>", True, False, 743),
    ("p2", 0, 20, 10, ",20x20/10x10,NT2=1,GEN>", True, True, 744)],
    ids=["advdiff-vf1-two-terms", "advdiff-vf0-one-term-E", "poisson-vf0-one-term", "four-channels-20x20-tight-plan"])
def test_projection_phase_general_forms(prob, vf, q, nt, want, four, tight, seed):
    _run("gen-%s-vf%d-%d" % (prob, vf, q), prob, vf, q, nt, nt, L3, ["k_iter_fused<L=3,SPLIT=false,", want], seed, four=four, tight=tight)


# ---- several workgroups per element ------------------------------------------------------------------------------------------------
def test_projection_phase_split_partners_equal_the_unsplit_run(monkeypatch):
    """The same four elements as a shard the plan runs with several workgroups per element (the default on a grid this small): every
    partner projects the whole element.  Against the oracle, and against one workgroup per element at the tolerances the split tests
    of test_gpu_parity.py use (gradient / residuals 1e-12, loss triple 1e-13)."""
    (l3s, gs, rs), (Mc, a, th, kw) = _run("split", "p2", 1, 20, 10, 10, L3, ["k_iter_fused<L=3,SPLIT=true,"], 750, structure="whole-iteration-split")
    monkeypatch.setenv("HPV_FUSE", "i")
    w = Mc(*a, init_params=th, **kw)
    l3u, gu = w.loss_and_grad()
    assert "SPLIT=false" in w.h.kernel_variant() and w.h.pass_structure() == "whole-iteration", w.h.kernel_variant()
    ru = w.h.residuals(400)
    print("split against unsplit: gradient %.2e loss %.2e residuals %.2e" % (rel(gs, gu), rel(l3s, l3u), rel(rs, ru)))
    assert rel(gs, gu) < 1e-12 and rel(l3s, l3u) < 1e-13 and rel(rs, ru) < 1e-12
