"""Parity at GENERIC points of the input space, one case per launch structure (tests/generic_point.py says why): warped grids -- no two
elements share J, J/Jx, J/Jy --, Xavier + 0.3 N(0,1) on every weight and every bias, V = 0.6 and epsilon = 0.9 in the AdvDiff cases,
right-hand sides recomputed for the warped grid or seeded random, lossb_weight = 3, Adam constants other than the defaults.

Every case asserts: the kernel instantiation that ran is the one meant; each entry of the loss triple within 1e-9; the gradient within
1e-9 PER PARAMETER BLOCK (W_l, b_l, epsilon -- and no block is negligible: generic_point.block_errors); the residuals within 1e-9 of
their norm; the parameters after four TF1-Adam steps within 1e-8 (epsilon also on its own).  The figures are DESIGN section 2's.  Reference: the
vectorised CPU oracle below 20 000 quadrature points and on the full config-4 / tight-plan grids, `backend="generic"` on the device for
the larger grids (the generic backend is itself checked against the oracle on warped grids here).  tests/test_generic_point_host.py
pins the reference side: three CPU restatements agree block-wise to 1e-12 at such points.

The instantiations reached are printed when the file's last test has run (pytest -rA / -s) and checked against a list by that test."""
import numpy as np
import pytest

import generic_point as gp
from cases import rel

pytestmark = pytest.mark.gpu

TOL = 1e-9          # one evaluation: loss triple, gradient per block, residuals
STEP_TOL = 1e-8     # parameters after four Adam steps (and epsilon on its own)
L2, L3 = [2, 20, 20, 1], [2, 20, 20, 20, 1]
REACHED = {}        # kernel variant -> the cases that ran it


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)


# The AdvDiff cases: the variational term carries (Jx Jt)^2, so on many small elements it -- and d loss / d epsilon with it -- sinks far
# below the data term.  Their grids are small and their seeds were taken, on the CPU oracle alone, as the first of seed, seed + 1000, ..
# with |d/d epsilon| >= 4e-4 of the gradient norm (generic_point.BLOCK_FLOOR is 1e-4: every block of every case is checked against it).


# ---- builders ----------------------------------------------------------------------------------------------------------------
def _setup(c):
    """the warped setup dict and the generic initial parameters of case dict `c`"""
    from hp_vpinns_amd.drivers import advdiff, poisson1d, poisson2d
    ntx, nty = c.get("counts", (c["nt"], c["nt"]))
    if c["prob"] == "p2":
        s = poisson2d.setup(N_el_x=c["nex"], N_el_y=c["ney"], N_test_x=ntx, N_test_y=nty, N_quad=c["q"], N_bound=c.get("nb", 13), with_test_grid=False)
        s = gp.warp_poisson2d(s, c["seed"], F=c.get("F", "recomputed"))
        th = gp.generic_theta(c["L"], c["seed"])
    elif c["prob"] == "adv":
        s = advdiff.setup(N_el_x=c["nex"], N_el_t=c["ney"], N_test_x=ntx, N_test_t=nty, N_quad=c["q"], N_bound=c.get("nb", 11), with_test_grid=False)
        s = gp.warp_advdiff(s, c["seed"])
        th = gp.generic_theta(c["L"], c["seed"], extra=[0.9])
    else:
        s = gp.warp_poisson1d(poisson1d.setup(N_Element=c["nex"], N_testfcn=c["nt"], N_Quad=c["q"]), c["seed"])
        th = gp.generic_theta(c["L"], c["seed"])
    if "ndata" in c:
        kx = "XT_u_train" if c["prob"] == "adv" else "X_u_train"
        s[kx], s["u_train"] = gp.data_subset(s[kx], s["u_train"], c["ndata"], c["seed"])
    return s, th


def _classes(prob):
    from hp_vpinns_amd import vpinn
    from oracle import vpinn_oracle as O
    return {"p2": (O.OracleVPINN2D, vpinn.VPINN2D, gp.p2_tuple), "adv": (O.OracleVPINNAdvDiff, vpinn.VPINNAdvDiff, gp.p3_tuple),
            "p1": (O.OracleVPINN1D, vpinn.VPINN1D, gp.p1_tuple)}[prob]


def _kw(c):
    kw = dict(var_form=c["vf"])
    if c["prob"] == "adv":
        kw["V"] = 0.6
    if "lbw" in c:
        kw["lossb_weight"] = c["lbw"]
    return kw


class _DeviceRef:
    """`backend="generic"` on the device behind the oracle's interface (the larger grids)."""

    def __init__(self, m, n_res):
        assert m.backend() == "generic"
        self.m, self.n_res, self.last = m, n_res, {}

    def loss_and_grad(self):
        l3, g = self.m.loss_and_grad()
        assert "generic" in self.m.h.kernel_variant(), self.m.h.kernel_variant()
        self.last["R"] = self.m.h.residuals(self.n_res)
        return l3, g

    def adam_step(self):
        self.m._step(1, False)

    def get_params(self):
        return self.m.get_params()


def _pair(c, monkeypatch):
    """(reference, product, layers, number of residuals) of case `c`; the switches of c['env'] are set before the handle exists"""
    s, th = _setup(c)
    Oc, Mc, tup = _classes(c["prob"])
    a = tup(s, c["L"])
    nt2 = c["nt"] * (c["nt"] if c["prob"] != "p1" else 1)
    n_res = c["nex"] * (c["ney"] if c["prob"] != "p1" else 1) * nt2
    if c.get("ref", "oracle") == "oracle":
        o = Oc(*a, init_params=th, **_kw(c))
        o.vectorized = True
    else:
        o = _DeviceRef(Mc(*a, init_params=th, backend="generic", **_kw(c)), n_res)
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, v)
    m = Mc(*a, init_params=th, backend=c.get("backend", "auto"), **_kw(c))
    return o, m, a, th, n_res


def _worst_element(r, r_ref, n_elem):
    d = np.linalg.norm((r - r_ref).reshape(n_elem, -1), axis=1) / np.maximum(np.linalg.norm(r_ref.reshape(n_elem, -1), axis=1), 1e-300)
    return int(np.argmax(d)), float(d.max())


def _check(name, o, m, layers, n_extra, n_res, n_elem, want, structure):
    """the five assertions of every case; every message names the instantiation that ran"""
    l3o, go = o.loss_and_grad()
    l3m, gm = m.loss_and_grad()
    v, ps = m.h.kernel_variant(), m.h.pass_structure()
    REACHED.setdefault(v, []).append(name)
    for w in want:
        if w.startswith("$"):
            assert v.endswith(w[1:]), (name, v, ps)
        else:
            assert w in v, (name, "wanted", w, "ran", v, ps)
    if structure is not None:
        assert ps == structure, (name, v, ps)
    l3o, l3m = np.asarray(l3o, dtype=np.float64), np.asarray(l3m, dtype=np.float64)
    e3 = np.abs(l3m - l3o) / np.abs(l3o)
    rm, ro = m.h.residuals(n_res), np.asarray(o.last["R"], dtype=np.float64).reshape(-1)
    kb, eb = gp.worst_block(gm, go, layers, n_extra)
    we = _worst_element(rm, ro, n_elem)
    print("%s | %s | %s | loss3 err %s | worst block %s %.2e (global %.2e) | residuals %.2e (worst element %d: %.2e)"
          % (name, v, ps, e3, kb, eb, rel(gm, go), rel(rm, ro), we[0], we[1]))
    assert e3.max() < TOL, (name, v, "loss triple", l3m, l3o)
    assert eb < TOL, (name, v, "gradient block", kb, eb, gp.block_errors(gm, go, layers, n_extra))
    assert rel(rm, ro) < TOL, (name, v, "residuals", rel(rm, ro), "worst element", we)
    for _ in range(4):
        o.adam_step()
    m._step(4, False)
    pm, po = m.get_params(), o.get_params()
    ep = rel(pm, po)
    print("%s | four Adam steps: parameters %.2e%s" % (name, ep, " | epsilon %.12f %.12f" % (pm[-1], po[-1]) if n_extra else ""))
    assert ep < STEP_TOL, (name, v, "parameters after four Adam steps", ep)
    if n_extra:                                          # (epsilon is one number among 900: on its own)
        assert abs(pm[-1] - po[-1]) < STEP_TOL * abs(po[-1]), (name, v, "epsilon after four Adam steps", pm[-1], po[-1])
    return v


def _C(name, prob, vf, q, nt, nex, ney, L, want, structure, seed, **kw):
    return pytest.param(dict(name=name, prob=prob, vf=vf, q=q, nt=nt, nex=nex, ney=ney, L=L, want=want, structure=structure, seed=seed, **kw), id=name)


ONE = {"HPV_FUSE": "i"}      # one workgroup per element on a grid smaller than the chip: k_iter_fused without SPLIT against the CPU oracle
WI, WS = "whole-iteration", "whole-iteration-split"

CASES = [
    # k_iter_fused, the two one-hot terms of Poisson-2D var_form 1 on 20x20 / 10x10
    _C("onehot-L3-quarter-tiles-config4", "p2", 1, 20, 10, 16, 16, L3, ["k_iter_fused<L=3,SPLIT=false,QT=true"], WI, 501, nb=40),
    _C("onehot-L2", "p2", 1, 20, 10, 5, 3, L2, ["k_iter_fused<L=2,SPLIT=false,QT=true"], WI, 502, env=ONE),
    _C("onehot-whole-tiles", "p2", 1, 20, 10, 5, 3, L3, ["k_iter_fused<L=3,SPLIT=false,QT=false"], WI, 503, env=dict(ONE, HPV_NO_QUARTER_TILE="1")),
    # the other shapes, random F
    _C("onehot-16x16", "p2", 1, 16, 8, 5, 3, L3, ["k_iter_fused<L=3,SPLIT=false,", ",16x16/8x8>"], WI, 504, env=ONE, F="random"),
    _C("onehot-12x12", "p2", 1, 12, 6, 5, 3, L2, ["k_iter_fused<L=2,SPLIT=false,", ",12x12/6x6>"], WI, 505, env=ONE, F="random"),
    # the general forms
    _C("gen-p2vf0-16x16", "p2", 0, 16, 8, 5, 3, L3, ["k_iter_fused<L=3,SPLIT=false,", ",16x16/8x8,NT2=1,GEN>"], WI, 506, env=ONE),
    _C("gen-advf0-16x16", "adv", 0, 16, 8, 2, 2, L3, ["k_iter_fused<L=3,SPLIT=false,", ",16x16/8x8,NT2=1,GEN>"], WI, 4507, env=ONE),
    _C("gen-advf1-12x12", "adv", 1, 12, 6, 3, 2, L2, ["k_iter_fused<L=2,SPLIT=false,", ",12x12/6x6,GEN>"], WI, 3508, env=ONE),
    _C("tight-plan-p2vf0-config4", "p2", 0, 20, 10, 16, 16, L3, ["k_iter_fused<L=3,SPLIT=false,", ",20x20/10x10,NT2=1,GEN>"], WI, 509, nb=40),
    _C("tight-plan-advf0", "adv", 0, 20, 10, 2, 2, L3, ["k_iter_fused<L=3,SPLIT=false,", ",20x20/10x10,NT2=1,GEN>"], WI, 5510, env=ONE),
    # a padded rule: q = 14 on the 16x16 kernel
    _C("padded-q14-p2vf1", "p2", 1, 14, 7, 5, 3, L3, ["k_iter_fused<L=3,SPLIT=true,", ",16x16/7x7>"], WS, 511),
    _C("padded-q14-advf0", "adv", 0, 14, 7, 2, 2, L3, ["k_iter_fused<L=3,SPLIT=true,", ",16x16/7x7,NT2=1,GEN>"], WS, 512),
    # the element loop and the ragged tail (larger grids: against the generic backend)
    _C("element-loop-17x17", "p2", 1, 16, 8, 17, 17, L3, ["k_iter_fused<L=3,", ",16x16/8x8>", "$elements-per-workgroup>1"], WI, 513,
       env={"HPV_FUSE": "m"}, nb=40, ref="generic"),
    _C("ragged-tail-24x23", "p2", 1, 20, 10, 24, 23, L3, ["k_iter_fused<L=3,SPLIT=false,", "SPLIT=true split=", "$on the last 40 elements"], WS, 514,
       nb=40, ref="generic"),
    # k_iter_small
    _C("small-L2", "p2", 1, 10, 5, 8, 8, L2, ["k_iter_small<L=2>"], WI, 515, nb=20),
    _C("small-L3", "p2", 1, 10, 5, 8, 8, L3, ["k_iter_small<L=3>"], WI, 516, nb=20),
    # k_iter_tile: the other channel sets on 10x10 / 5x5
    _C("tile-advf0", "adv", 0, 10, 5, 3, 2, L3, ["k_iter_tile<D=2,"], "whole-iteration-tile", 517),
    _C("tile-advf1", "adv", 1, 10, 5, 3, 2, L3, ["k_iter_tile<D=2,"], "whole-iteration-tile", 1518),
    _C("tile-p2vf0", "p2", 0, 10, 5, 3, 2, L3, ["k_iter_tile<D=2,"], "whole-iteration-tile", 519, nb=30),
    _C("tile-p2vf2", "p2", 2, 10, 5, 3, 2, L3, ["k_iter_tile<D=2,"], "whole-iteration-tile", 520, nb=30),
    # the 1-D rule 80 / 60, sin network, every bias non-zero: k_iter_tile under var_forms 1 / 2; var_form 3 has the element-edge batch
    # (P1:88-91), which no whole-iteration kernel takes: forward, workgroup-per-element projection and reverse as separate launches
    _C("tile-1d-vf1", "p1", 1, 80, 60, 5, 1, [1, 20, 20, 20, 1], ["k_iter_tile<D=1,", "80x1/60x1"], "whole-iteration-tile", 521),
    _C("tile-1d-vf2", "p1", 2, 80, 60, 5, 1, [1, 20, 20, 20, 1], ["k_iter_tile<D=1,", "80x1/60x1"], "whole-iteration-tile", 522),
    _C("1d-vf3-edge-terms", "p1", 3, 80, 60, 5, 1, [1, 20, 20, 20, 1], ["k_fwd_mfma<D=1,NT1=0,NT2=0,sin,L=3,H=20>", "k_project_wg<80x1/60x1>", "k_bwd_mfma<D=1,NT1=0,NT2=0,sin,L=3,H=20>"], "separate", 523),
    # k_iter_tall: 8 x 1 elements of 80x80 points
    _C("tall-advf0", "adv", 0, 80, 5, 8, 1, L3, ["k_iter_tall<NT1=2,NT2=1,"], "whole-iteration-tall", 2524, ref="generic"),
    _C("tall-advf1", "adv", 1, 80, 5, 8, 1, L3, ["k_iter_tall<NT1=2,NT2=0,"], "whole-iteration-tall", 1525, ref="generic"),
    # k_iter_elem
    _C("elem-16x16-p2vf2", "p2", 2, 16, 8, 5, 3, L3, ["k_iter_elem<", "H=20,16x16/8x8,"], "whole-iteration-element", 526, env={"HPV_FUSE": "e"}),
    _C("elem-H32", "p2", 1, 16, 8, 3, 3, [2, 32, 32, 32, 1], ["k_iter_elem<", "H=32,16x16/8x8,"], "whole-iteration-element", 527, env={"HPV_FUSE": "e"}),
    # the separate launches on the config-4 shape
    _C("separate-project-wg", "p2", 1, 20, 10, 5, 3, L3, ["k_fwd_mfma<", "k_project_wg<20x20/10x10>", "k_bwd_mfma<"], "separate", 528, env={"HPV_FUSE": "n"}),
    _C("separate-project-tp", "p2", 1, 20, 10, 24, 22, L3, ["k_fwd_mfma<", "k_project_tp<20x20/10x10>", "k_bwd_mfma<"], "separate", 529,
       env={"HPV_FUSE": "n"}, nb=40, ref="generic"),
    _C("projection-in-the-reverse-kernel", "p2", 1, 20, 10, 5, 3, L3, ["k_bwd_mfma<", "proj=20x20/10x10"], "fused-reverse", 530, env={"HPV_FUSE": "b"}),
    _C("project-wg-q24", "p2", 1, 24, 12, 2, 2, L3, ["k_project_wg<24x24/12x12>"], "separate", 531),
    _C("project-wg-q32", "p2", 1, 32, 16, 2, 2, L3, ["k_project_wg<32x32/16x16>"], "separate", 532),
    # the width-generic kernels
    _C("wide-H32", "p2", 1, 10, 5, 3, 2, [2, 32, 32, 32, 1], ["k_fwd_wide<", "k_project_wg<10x10/5x5>", "k_bwd_wide<", "H=32>"], "separate", 533),
    _C("wide-H64-p2vf0", "p2", 0, 10, 5, 3, 2, [2, 64, 64, 1], ["k_fwd_wide<", "k_project_wg<10x10/5x5>", "k_bwd_wide<", "H=64>"], "separate", 534),
    _C("wide-H32-advf0", "adv", 0, 10, 5, 3, 2, [2, 32, 32, 32, 1], ["k_fwd_wide<", "k_project_wg<10x10/5x5>", "k_bwd_wide<", "H=32>"], "separate", 1535),
    # backend="generic": what the larger grids above are compared against
    _C("generic-p2vf1", "p2", 1, 12, 6, 4, 3, L3, ["k_mlp_fwd_generic", "k_mlp_bwd_generic"], "separate", 536, backend="generic"),
    _C("generic-advf0", "adv", 0, 12, 6, 4, 3, L3, ["k_mlp_fwd_generic", "k_mlp_bwd_generic"], "separate", 537, backend="generic"),
    _C("generic-advf1", "adv", 1, 20, 10, 3, 2, L3, ["k_mlp_fwd_generic", "k_mlp_bwd_generic"], "separate", 6538, backend="generic"),
    # lossb_weight = 3
    _C("lossb-weight-3-p2", "p2", 1, 20, 10, 4, 3, L3, ["k_iter_fused<L=3,SPLIT=true,"], WS, 539, lbw=3, F="random"),
    _C("lossb-weight-3-adv", "adv", 0, 16, 8, 2, 2, L3, ["k_iter_fused<L=3,SPLIT=true,", "GEN>"], WS, 540, lbw=3),
] + [
    # the data tiles' tail
    _C("data-points-%d" % n, "p2", 1, 20, 10, 4, 3, L3, ["k_iter_fused<L=3,SPLIT=true,"], WS, 541 + i, ndata=n, F="random")
    for i, n in enumerate((1, 15, 16, 17, 33))
] + [
    _C("data-points-17-tile", "adv", 0, 10, 5, 3, 2, L3, ["k_iter_tile<D=2,"], "whole-iteration-tile", 2547, ndata=17),
]


@pytest.mark.parametrize("c", CASES)
def test_launch_structure_at_a_generic_point(c, monkeypatch):
    o, m, a, th, n_res = _pair(c, monkeypatch)
    n_elem = c["nex"] * (c["ney"] if c["prob"] != "p1" else 1)
    assert c.get("ref") == "generic" or n_elem * c["q"] * (c["q"] if c["prob"] != "p1" else 1) < 20000 or "config4" in c["name"]
    _check(c["name"], o, m, c["L"], 1 if c["prob"] == "adv" else 0, n_res, n_elem, c["want"], c["structure"])


# ---- SPLIT shards taken from the MIDDLE of a warped 16 x 16 grid ------------------------------------------------------------------
@pytest.mark.parametrize("vf,q,nt,eb,ee,want", [(1, 20, 10, 96, 160, ["k_iter_fused<L=3,SPLIT=true,"]),
                                                 (1, 20, 10, 100, 115, ["k_iter_fused<L=3,SPLIT=true,"]),
                                                 (0, 16, 8, 64, 96, ["k_iter_fused<L=3,SPLIT=true,", ",16x16/8x8,NT2=1,GEN>"])],
                         ids=["64-elements", "15-elements", "general-form-32-elements"])
def test_split_shard_from_the_middle_of_a_warped_grid(vf, q, nt, eb, ee, want, monkeypatch):
    """hpv_set_elements(e_begin, e_end) on the full warped grid: an element index that misses e_begin reads another element's
    coefficient, F row or affine map.  Reference: the element loop of the oracle restricted to [e_begin, e_end) on the SAME full
    grid (loss, gradient, Adam steps) and the vectorised oracle on the grid rows that hold the shard (residuals).  Poisson-2D
    var_form 1 (one-hot) and var_form 0 (the general form): on 256 AdvDiff elements the variational term, and with it d/d epsilon,
    is 1e-7 of the gradient -- below generic_point.BLOCK_FLOOR."""
    c = dict(prob="p2", vf=vf, q=q, nt=nt, nex=16, ney=16, L=L3, seed=560 + ee, nb=13)
    s, th = _setup(c)
    Oc, Mc, tup = _classes("p2")
    a = tup(s, L3)
    o = Oc(*a, init_params=th, **_kw(c))
    o.e_range = (eb, ee)                                 # (the element loop: `vectorized` stays off)
    rb, re_ = eb // 16, (ee + 15) // 16                  # the grid rows ex that hold the shard
    ar = list(a)
    ar[7], ar[8], ar[10] = a[7][rb:re_], a[8][rb:re_ + 1], [a[10][0][rb:re_], a[10][1]]
    orow = Oc(*ar, init_params=th, **_kw(c))
    orow.loss_parts_vectorized()
    o.last = {"R": orow.last["R"].reshape((re_ - rb) * 16, -1)[eb - rb * 16:ee - rb * 16]}
    m = Mc(*a, init_params=th, **_kw(c))
    m.h.set_elements(a[8], a[9], eb, ee)
    _check("split-shard-p2-vf%d-[%d,%d)" % (vf, eb, ee), o, m, L3, 0, (ee - eb) * nt * nt, ee - eb, want, WS)


# ---- per-element test-function counts (,NACT) on a warped grid ---------------------------------------------------------------------
def test_counted_run_on_a_warped_grid(monkeypatch):
    """N_test_x / N_test_y lists of unequal counts: the oracle's element loop reads them per element; the residual blocks against the
    vectorised oracle with the largest counts everywhere (phi_k does not depend on how many follow: an element's block is a corner)."""
    nax, nay = [10, 4, 7, 9, 5], [6, 10, 8]
    c = dict(prob="p2", vf=1, q=20, nt=10, nex=5, ney=3, L=L3, seed=570, counts=(nax, nay))
    s, th = _setup(c)
    Oc, Mc, tup = _classes("p2")
    a = tup(s, L3)
    o = Oc(*a, init_params=th, var_form=1)               # (the element loop)
    dense = np.zeros((5, 3, 10, 10))
    for ex in range(5):
        for ey in range(3):
            dense[ex, ey, :nay[ey], :nax[ex]] = s["F_ext_total"][ex, ey]
    ad = list(a)
    ad[7], ad[10] = dense, [[10] * 5, [10] * 3]
    od = Oc(*ad, init_params=th, var_form=1)
    od.loss_parts_vectorized()
    R = od.last["R"].copy()
    for ex in range(5):
        for ey in range(3):
            R[ex, ey, nay[ey]:, :] = 0.0
            R[ex, ey, :, nax[ex]:] = 0.0
    o.last = {"R": R}
    m = Mc(*a, init_params=th, var_form=1)
    _check("counted-5x3", o, m, L3, 0, 15 * 100, 15, ["k_iter_fused<L=3,", ",NACT>"], WS)


# ---- device RHS assembly ----------------------------------------------------------------------------------------------------------
def test_device_rhs_assembly_on_a_warped_grid():
    """hpv_assemble_rhs reads jac[e] per element: against the numpy F (test_generic_point_host.py pins it to the driver's loop)."""
    from hp_vpinns_amd.drivers.poisson2d import f_ext
    from hp_vpinns_amd.rhs import assemble_F_ext_2d
    rng = np.random.default_rng(580)
    gx, gy = gp.warp(np.linspace(-1, 1, 8), rng), gp.warp(np.linspace(-1, 1, 6), rng)
    for q, ntx, nty in ((10, 5, 4), (20, 10, 10)):
        F = assemble_F_ext_2d(f_ext, gx, gy, ntx, nty, q)
        Fn = gp.poisson2d_F(gx, gy, ntx, nty, q)
        e, worst = _worst_element(F.reshape(-1), Fn.reshape(-1), 35)
        print("device F on a warped 7x5 grid, q = %d: rel %.2e, worst element %d %.2e" % (q, rel(F, Fn), e, worst))
        assert rel(F, Fn) < 1e-12 and worst < 1e-12, (q, rel(F, Fn), e, worst)


# ---- hpv_eval_channels and hpv_predict --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fused-dispatch-shape", "wide"])
def test_channels_and_predict_at_a_generic_point(kind, monkeypatch):
    if kind == "wide":
        c = dict(prob="adv", vf=0, q=10, nt=5, nex=3, ney=2, L=[2, 32, 32, 32, 1], seed=590)
    else:
        c = dict(prob="p2", vf=1, q=16, nt=8, nex=5, ney=3, L=L3, seed=591)
    o, m, a, th, n_res = _pair(c, monkeypatch)
    o.loss_and_grad()
    m.loss_and_grad()
    v = m.h.kernel_variant()
    assert ("k_fwd_wide" in v) if kind == "wide" else ("k_iter_fused<" in v), v
    chans = o.last["channels"]
    ch = m.h.channels(chans[0].size, len(chans))
    for k in range(len(chans)):
        print("%s channel %d: rel %.2e" % (kind, k, rel(ch[k], chans[k])))
    for k in range(len(chans)):
        assert rel(ch[k], chans[k]) < 1e-12, (v, "channel", k, rel(ch[k], chans[k]))
    rng = np.random.default_rng(592)
    lo, hi = (np.array([-1.0, 0.0]), np.array([1.0, 1.0])) if c["prob"] == "adv" else (np.array([-1.0, -1.0]), np.array([1.0, 1.0]))
    for n in (1, 15, 17, 1000):
        X = lo + (hi - lo) * rng.uniform(size=(n, 2))
        um, uo = m.predict(X), o.predict(X)
        assert um.shape == uo.shape == (n, 1)
        print("%s predict n = %d: rel %.2e" % (kind, n, rel(um, uo)))
        assert rel(um, uo) < 1e-12, (v, "predict", n, rel(um, uo))


# ---- the three implementations of the TF1-Adam update with other constants than the defaults ---------------------------------------
ADAM = dict(beta1=0.8, beta2=0.99, eps=1e-6)
ADAM_LR = 3e-3


def _with_adam_constants(m):
    """The model's problem on a handle created with ADAM through _lib's handle constructor.  The classes of vpinn.py do not pass the
    Adam constants on, so this follows vpinn._new_handle step by step and reads its private pieces (_handle_args, _populate,
    _init_params, _to_dev): if those are renamed, this helper moves with them."""
    from hp_vpinns_amd import _lib
    args, kw = m._handle_args
    m.h.close()
    m.h = _lib.Handle(*args, **dict(kw, lr=ADAM_LR), **ADAM)
    m._populate()
    m.h.set_params(m._to_dev(m._init_params))
    m.h.backend_in_use()
    return m


@pytest.mark.parametrize("how", ["fused-in-k_finalize", "k_adam", "deferred-prologue"])
def test_adam_constants_reach_every_update_implementation(how, monkeypatch):
    """beta1 = 0.8, beta2 = 0.99, eps = 1e-6, lr = 3e-3 for 20 steps from the generic point: parameters and the packed state
    [theta | m | v | beta1^t | beta2^t] against the oracle's TF1 rule with the same constants, each piece within 1e-7.

    The deferred prologue is reached as test_gpu_deferred.py reaches it: in this process, the handle's in-library exchange
    connected to a 1-rank world with rccl_connect(1, 0, id) -- not HPV_FORCE_DIST=1 in a child process, because the handle with the
    Adam constants is created here, after the class has built its own.  The library does not report whether an update rode in the
    prologue; the shard is the 8 x 4 one test_gpu_deferred.py establishes as riding (its 'shared-element' case: bit-equal to the
    per-iteration k_adam sequence there), where 19 of the 20 updates are formed in k_iter_fused's prologue and the last is k_adam."""
    from hp_vpinns_amd import _lib
    if how == "deferred-prologue" and int(_lib.load().hpv_rccl_available()) != 1:
        pytest.skip("librccl cannot be loaded: no in-library exchange, no deferred update")
    c = dict(prob="p2", vf=1, q=20, nt=10, nex=8, ney=4, L=L3, seed=600, F="random")
    o, m, a, th, n_res = _pair(c, monkeypatch)
    o.set_adam(ADAM["beta1"], ADAM["beta2"], ADAM["eps"], LR=ADAM_LR)
    m = _with_adam_constants(m)
    if how == "deferred-prologue":
        m.h.rccl_connect(1, 0, m.h.rccl_unique_id())
        assert m.h.exchange_in_use() == "rccl"
    if how == "k_adam":
        for _ in range(20):
            m.h.forward_backward()
            m.h.apply_adam()
    else:
        m.h.step(20, False)
    v = m.h.kernel_variant()
    REACHED.setdefault(v, []).append("adam-" + how)
    assert "k_iter_fused<L=3,SPLIT=true," in v and m.h.pass_structure() == WS, (how, v, m.h.pass_structure())
    assert m.h.updates_applied() == 20
    for _ in range(20):
        o.adam_step()
    st = m.h.get_state()
    P = th.size
    pieces = {"theta": (st[:P], o.get_params()), "m": (st[P:2 * P], o.m.numpy()), "v": (st[2 * P:3 * P], o.v.numpy()),
              "beta1^t": (st[3 * P], o.beta1_power), "beta2^t": (st[3 * P + 1], o.beta2_power)}
    errs = {k: rel(x, y) for k, (x, y) in pieces.items()}
    print(how, v, errs)
    assert rel(m.get_params(), o.get_params()) < 1e-7, (how, v, errs)
    for k, e in errs.items():
        assert e < 1e-7, (how, v, k, e, errs)
    # the constants are visible: the same 20 steps under the default constants end somewhere else
    assert abs(ADAM["beta1"] ** 21 - 0.9 ** 21) > 0.05 and abs(float(st[3 * P]) - 0.9 ** 21) > 0.05


# every row of DESIGN section 5's table: a substring of the variant one of the cases above must have run
FAMILIES = ["k_iter_fused<L=3,SPLIT=false,QT=true>", "k_iter_fused<L=2,SPLIT=false,", "SPLIT=false,QT=false", "SPLIT=true,", ",16x16/8x8>",
            ",12x12/6x6>", ",NT2=1,GEN>", ",12x12/6x6,GEN>", ",20x20/10x10,NT2=1,GEN>", ",NACT>", "elements-per-workgroup>1", "on the last 40 elements",
            "k_iter_small<L=2>", "k_iter_small<L=3>", "k_iter_tile<D=2,", "k_iter_tile<D=1,", "k_iter_tall<", "k_iter_elem<", "H=32,16x16/8x8",
            "k_project_wg<20x20/10x10>", "k_project_tp<20x20/10x10>", "proj=20x20/10x10", "k_project_wg<24x24/12x12>", "k_project_wg<32x32/16x16>",
            "k_project_wg<80x1/60x1>", "k_fwd_wide<", "H=64>", "k_mlp_fwd_generic", "k_project<"]


@pytest.fixture(scope="module", autouse=True)
def _report_instantiations():
    """prints, when the module's last test has run, which kernel instantiation every case ran (pytest -rA / -s)"""
    yield
    print("\ninstantiations reached on warped grids at generic points (%d):" % len(REACHED))
    for v in sorted(REACHED):
        print("  %-110s <- %s" % (v, ", ".join(REACHED[v])))


def test_zz_every_kernel_family_was_reached():
    """Runs last in the file: the cases above, together, ran every launch structure of DESIGN section 5 (on its own, e.g. under -k,
    it fails: it judges the whole file)."""
    assert REACHED, "run the whole file: this test judges what the cases above reached"
    missing = [f for f in FAMILIES if not any(f in v for v in REACHED)]
    assert not missing, (missing, sorted(REACHED))
