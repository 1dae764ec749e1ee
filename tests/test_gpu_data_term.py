"""The boundary / data term at its point-count edges on EVERY launch structure (profiles/data_term_edges.md has the measured errors).

One handle per structure -- the smallest grid of its family in CASES of tests/test_gpu_generic_point.py, at a generic point, on warped
grids, lossb_weight != 1 -- and the data set swept on that LIVE handle with hpv_set_data: 1, 15, 16, 17, 31, 33 points, the structure's
own edge (data tiles against workgroups / free slots / extra workgroups / partial sums: data_term_reference.STRUCTURES), then DOWN to 7
and 16 (stale adjoints behind the new end, stale partials, gradient rows of the larger batch), no data at all (lossb exactly 0, the
gradient the variational one), and 17 again.  After every call: loss_and_grad() -- loss triple and gradient per block -- and the
forward-only loss() against  var_part + data_part  of tests/data_term_reference.py (CPU, fp64; tests/test_data_term_host.py proves it);
the kernel instantiation and the pass structure where the structure must stay.  One workgroup count past a whole-iteration
kernel's limit the plan declines the pass: the result must be right on whatever takes it, and the structure that did is printed.

Bounds: TOL and STEP_TOL of tests/test_gpu_generic_point.py (imported), nothing new; the lossb slot against numpy within
data_term_reference.LOSSB_TOL (1e-12).  Conditions (a) - (c) of the reference module are asserted on the reference alone before the device's
numbers are looked at.  For n > 321 condition (c) is the loss's: every term >= 0.25 against a sum <= 2.25 n, a dropped point moves
msq by at least 1/(9 n) ~ 7e-6 at 16 385 points.

No Adam step runs on a generic-backend or PINN-scheme handle here (loss_and_grad() / loss() only: eager launches)."""
import re
import time

import numpy as np
import pytest

import data_term_reference as dr
import generic_point as gp
from cases import rel
from test_gpu_generic_point import STEP_TOL, TOL, _DeviceRef, _classes, _kw, _pair

pytestmark = pytest.mark.gpu

REACHED = {}        # structure -> {kernel variant: [point counts]}
OVER = {}           # structure -> [(n, variant, pass structure)] of the passes the whole-iteration plan declined
WORST = {}          # (structure, n) -> (loss triple, gradient block, lossb slot, forward-only triple)


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)


def _rel3(l3m, l3o):
    """entry-wise relative error of a loss triple; an entry the reference has as 0 must BE 0"""
    l3m, l3o = np.asarray(l3m, dtype=np.float64), np.asarray(l3o, dtype=np.float64)
    out = np.zeros(3)
    for k in range(3):
        if l3o[k] == 0.0:
            assert l3m[k] == 0.0, ("an exact zero of the reference", k, l3m, l3o)
        else:
            out[k] = abs(l3m[k] - l3o[k]) / abs(l3o[k])
    return out


def _compare(tag, n, m, prob, L, th, w, var, X, u, want=None, structure=None, record=None):
    """set_data(X[:n], u[:n]) on the live handle, then both passes against the reference; returns (variant, pass structure)"""
    ne = dr.n_extra(prob)
    if n > 0:
        fig = dr.conditions(prob, L, th, X[:n], u[:n], w, var["grad"], TOL)        # the reference alone, first
    d = dr.data_part(prob, L, th, X[:n], u[:n], w)
    l3o, go = dr.reference(prob, var, d)
    if n > 0:
        m.h.set_data(X[:n], u[:n].reshape(-1))
    else:
        m.h.set_data(None, None)
    l3m, gm = m.loss_and_grad()
    v, ps = m.h.kernel_variant(), m.h.pass_structure()
    lf = m.loss()
    e3, ef = _rel3(l3m, l3o), _rel3(lf, l3o)
    if n > 0:
        kb, eb = gp.worst_block(gm, go, L, ne)
    else:
        eb_all = dr.without_data_errors(gm, go, L, ne)
        kb = max(eb_all, key=eb_all.get)
        eb = eb_all[kb]
    print("%s n = %d | %s | %s | loss3 %s | worst block %s %.2e (global %.2e) | forward-only %s%s"
          % (tag, n, v, ps, e3, kb, eb, rel(gm, go), ef,
             " | data share %.1e, leave-one-out %s" % (fig["share"], "%.1e" % fig["loo"] if fig["loo"] is not None else "loss") if n > 0 else ""))
    if record is not None:
        now = (float(e3.max()), float(eb), float(e3[1]), float(ef.max()))      # 16 and 17 points are visited twice: the larger figure
        record[(tag, n)] = tuple(max(x, y) for x, y in zip(now, record.get((tag, n), now)))
    for s in (want or []):
        assert s in v, (tag, n, "wanted", s, "ran", v, ps)
    if structure is not None:
        assert ps == structure, (tag, n, v, ps)
    assert e3.max() < TOL, (tag, n, v, "loss triple", l3m, l3o)
    assert e3[1] < dr.LOSSB_TOL, (tag, n, v, "lossb slot", l3m[1], l3o[1], e3[1], dr.LOSSB_TOL)
    assert eb < TOL, (tag, n, v, "gradient block", kb, eb)
    assert ef.max() < TOL and ef[1] < dr.LOSSB_TOL, (tag, n, v, "forward-only pass", lf, l3o)
    return v, ps


def _workgroups(c, v):
    """elements x split of the whole-iteration launch that ran (hpv_kernel_variant names the split)"""
    n_elem = c["nex"] * (c["ney"] if c["prob"] != "p1" else 1)
    s = re.search(r"split=(\d+)", v)
    return n_elem * (int(s.group(1)) if s else 1)


@pytest.mark.parametrize("name", list(dr.STRUCTURES))
def test_data_point_sweep_on_a_live_handle(name, monkeypatch):
    spec, c = dr.STRUCTURES[name], dr.case_of(name)
    prob, L, w = c["prob"], c["L"], float(c["lbw"])
    t0 = time.time()
    o, m, a, th, n_res = _pair(c, monkeypatch)
    if isinstance(o, _DeviceRef):            # the 80x80-point elements: the generic backend with the data taken away
        o.m.h.set_data(None, None)
        l3, g = o.m.loss_and_grad()
        assert l3[1] == 0.0 and l3[0] == l3[2] and "generic" in o.m.h.kernel_variant()
        var = dict(lossv=float(l3[2]), grad=np.asarray(g, dtype=np.float64))
    else:
        var = dr.var_part(o, prob, L, th, a[0], a[1], w)
    # the handle as the class built it: the structure, and with it the workgroup count W the point counts are taken from
    m.loss_and_grad()
    v0 = m.h.kernel_variant()
    traj = m.backend() == "mfma" and not isinstance(o, _DeviceRef)
    if traj:
        # capture, on the STARTING data, the very graph the three steps at the end replay (hpv_step serves n < 8 iterations from one
        # n-iteration graph); then the initial parameters and a fresh optimizer again -- hpv_set_params keeps the graphs
        m._step(3, False)
        assert m.h.graphs_in_use(), (name, "hpv_step fell back to eager launches: nothing was captured")
        m.set_params(th)
    W = _workgroups(c, v0) if spec["edge"] == "wg" else None
    if W is not None:
        # (k_iter_fused / k_iter_small: hpv_fused_plan declines `rest > workgroups`, rest = batch tiles - n_elem * tiles-per-element
        #  INCLUDING the pad tile where n_elem * Nq is no multiple of 16; every grid here has n_elem * Nq % 16 == 0 -- asserted --
        #  so rest is the number of data tiles.  k_iter_tall: the same count at `rest > blocks`.)
        nq = c["q"] if name != "fused-split-q14" else 16
        assert (c["nex"] * c["ney"] * nq * nq) % 16 == 0
        assert W == spec["w_static"], ("the host test checked the conditions for another workgroup count", W, spec["w_static"], v0)
    counts = dr.sweep_counts(spec, W)
    nmax = max(n for n, _ in counts)
    X = dr.points(prob, nmax, spec["seed"])
    u = dr.targets(prob, L, th, X, spec["seed"])
    print("%s: %s | W = %s | counts %s" % (name, v0, W, [n for n, _ in counts]))
    for n, kind in counts:
        stay = kind == "in"
        v, ps = _compare(name, n, m, prob, L, th, w, var, X, u, c["want"] if stay else None, c["structure"] if stay else None, WORST)
        REACHED.setdefault(name, {}).setdefault(v, []).append(n)
        if kind == "over":
            OVER.setdefault(name, []).append((n, v, ps))
            print("%s: %d points = %d data tiles, one workgroup count past the limit -> %s (%s)" % (name, n, (n + 15) // 16, v, ps))
    # one short trajectory on the merged MFMA handles (CPU oracle): the 3-iteration graph captured on the starting data above must not
    # be what runs now -- hpv_set_data drops it, the re-captured one sees the batch of 17 points the sweep ended on
    if traj:
        Oc = _classes(prob)[0]
        o2 = Oc(*dr.with_data(c, a, X[:17], u[:17]), init_params=th, **_kw(c))
        o2.vectorized = True
        for _ in range(3):
            o2.adam_step()
        m._step(3, False)
        assert m.h.graphs_in_use(), (name, "eager launches")
        pm, po = m.get_params(), o2.get_params()
        print("%s | three Adam steps on the 17 points: parameters %.2e | %s" % (name, rel(pm, po), m.h.kernel_variant()))
        assert rel(pm, po) < STEP_TOL, (name, "parameters after three Adam steps", rel(pm, po))
        if dr.n_extra(prob):
            assert abs(pm[-1] - po[-1]) < STEP_TOL * abs(po[-1]), (name, "epsilon after three Adam steps", pm[-1], po[-1])
    print("%s: %.1f s" % (name, time.time() - t0))


# ---- k_data_loss: one block, two, three, and the grid-stride loop behind the 64-block cap ---------------------------------------------
def test_k_data_loss_on_the_generic_backend(monkeypatch):
    c = dr.small_generic_case()
    o, m, a, th, n_res = _pair(c, monkeypatch)
    var = dr.var_part(o, "p2", c["L"], th, a[0], a[1], 3.0)
    X = dr.points("p2", max(dr.DATA_LOSS_COUNTS), c["seed"])
    u = dr.targets("p2", c["L"], th, X, c["seed"])
    for n in dr.DATA_LOSS_COUNTS:
        v, ps = _compare("generic-small", n, m, "p2", c["L"], th, 3.0, var, X, u, c["want"], c["structure"], WORST)
        REACHED.setdefault("generic-small", {}).setdefault(v, []).append(n)
    assert m.backend() == "generic"


def _pinn_model(prob, a, th, backend):
    from hp_vpinns_amd.vpinn import VPINN1D, VPINN2D, VPINNAdvDiff
    kw = dict(scheme="PINNs", lossb_weight=dr.PINN_W[prob], LR=0.001, init_params=th, backend=backend)
    if prob == "p1":
        return VPINN1D(*a, **kw)
    if prob == "p2":
        return VPINN2D(*a, **kw)
    return VPINNAdvDiff(*a, V=dr.PINN_V, **kw)


@pytest.mark.parametrize("backend", ["generic", "mfma"])
@pytest.mark.parametrize("prob", ["p1", "p2", "adv"])
def test_data_batch_of_the_pinn_scheme(prob, backend):
    """scheme='PINNs': the data points are a batch of their own.  backend='generic': k_data_loss at 1 .. 16 641 points; 'mfma': the small
    MFMA batch of exactly n points (ensure_small_mfma), whose last tile carries the tail, up and then down to 3 points."""
    o, a, L, th = dr.pinn_case(prob, backend)
    w = dr.PINN_W[prob]
    var = dr.var_part(o, prob, L, th, a[0], a[1], w)
    m = _pinn_model(prob, a, th, backend)
    counts = dr.DATA_LOSS_COUNTS if backend == "generic" else dr.PINN_MFMA_COUNTS
    X = dr.points(prob, max(counts), 9400)
    u = dr.targets(prob, L, th, X, 9400)
    tag = "pinn-%s-%s" % (prob, backend)
    for n in counts:
        v, ps = _compare(tag, n, m, prob, L, th, w, var, X, u, ["k_pinn_residual"], None, WORST)
        REACHED.setdefault(tag, {}).setdefault(v, []).append(n)
    assert m.backend() == backend


# ---- what ran ------------------------------------------------------------------------------------------------------------------------
FAMILIES = {"fused-unsplit": "k_iter_fused<L=2,SPLIT=false,", "fused-gen": ",16x16/8x8,NT2=1,GEN>", "fused-split-q14": "SPLIT=true,QT=false,16x16/7x7>",
            "small": "k_iter_small<L=2>", "tile-2d": "k_iter_tile<D=2,", "tile-1d": "k_iter_tile<D=1,", "tall": "k_iter_tall<", "elem": "k_iter_elem<",
            "separate": "k_project_wg<20x20/10x10>", "reverse-projection": "proj=20x20/10x10", "wide-H32": "k_fwd_wide<", "generic": "k_mlp_fwd_generic",
            "generic-small": "k_mlp_bwd_generic", "pinn-p1-generic": "k_mlp_fwd_generic + k_pinn_residual", "pinn-p2-generic": "k_mlp_fwd_generic + k_pinn_residual",
            "pinn-adv-generic": "k_mlp_fwd_generic + k_pinn_residual", "pinn-p1-mfma": "k_fwd_mfma<D=1,", "pinn-p2-mfma": "k_fwd_mfma<D=2,",
            "pinn-adv-mfma": "k_fwd_mfma<D=2,"}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """prints, when the module's last test has run, the instantiations every structure ran and the table of worst errors (pytest -rA / -s)"""
    yield
    print("\nstructures reached by the data-term sweeps (%d):" % len(REACHED))
    for k in REACHED:
        for v, ns in REACHED[k].items():
            print("  %-20s %-100s n = %s" % (k, v, ns))
    print("\npasses the whole-iteration plan declined (one workgroup count past the limit):")
    for k, rows in OVER.items():
        for n, v, ps in rows:
            print("  %-20s n = %-6d %s (%s)" % (k, n, v, ps))
    print("\n| structure | n | loss triple | gradient block | lossb slot | forward-only |")
    for (k, n), e in WORST.items():
        print("| %s | %d | %.1e | %.1e | %.1e | %.1e |" % ((k, n) + e))


def test_zz_every_structure_of_the_table_was_reached():
    """Runs last in the file: every structure of the table ran its own kernel family at least once, and every count past a
    whole-iteration kernel's limit ran SOMETHING that produced the right result (on its own, e.g. under -k, it fails: it judges the
    whole file)."""
    assert REACHED, "run the whole file: this test judges what the cases above reached"
    missing = [k for k, f in FAMILIES.items() if not any(f in v for v in REACHED.get(k, {}))]
    assert not missing, (missing, {k: list(v) for k, v in REACHED.items()})
    assert set(OVER) == {k for k, s in dr.STRUCTURES.items() if s["edge"] == "wg"}, sorted(OVER)
