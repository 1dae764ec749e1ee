"""Shape sweep of the variable-coefficient kernels (k_project_lin, k_project_nl, k_project_id, k_lin_indicators, k_ansatz_fwd /
k_ansatz_adj) on the device against the CPU references, over the case table of tests/linop_sweep.py: the shapes at which each
`idx += 256` loop of these run-time-shaped kernels takes another number of trips, the extents that are 1, the strongly non-square
rules, one-sided zero-weight padding, and both sides of the 64 KiB LDS guard.  tests/test_linop_sweep_host.py proves every fixed case
on the CPU; profiles/linop_sweep.md holds the measured errors.

Every case: loss triple, forward-only loss, gradient per block (the d c block included) and the validation sums within TOL = 1e-9
(test_gpu_ansatz._against_reference, unchanged); hpv_get_residuals within TOL of the reference's norm and exactly 0 where the counts
mask; a second loss_and_grad bit-equal to the first; the kernel's name and shape in the variant string.  The rows of
linop_sweep.ALL_VARIANTS also take eight Adam steps against ansatz_reference.adam_trajectory within STEP_TOL = 1e-8, through the
captured graphs and with HPV_NO_GRAPH=1.  Six further cases rotate with HPV_FUZZ_SEED (tests/test_gpu_fuzz.py)."""
import numpy as np
import pytest

import ansatz_reference as ar
import generic_point as gp
import linadapt_reference as la
import linear_reference as lr
import linop_sweep as ls
import test_gpu_linadapt as tla
from cases import rel
from test_gpu_ansatz import Dev, _against_reference, _rel3
from test_gpu_fuzz import FUZZ_SEED
from test_gpu_generic_point import STEP_TOL, TOL

pytestmark = pytest.mark.gpu

FIXED = ls.fixed_cases()
BY_NAME = {c["name"]: c for c in FIXED}
STEPS = 8
SEED_TAG = "HPV_FUZZ_SEED=%d" % FUZZ_SEED
_PROBLEMS = {}
_TRAJ = {}
WORST = {}          # case -> [loss, worst block, residuals, steps]
REACHED = set()     # (kernel, dim, ansatz)


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _problem(name):
    """the fixed case's arrays and its reference (loss triple, gradient, R), computed once and left unchanged"""
    if name not in _PROBLEMS:
        p = ls.problem(BY_NAME[name])
        _PROBLEMS[name] = (p, ar.reference(p))
    return _PROBLEMS[name]


def _mask(p):
    ne, ntx, nty = p["ee"] - p["eb"], p["ntx"], p["nty"]
    nax = np.full(ne, ntx) if p["nax"] is None else p["nax"][p["eb"]:p["ee"]]
    nay = np.full(ne, nty) if p["nay"] is None else p["nay"][p["eb"]:p["ee"]]
    return (np.arange(ntx)[None, None, :] < nax[:, None, None]) & (np.arange(nty)[None, :, None] < nay[:, None, None])


def _check(name, variant, d, ref):
    """everything the module docstring lists per case, on the live handle `d` against `ref` = (loss triple, gradient, R)"""
    p = d.p
    tag = "%s [%s]" % (name, SEED_TAG)
    first = d.loss_and_grad()
    v = _against_reference(tag, d, ref, validation=d.has_val)
    # the kernel and its shape
    qx, qy = p["xr"][0].size, 1 if p["yr"] is None else p["yr"][0].size
    want = "%s%dx%d/%dx%d" % (ls.KERNEL[variant], qx, qy, p["ntx"], p["nty"])
    assert want in v and (";ansatz>" in v) == (p["ans"] is not None), (tag, "wanted", want, "ran", v)
    assert d.h.lib.hpv_pass_structure(d.h._h) == 0, (tag, v)
    REACHED.add((variant, p["dim"], p["ans"] is not None))
    # residuals
    Ro = ref[2]
    Rm = d.h.residuals(Ro.size).reshape(Ro.shape)
    eR = float(np.linalg.norm(Rm - Ro) / np.linalg.norm(Ro))
    m = _mask(p)
    print("%s | residuals %.2e | %d of %d entries masked" % (tag, eR, int((~m).sum()), m.size))
    assert eR < TOL, (tag, v, "residuals", eR)
    assert np.all(Rm[~m] == 0.0) and np.all(Ro[~m] == 0.0), (tag, v, "masked residual entries are exactly 0")
    # a second pass: the same bits
    again = d.loss_and_grad()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), (tag, v, "a second loss_and_grad differs from the first")
    e3 = float(_rel3(first[0], ref[0]).max())
    eb = float(gp.worst_block(first[1], ref[1], p["layers"], d.nc)[1])
    WORST[name] = [e3, eb, eR, float("nan")]
    return v


# ---- the fixed table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BY_NAME))
def test_fixed_shape_against_the_reference(name):
    c = BY_NAME[name]
    p, ref = _problem(name)
    d = Dev(p)
    v = _check(name, c["variant"], d, ref)
    wide = p["layers"][1] == 24
    assert ("k_fwd_wide<" in v and "H=24>" in v) if wide else "k_fwd_mfma<" in v, (name, v)


STEP_CASES = [c["name"] for c in FIXED if c["row"] in ls.ALL_VARIANTS]


@pytest.mark.parametrize("graph", [True, False], ids=["graphs", "no-graph"])
@pytest.mark.parametrize("name", STEP_CASES)
def test_eight_adam_steps(name, graph, monkeypatch):
    p, _ = _problem(name)
    if not graph:
        monkeypatch.setenv("HPV_NO_GRAPH", "1")
    d = Dev(p, validation=False)
    d.h.step(STEPS, False)
    v = d.h.kernel_variant()
    assert d.h.graphs_in_use() == graph and ls.KERNEL[BY_NAME[name]["variant"]] in v, (name, graph, v)
    if name not in _TRAJ:
        _TRAJ[name] = ar.adam_trajectory(p, STEPS)
    e = float(rel(d.params(), _TRAJ[name]))
    print("%s | %d Adam steps, graphs %s: parameters %.2e" % (name, STEPS, graph, e))
    w = WORST.setdefault(name, [float("nan")] * 4)
    w[3] = e if np.isnan(w[3]) else max(w[3], e)
    assert e < STEP_TOL, (name, v, "parameters after %d Adam steps" % STEPS, "graphs %s" % graph, e)


# ---- the rotating part -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(ls.N_ROTATING), ids=["rotating%d" % i for i in range(ls.N_ROTATING)])
def test_rotating_shape_against_the_reference(i):
    c, p, tries = ls.rotating_case(FUZZ_SEED, i)       # the reference alone, before the device is touched
    if c is None:
        pytest.fail("rotating%d [%s]: no draw out of %d keeps the conditions on the reference: %s" % (i, SEED_TAG, tries, p))
    print("rotating%d [%s], draw %d: %s" % (i, SEED_TAG, tries, {k: v for k, v in c.items() if k != "boxes"}))
    _check("rotating%d" % i, c["variant"], Dev(p), ar.reference(p))


# ---- a smaller mesh on a live handle ---------------------------------------------------------------------------------------------------
def test_shrinking_on_a_live_handle():
    """four boxes of the nr272 shape, a pass; then one box on the same handle, planes set again: loss_e, R and GBAR rows of the larger
    batch must not reach the loss, the gradient or the residuals; then counts (1, 1) on that handle"""
    c4 = dict(BY_NAME["nr272-lin"], boxes=lr.BOXES2)
    p4 = ls.problem(c4)
    d = Dev(p4, validation=False)
    _check("nr272 on four boxes", "lin", d, ar.reference(p4))
    c1 = dict(c4, boxes=lr.BOXES2[3:])
    p1 = ls.problem(c1)
    d.p = p1
    d.h.set_rhs(None)
    d.h.set_element_boxes(p1["boxes"], p1["eb"], p1["ee"])
    d.h.set_rhs(p1["F"].reshape(-1))
    d.set_planes()
    _check("nr272 shrunk to one box", "lin", d, ar.reference(p1))
    p1c = ls.problem(dict(c1, counts=([1], [1])))
    assert np.array_equal(p1c["planes"], p1["planes"]) and np.array_equal(p1c["F"], p1["F"])
    d.p = p1c
    d.set_counts()
    ref = ar.reference(p1c)
    assert np.count_nonzero(ref[2]) == 1
    _check("nr272 shrunk to one box, counts (1, 1)", "lin", d, ref)


# ---- both sides of the 64 KiB guard -------------------------------------------------------------------------------------------------------
def _refused(call, what):
    """the call is refused on the host with -1 (never -2, a launch failure)"""
    from hp_vpinns_amd import _lib
    with pytest.raises(_lib.HpvError) as e:
        call()
    assert e.value.code == -1 and "LDS" in str(e.value), (what, e.value.code, str(e.value))


@pytest.mark.parametrize("variant", ["lin", "nl", "id"])
def test_lds_limit(variant):
    """ldsmax runs and matches; each neighbour shape is refused by hpv_set_tables with -1; the same handle then takes an admitted
    shape and matches its reference; with admitted tables in place a refused hpv_set_tables leaves the handle as it was"""
    from hp_vpinns_amd.testfcn import tables_1d
    p, ref = _problem("ldsmax-" + variant)
    d = Dev(p)
    _check("ldsmax-%s before the refusals" % variant, variant, d, ref)
    nt = ls.LDSMAX_NT
    # with the admitted rule still in place: more functions than fit -- the handle keeps its tables and its numbers
    xi, yi = p["xr"][0], p["yr"][0]
    _refused(lambda: d.h.set_tables(tables_1d(nt + 1, xi), tables_1d(nt + 1, yi)), "ldsmax rule with 18 x 18 functions")
    l3, g = d.loss_and_grad()
    assert "/%dx%d" % (nt, nt) in d.h.kernel_variant()
    assert _rel3(l3, ref[0]).max() < TOL and gp.worst_block(g, ref[1], p["layers"], d.nc)[1] < TOL, (variant, "after a refused hpv_set_tables", l3, ref[0])
    for qx, qy in ls.LDS_NEIGHBOURS:
        (x, wx), (y, wy) = lr.rule(qx), lr.rule(qy)
        d.h.set_quadrature(x, wx, y, wy)
        _refused(lambda: d.h.set_tables(tables_1d(nt, x), tables_1d(nt, y)), (qx, qy, ls.lds_bytes(qx, qy, nt, nt)))
    p2, ref2 = _problem("nq272-" + variant)
    d.populate(p2)
    _check("nq272-%s after the refusals" % variant, variant, d, ref2)


def test_lds_limit_1d():
    from hp_vpinns_amd.testfcn import tables_1d
    p, ref = _problem("1d-272-lin")
    d = Dev(p)
    xi = p["xr"][0]
    for n in ls.NT1D_REFUSED:
        _refused(lambda: d.h.set_tables(tables_1d(n, xi)), (ls.Q1D, n, ls.lds_bytes(ls.Q1D, 1, n, 1)))
    _check("1d-272-lin after the refusals", "lin", d, ref)


# ---- the indicator kernel ---------------------------------------------------------------------------------------------------------------
QI = ls.largest_indicator_rule()
IND_CASES = {
    "min": la._c("ind-min", la.S8, la.BOXES2[3:4], (3, 3), (1, 1), 9981),
    "nq256": la._c("ind-nq256", la.S8, la.BOXES2[:2], (16, 16), (8, 8), 9982),
    "nq272": la._c("ind-nq272", la.S8, la.BOXES2[:3], (17, 16), (5, 4), 9983),
    "largest": la._c("ind-largest", la.S8, la.BOXES2[3:4], (QI, QI), (3, 3), 9984),
}


@pytest.mark.parametrize("name", list(IND_CASES))
def test_indicators_against_the_reference(name):
    p = la.problem(IND_CASES[name])
    d = tla.Dev(p)
    ind, r = tla._against_reference("%s %s" % (IND_CASES[name]["name"], IND_CASES[name]["q"]), d, la.reference(p))
    ind2, r2 = d.h.linear_indicators(p["f"], want_r=True)
    assert ind2.tobytes() == ind.tobytes() and r2.tobytes() == r.tobytes()


def test_indicator_rule_past_the_limit_is_refused():
    from hp_vpinns_amd import _lib
    q = QI + 1
    p = la.problem(la._c("ind-past", la.S8, la.BOXES2[3:4], (q, q), (3, 3), 9985))
    d = tla.Dev(p, strong=False)                       # (hpv_set_tables admits the shape)
    l0, g0 = d.loss_and_grad()
    _refused(lambda: d.h.set_strong_form(*d.D), (q, la.lds_bytes(2, q, q)))
    with pytest.raises(_lib.HpvError) as e:            # no matrices, no launch
        d.h.linear_indicators(p["f"])
    assert e.value.code != -2, (e.value.code, str(e.value))
    l1, g1 = d.loss_and_grad()
    assert np.array_equal(l0, l1) and np.array_equal(g0, g1)


# ---- the report and the coverage -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _report():
    """prints, when the module's last test has run, the errors of every case (pytest -rA / -s)"""
    yield
    print("\n%s\ncase | loss | worst block | residuals | eight steps" % SEED_TAG)
    for k, e in WORST.items():
        print("  %-42s %.2e %.2e %.2e %.2e" % ((k,) + tuple(e)))
    if WORST:
        w = np.array(list(WORST.values()))
        print("worst over %d cases: loss %.2e, block %.2e, residuals %.2e, steps %.2e" % ((len(WORST),) + tuple(np.nanmax(w, axis=0))))


def test_zz_the_sweep_reached_every_kernel():
    """Runs last in the file: the cases above, together, reached all three projection kernels, in 1-D and in 2-D, with and without
    the ansatz (on its own, e.g. under -k, it fails: it judges the whole file)"""
    assert REACHED, "run the whole file: this test judges what the cases above reached"
    print("reached: %s" % sorted(REACHED))
    assert {r[0] for r in REACHED} == {"lin", "nl", "id"} and {r[1] for r in REACHED} == {1, 2} and {r[2] for r in REACHED} == {True, False}, sorted(REACHED)
    for k in ("lin", "nl", "id"):
        assert {r[1] for r in REACHED if r[0] == k} == {1, 2}, (k, sorted(REACHED))
    assert {r[0] for r in REACHED if r[2]} >= {"nl", "id"}, sorted(REACHED)
