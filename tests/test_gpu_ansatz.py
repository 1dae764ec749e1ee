"""Exact Dirichlet conditions by ansatz u = G + D N (hpv_set_ansatz, k_ansatz_fwd / k_ansatz_adj, VPINNLinear(hard_bc=...)) on the
device against tests/ansatz_reference.py (CPU, fp64; tests/test_ansatz_host.py proves it); measurements in profiles/hard_bc.md.

Every row of ansatz_reference.CASES (21, 180 and 840 quadrature points; 1 and 17 data points, 3 flux points, 33 validation points;
the linear operator alone, with all four nonlinear terms, with two trainable coefficients): loss triple, forward-only loss, gradient
per block and the six sums of hpv_validate.  Bounds (as tests/test_gpu_linear.py uses them): TOL = 1e-9 on the
loss triple, the validation sums and the gradient per block, STEP_TOL = 1e-8 on the parameters after Adam steps."""
import numpy as np
import pytest

import ansatz_reference as ar
import flux_reference as fr
import generic_point as gp
from cases import rel
from test_gpu_generic_point import STEP_TOL, TOL

pytestmark = pytest.mark.gpu

_PROBLEMS = {}
SETS = ("quad", "data", "flux", "val")      # HPV_ANSATZ_QUAD .. HPV_ANSATZ_VALID, in that order


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _problem(name, kind="generic"):
    """the case's arrays and its reference (loss triple, gradient, R), computed once and left unchanged"""
    if (name, kind) not in _PROBLEMS:
        p = ar.problem(ar.CASES[name], kind)
        _PROBLEMS[(name, kind)] = (p, ar.reference(p))
    return _PROBLEMS[(name, kind)]


class Dev:
    """the C-ABI on problem dict `p`: a narrow network is zero-padded onto its device width as the Python classes do (init.pad_plan)"""

    def __init__(self, p, ansatz=True, validation=True):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.init import n_params, pad_plan
        self.p, L, self.nc = p, p["layers"], p["c0"].size
        plan = pad_plan(L, self.nc)
        self.dev_layers, self.idx = plan if plan is not None else (L, None)
        self.n_dev = n_params(self.dev_layers, self.nc)
        self.h = _lib.Handle(_lib.PDE_LINEAR1D if p["dim"] == 1 else _lib.PDE_LINEAR2D, 1, _lib.ACT_SIN if p["act"] == "sin" else _lib.ACT_TANH,
                             self.dev_layers, lr=1e-3, lossb_weight=p["lbw"], n_coef=self.nc)
        self.populate(p, ansatz, validation)

    def populate(self, p, ansatz=True, validation=True):
        """rule, tables, elements, F, counts, planes and point sets of problem dict `p` (same network, same n_coef) on the live handle --
        a data or flux set the problem lacks is removed, validation=False leaves the handle without a validation set --, the ansatz
        planes of the sets that exist where p has an ansatz, and p's parameters"""
        from hp_vpinns_amd.testfcn import tables_1d
        self.p, h = p, self.h
        h.set_rhs(None)                                 # (per-grid inputs of an earlier, other mesh)
        h.set_active_tests(None)
        (xi, wx), yr = p["xr"], p["yr"]
        h.set_quadrature(xi, wx, *(yr if yr is not None else (None, None)))
        h.set_tables(tables_1d(p["ntx"], xi), None if yr is None else tables_1d(p["nty"], yr[0]))
        h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
        h.set_rhs(p["F"].reshape(-1))
        self.set_counts()
        self.set_planes()
        h.set_data(*(p["data"] if p["data"] is not None else (None, None)))
        if p["flux"] is not None:
            h.set_flux_data(p["flux"]["X"], fr.coef(p["flux"]), p["flux"]["g"], fr.W_F)
        else:
            h.set_flux_data(None, None, None)
        self.has_val = validation
        if validation:
            h.set_validation(*p["val"])
        else:
            h.set_validation(None, None)
        if ansatz and p["ans"] is not None:
            self.set_ansatz([k for k in SETS if p["ans"][k] is not None and (k != "val" or validation)])
        self.set_params(p["full"])

    def set_counts(self):
        p, h = self.p, self.h
        if p["nax"] is None:
            h.set_active_tests(None)
        elif p["dim"] == 1:
            h.set_active_tests(p["nax"])
        else:
            h.set_active_tests_2d(p["nax"], p["nay"])

    def set_planes(self):
        p, h = self.p, self.h
        h.set_operator(p["planes"])
        if p["terms"]:
            h.set_nonlinear(p["nl"])
        if self.nc:
            h.set_trainable(p["dirs"])

    def set_ansatz(self, sets=SETS, A=None):
        A = self.p["ans"] if A is None else A
        for k in sets:
            self.h.set_ansatz(SETS.index(k), None if A is None else A[k])

    def set_params(self, th):
        t = np.asarray(th, dtype=np.float64)
        if self.idx is not None:
            t = np.zeros(self.n_dev)
            t[self.idx] = th
        self.h.set_params(t)

    def params(self):
        t = self.h.get_params()
        return t if self.idx is None else t[self.idx]

    def loss_and_grad(self):
        l3, g = self.h.loss_and_grad(True)
        if self.idx is not None:
            pad = np.ones(g.size, dtype=bool)
            pad[self.idx] = False
            assert np.all(g[pad] == 0.0)                # (a padded neuron's gradient entries are exact zeros)
            g = g[self.idx]
        return np.asarray(l3), g


def _rel3(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def _against_reference(tag, d, ref, validation=True):
    p = d.p
    l3o, go, _ = ref
    l3m, gm = d.loss_and_grad()
    v = d.h.kernel_variant()
    lf = d.h.loss_and_grad(False)[0]
    e3, ef = _rel3(l3m, l3o), _rel3(lf, l3o)
    kb, eb = gp.worst_block(gm, go, p["layers"], d.nc)
    ev = _rel3(d.h.validate(), ar.validation(p)) if validation else np.zeros(1)
    print("%s | %s | loss3 %s | worst block %s %.2e (global %.2e) | forward-only %s | validation %s" % (tag, v, e3, kb, eb, rel(gm, go), ef, ev))
    assert e3.max() < TOL, (tag, v, "loss triple", l3m, l3o)
    assert eb < TOL, (tag, v, "gradient block", kb, eb)
    assert ef.max() < TOL, (tag, v, "forward-only pass", lf, l3o)
    assert ev.max() < TOL, (tag, v, "validation sums", ev)
    return v


@pytest.mark.parametrize("name", list(ar.CASES))
def test_loss_gradient_and_validation_against_the_reference(name):
    p, ref = _problem(name)
    d = Dev(p)
    v = _against_reference(name, d, ref)
    kernel = {"lin": "k_project_lin<", "nl": "k_project_nl<", "id": "k_project_id<"}[ar.CASES[name]["variant"]]
    assert kernel in v and ";ansatz>" in v and d.h.lib.hpv_pass_structure(d.h._h) == 0, v
    if name.endswith("d17"):      # the validation set without exact gradients: a value-only batch, one channel
        d.h.set_validation(p["val"][0], p["val"][1])
        d.h.set_ansatz(3, p["ans"]["val"])
        ev = _rel3(d.h.validate(), ar.validation(p, with_du=False))
        assert ev.max() < TOL, (name, "value-only validation", ev)


_TRAJ = {}


@pytest.mark.parametrize("graph", [True, False])
def test_twenty_adam_steps(graph, monkeypatch):
    """the 180-point case against the reference's TF1-rule Adam: through the captured iteration graphs, and with HPV_NO_GRAPH=1"""
    name = "2d-180-nl-d17"
    p, _ = _problem(name)
    if not graph:
        monkeypatch.setenv("HPV_NO_GRAPH", "1")
    d = Dev(p)
    d.h.step(20, False)
    assert d.h.graphs_in_use() == graph and ";ansatz>" in d.h.kernel_variant()
    if name not in _TRAJ:
        _TRAJ[name] = ar.adam_trajectory(p, 20)
    e = rel(d.params(), _TRAJ[name])
    print("%s, 20 Adam steps, graphs %s: parameters %.2e" % (name, graph, e))
    assert e < STEP_TOL


def test_bytes_with_without_and_after_removal():
    name = "2d-180-id-d17"
    p, ref = _problem(name)
    plain = Dev(p, ansatz=False)
    l0, g0 = plain.loss_and_grad()
    d = Dev(p)
    a, b = d.loss_and_grad(), d.loss_and_grad()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], l0)
    va = d.h.validate()
    assert np.array_equal(va, d.h.validate())
    d.set_ansatz(A={k: None for k in SETS})
    l1, g1 = d.loss_and_grad()
    assert ";ansatz" not in d.h.kernel_variant()
    assert np.array_equal(l1, l0) and np.array_equal(g1, g0)
    assert np.array_equal(d.h.validate(), plain.h.validate())
    d.h.step(3, False)
    plain.h.step(3, False)
    assert np.array_equal(d.h.get_params(), plain.h.get_params())
    d.set_ansatz()                                       # ... and back: the reference's numbers again
    d.set_params(p["full"])
    _against_reference(name + " set again", d, ref)


@pytest.mark.parametrize("name", ["1d-21-lin-d1", "2d-180-nl-d17"])
def test_identity_ansatz_against_the_plain_handle(name):
    """G = 0, D = 1: the data term runs in a batch of its own, so the bytes may differ from the merged launch's"""
    p, _ = _problem(name, "identity")
    l0, g0 = Dev(p, ansatz=False).loss_and_grad()
    d = Dev(p)
    l1, g1 = d.loss_and_grad()
    kb, eb = gp.worst_block(g1, g0, p["layers"], d.nc)
    print("%s identity: loss %s, worst block %s %.2e" % (name, _rel3(l1, l0), kb, eb))
    assert ";ansatz>" in d.h.kernel_variant() and _rel3(l1, l0).max() < TOL and eb < TOL


def test_refusals_leave_the_handle_usable():
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.quadrature import diff_matrix
    name = "2d-180-lin-d17"
    p, ref = _problem(name)
    d = Dev(p)
    A = p["ans"]

    def refused(call, code=-1, word=None):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == code and (word is None or word in str(e.value)), (e.value.code, str(e.value))
    bad = A["quad"].copy()
    bad[4, 7] = np.nan
    refused(lambda: d.h.set_ansatz(0, A["quad"][:, :-1]))
    refused(lambda: d.h.set_ansatz(1, A["quad"]))
    refused(lambda: d.h.set_ansatz(0, bad))
    refused(lambda: d.h.set_ansatz(4, A["quad"]))
    refused(lambda: d.h.set_strong_form(diff_matrix(p["xr"][0]), diff_matrix(p["yr"][0])))
    _against_reference("after five refusals", d, ref)
    # another pde
    other = _lib.Handle(_lib.PDE_POISSON2D, 1, _lib.ACT_TANH, [2, 20, 20, 1])
    refused(lambda: other.set_ansatz(1, A["data"]))
    # the strong form active on a handle without an ansatz
    s = Dev(p, ansatz=False)
    l0, g0 = s.loss_and_grad()
    s.h.set_strong_form(diff_matrix(p["xr"][0]), diff_matrix(p["yr"][0]))
    refused(lambda: s.h.set_ansatz(0, A["quad"]))
    l1, g1 = s.loss_and_grad()
    assert np.array_equal(l0, l1) and np.array_equal(g0, g1)
    s.h.set_strong_form(None, None)
    s.set_ansatz()
    _against_reference("after the strong form left", s, ref)
    # hpv_set_data drops the DATA planes, hpv_set_validation those of VALID: -3 until they are set again
    d.h.set_data(*p["data"])
    refused(lambda: d.h.loss_and_grad(True), -3, "set DATA")
    refused(lambda: d.h.step(1, False), -3, "set DATA")
    d.set_ansatz(("data",))
    d.h.set_validation(*p["val"])
    refused(lambda: d.h.validate(), -3, "set VALID")
    d.set_ansatz(("val",))
    _against_reference("after new data", d, ref)
    # hpv_set_element_boxes drops QUAD
    d.h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
    d.set_planes()
    refused(lambda: d.h.loss_and_grad(True), -3, "set QUAD")
    d.set_ansatz(("quad",))
    _against_reference("after new elements", d, ref)


def test_python_class_boundary_layer_with_exact_conditions():
    """1-D boundary layer with hard_bc and no X_u_train: the end values to the last bit before and after training and on a bisected
    mesh, a decreasing loss, and the class's loss against the reference's for its own fields"""
    from hp_vpinns_amd.adapt import ElementMesh
    from hp_vpinns_amd.drivers import linear
    from hp_vpinns_amd.vpinn import VPINNLinear
    ua, ub = 0.25, -0.5
    grid = linear.graded_grid(3)
    m = VPINNLinear([1, 8, 8, 1], grid_x=grid, n_quad=8, n_test=4, kappa=-0.2, beta=1.0, sigma=0.0, f=1.0, activation="sin", LR=5e-3,
                    hard_bc=linear.interval_hard_bc(0.0, 1.0, ua, ub))
    ends, want = np.array([[0.0], [1.0]]), np.array([ua, ub])
    assert m.X_u_train is None and np.array_equal(m.predict(ends).reshape(-1), want)
    l0 = m.loss()
    assert l0[1] == 0.0 and l0[0] == l0[2]               # no boundary term at all
    m.train(50)
    assert ";ansatz>" in m.h.kernel_variant() and m.h.graphs_in_use()
    l1 = m.loss()
    print("boundary layer with exact conditions: loss %.4e -> %.4e after 50 steps" % (l0[0], l1[0]))
    assert l1[0] < l0[0] and np.array_equal(m.predict(ends).reshape(-1), want)
    ev = m.evaluate(ends)
    assert sorted(ev) == ["u", "u_x"] and np.array_equal(ev["u"].reshape(-1), want)
    fine = np.sort(np.concatenate([grid, 0.5 * (grid[:-1] + grid[1:])]))
    m.set_mesh(ElementMesh(ElementMesh.from_grid(fine).boxes, 4))
    m.train(10)
    assert len(m.mesh) == 6 and np.all(np.isfinite(m.loss_his)) and np.array_equal(m.predict(ends).reshape(-1), want)
    # the constructor's checks
    with pytest.raises(ValueError, match="'d'"):
        VPINNLinear([1, 8, 8, 1], grid_x=grid, n_quad=8, n_test=4, hard_bc=dict(g=0.0, d=lambda P: np.stack([P[:, 0] * (1 - P[:, 0]), 1 + 2 * P[:, 0]], 1)))
    with pytest.raises(ValueError, match="strong_form"):
        VPINNLinear([1, 8, 8, 1], grid_x=grid, n_quad=8, n_test=4, strong_form="elementwise", hard_bc=linear.interval_hard_bc(0.0, 1.0, ua, ub))
    # set_hard_bc on the live model: removal gives the raw network back, parameters kept
    th = m.get_params()
    m.set_hard_bc()
    assert ";ansatz" not in (m.loss_and_grad() and m.h.kernel_variant()) and np.array_equal(m.get_params(), th)
    assert not np.array_equal(m.predict(ends).reshape(-1), want)
    m.set_hard_bc(g=1.5, d=linear.interval_hard_bc(0.0, 1.0, 0.0, 0.0)["d"])
    assert np.array_equal(m.predict(ends).reshape(-1), [1.5, 1.5]) and np.isfinite(m.loss()[0]) and np.array_equal(m.get_params(), th)
