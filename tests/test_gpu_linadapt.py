"""The element-wise strong form of the variable-coefficient classes on the device (hpv_set_strong_form, hpv_linear_indicators,
k_lin_indicators; VPINNLinear(strong_form="elementwise")) against tests/linadapt_reference.py (CPU, fp64; tests/test_linadapt_host.py
proves it and the well-posedness of every case here); the measured errors are in profiles/linear_adaptivity.md.

Bounds: TOL = 1e-9 as in tests/test_gpu_adapt.py -- relative per indicator column, and on the strong residual relative to max|r|."""
import numpy as np
import pytest

import linadapt_reference as la
from cases import rel

pytestmark = pytest.mark.gpu

TOL = 1e-9
_REF = {}


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _case(name):
    """the case's arrays and its reference, computed once and left unchanged"""
    if name not in _REF:
        p = la.twin_problem() if name == "twin" else la.class_problem() if name == "class" else la.problem(la.CASES[name])
        _REF[name] = (p, la.reference(p))
    return _REF[name]


class Dev:
    """the C-ABI on problem dict `p` of linadapt_reference: the sequence of tests/test_gpu_ident.Dev (operator, nonlinear term where
    the case has one, directions where it has coefficients), then hpv_set_strong_form unless strong=False"""

    def __init__(self, p, strong=True, backend=None, pde=None):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.init import n_params, pad_plan
        from hp_vpinns_amd.quadrature import diff_matrix
        from hp_vpinns_amd.testfcn import tables_1d
        self.p, L = p, p["layers"]
        self.nc = nc = 0 if pde is not None else p["dirs"].shape[0]
        plan = pad_plan(L, nc)
        self.dev_layers, self.idx = plan if plan is not None else (L, None)
        self.n_dev = n_params(self.dev_layers, nc)
        kw = {} if backend is None else dict(backend=backend)
        self.linear = pde is None
        if pde is None:
            pde = _lib.PDE_LINEAR1D if p["dim"] == 1 else _lib.PDE_LINEAR2D
        self.h = h = _lib.Handle(pde, 1, _lib.ACT_SIN if p["act"] == "sin" else _lib.ACT_TANH, self.dev_layers, lr=1e-3,
                                 lossb_weight=p["lbw"], V=0.6, n_coef=nc, **kw)
        self.populate(p, strong)
        self.set_params(np.concatenate([p["theta"], p["c0"]]) if nc else p["theta"])

    def populate(self, p, strong=True):
        """rule, tables, elements, F, counts, planes and (strong) the differentiation matrices of problem dict `p` on the live handle"""
        from hp_vpinns_amd.quadrature import diff_matrix
        from hp_vpinns_amd.testfcn import tables_1d
        self.p, h = p, self.h
        (xi, wx), yr = p["xr"], p["yr"]
        h.set_quadrature(xi, wx, *(yr if yr is not None else (None, None)))
        h.set_tables(tables_1d(p["ntx"], xi), None if yr is None else tables_1d(p["nty"], yr[0]))
        h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
        h.set_rhs(p["F"].reshape(-1))
        if p["nax"] is not None:
            if p["dim"] == 1:
                h.set_active_tests(p["nax"])
            else:
                h.set_active_tests_2d(p["nax"], p["nay"])
        if self.linear:
            h.set_operator(p["planes"])
            if np.any(p["nl"] != 0.0):
                h.set_nonlinear(p["nl"])
            if self.nc:
                h.set_trainable(p["dirs"])
        self.D = (diff_matrix(xi), None if yr is None else diff_matrix(yr[0]))
        if strong:
            h.set_strong_form(*self.D)

    def loss_and_grad(self):
        l3, g = self.h.loss_and_grad(True)
        return np.asarray(l3), (g if self.idx is None else g[self.idx])

    def set_params(self, th):
        t = np.asarray(th, dtype=np.float64)
        if self.idx is not None:
            t = np.zeros(self.n_dev)
            t[self.idx] = th
        self.h.set_params(t)

    def everything(self):
        """(loss triple, gradient, residuals, parameters): what a pass and an update leave behind"""
        l3, g = self.h.loss_and_grad(True)
        p = self.p
        return np.asarray(l3), g, self.h.residuals((p["ee"] - p["eb"]) * p["ntx"] * p["nty"]), self.h.get_params()


def _col_err(ind, ref):
    return np.array([rel(ind[:, c], ref[:, c]) if np.any(ref[:, c] != 0.0) else float(np.abs(ind[:, c]).max()) for c in range(5)])


def _against_reference(tag, d, ref, f="case"):
    p = d.p
    fq = p["f"] if f == "case" else f
    ind, r = d.h.linear_indicators(fq, want_r=True)
    ec = _col_err(ind, ref["ind"])
    er = float(np.abs(r.reshape(ref["r"].shape) - ref["r"]).max() / np.abs(ref["r"]).max())
    print("%s | columns %s | r %.2e (max|r| %.3g)" % (tag, np.array2string(ec, precision=2), er, np.abs(ref["r"]).max()))
    assert ec.max() < TOL, (tag, "indicator columns", ec)
    assert er < TOL, (tag, "strong residual", er)
    if p["dim"] == 1:
        assert np.all(ind[:, 4] == 0.0)
    return ind, r


@pytest.mark.parametrize("name", list(la.CASES))
def test_cases_against_the_reference(name):
    p, ref = _case(name)
    d = Dev(p)
    ind, r = _against_reference("%s backend %d" % (name, d.h.backend_in_use()), d, ref)
    # f_quad NULL vs given, r_out NULL vs given: the five columns are the same bytes within each pair
    assert d.h.linear_indicators(p["f"]).tobytes() == ind.tobytes()
    z, rz = d.h.linear_indicators(None, want_r=True)
    assert d.h.linear_indicators(None).tobytes() == z.tobytes()
    assert d.h.linear_indicators(np.zeros_like(p["f"])).tobytes() == z.tobytes()
    ref0 = la.reference(p, f=0.0)
    assert _col_err(z, ref0["ind"]).max() < TOL
    # two calls: the same bytes
    ind2, r2 = d.h.linear_indicators(p["f"], want_r=True)
    assert ind2.tobytes() == ind.tobytes() and r2.tobytes() == r.tobytes()


def test_generic_backend():
    from hp_vpinns_amd import _lib
    p, ref = _case("2d-7x5")
    d = Dev(p, backend=_lib.BACKEND_GENERIC)
    assert d.h.backend_in_use() == _lib.BACKEND_GENERIC
    _against_reference("2d-7x5 generic", d, ref)


def test_poisson_twin():
    """kappa = 1, beta = sigma = 0 on seven boxes is Poisson-2D var_form 1: the five columns of hpv_element_indicators"""
    from hp_vpinns_amd import _lib
    p, ref = _case("twin")
    lin, poi = Dev(p), Dev(p, strong=False, pde=_lib.PDE_POISSON2D)
    a = _against_reference("twin", lin, ref)[0]
    b = poi.h.element_indicators(p["f"])
    e = _col_err(a, b)
    print("twin | linear vs Poisson-2D handle, columns %s" % np.array2string(e, precision=2))
    assert e.max() < TOL


def test_training_is_not_disturbed():
    """a call between two step(3)s whose graph is captured, and a set / remove pair anywhere: bitwise the twin that never opted in"""
    p, _ = _case("id-6x5")
    a, b = Dev(p), Dev(p, strong=False)
    for d in (a, b):
        d.h.step(3)
    assert a.h.graphs_in_use() and b.h.graphs_in_use()
    a.h.linear_indicators(p["f"])
    a.h.set_strong_form(None, None)
    a.h.set_strong_form(*a.D)
    for d in (a, b):
        d.h.step(3)
    assert a.h.graphs_in_use()                                         # (nothing dropped the captured graph)
    a.h.set_strong_form(None, None)
    for x, y in zip(a.everything(), b.everything()):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert a.h.get_state().tobytes() == b.h.get_state().tobytes()


_LG = {}


def _usable(tag, d):
    """loss_and_grad of the live handle against linear_reference at the handle's current problem dict (bound TOL): the check of
    tests/test_gpu_linear.py after a refusal"""
    import linear_reference as lr
    p = d.p
    if id(p) not in _LG:
        _LG[id(p)] = (p, lr.reference(p)[:2])
    l3o, go = _LG[id(p)][1]
    l3m, gm = d.loss_and_grad()
    e3 = np.abs(l3m - np.asarray(l3o)) / np.where(np.asarray(l3o) == 0.0, 1.0, np.abs(l3o))
    print("%s | usable: loss3 %s grad %.2e" % (tag, np.array2string(e3, precision=2), rel(gm, go)))
    assert e3.max() < TOL and rel(gm, go) < TOL, (tag, l3m, l3o, rel(gm, go))


def test_refusals_leave_the_handle_usable():
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.quadrature import diff_matrix
    import linear_reference as lr
    p, ref = _case("2d-7x5")
    d = Dev(p, strong=False)
    _usable("start", d)

    def refused(call, code=-1, message=None):
        with pytest.raises(_lib.HpvError) as ei:
            call()
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        if message:
            assert message in str(ei.value), str(ei.value)

    Dx, Dy = d.D
    # no matrices set
    refused(lambda: d.h.linear_indicators(p["f"]), -1, "hpv_set_strong_form")
    _usable("no matrices", d)
    # wrong sizes (7 x 5: swapped; Dy missing; a row short), then NaN
    refused(lambda: d.h.set_strong_form(Dy, Dx))
    refused(lambda: d.h.set_strong_form(Dx, None))
    refused(lambda: d.h.set_strong_form(Dx[:-1], Dy))
    _usable("wrong sizes", d)
    bad = Dy.copy()
    bad[2, 3] = np.nan
    refused(lambda: d.h.set_strong_form(Dx, bad), -1, "non-finite")
    refused(lambda: d.h.linear_indicators(p["f"]), -1, "hpv_set_strong_form")          # (nothing of the refused calls stayed)
    _usable("NaN", d)
    d.h.set_strong_form(Dx, Dy)
    refused(lambda: d.h.linear_indicators(p["f"][:-1]))                                 # wrong n
    bad[2, 3] = np.inf
    refused(lambda: d.h.set_strong_form(Dx, bad), -1, "non-finite")                     # (the matrices given before stay)
    _against_reference("after refusals", d, ref)
    _usable("after refusals", d)
    # the old entry points stay refused on a linear handle, strong form or not
    refused(lambda: d.h.element_indicators(p["f"]))
    refused(lambda: d.h.residual_points(np.zeros((3, 2))))
    # hpv_set_quadrature with another rule drops the matrices; with everything of the new rule set again the SAME handle agrees with
    # the reference at that rule (the cached indicator buffers are re-keyed: 6 x 5 instead of 7 x 5 points per element)
    p2 = la.problem(dict(la.CASES["2d-7x5"], q=(6, 5)))
    (x2, w2), (y2, v2) = p2["xr"], p2["yr"]
    d.h.set_quadrature(x2, w2, y2, v2)
    refused(lambda: d.h.set_strong_form(Dx, Dy))                                        # (the old rule's sizes)
    refused(lambda: d.h.linear_indicators(None), -1, "hpv_set_strong_form")
    d.h.set_strong_form(diff_matrix(x2), diff_matrix(y2))
    refused(lambda: d.h.linear_indicators(None), -3)                                    # (where a pass would: no tables yet)
    d.populate(p2, strong=False)                                                        # (its hpv_set_quadrature drops them once more)
    refused(lambda: d.h.linear_indicators(p2["f"]), -1, "hpv_set_strong_form")
    d.h.set_strong_form(*d.D)
    _against_reference("after another rule", d, la.reference(p2))
    _usable("after another rule", d)
    # a Poisson handle
    pq = dict(p, planes=np.repeat(np.array([1.0, 1.0, 0.0, 0.0, 0.0])[:, None], p["planes"].shape[1], axis=1))
    q = Dev(pq, strong=False, pde=_lib.PDE_POISSON2D)
    refused(lambda: q.h.set_strong_form(Dx, Dy))
    refused(lambda: q.h.linear_indicators(p["f"]))
    _usable("Poisson handle", q)
    # a rule over the LDS limit, from the host formula: 1-D, 89 points fit, 90 do not; the refused handle then takes the case's own
    # 33-point rule back and agrees with the reference
    assert la.lds_bytes(1, 89, 1) <= 65536 < la.lds_bytes(1, 90, 1)
    c, cref = _case("1d-33-counts")
    e = Dev(c, strong=False)
    _usable("1-D start", e)
    for q_, ok in ((89, True), (90, False)):
        x, w = lr.rule(q_)
        e.h.set_quadrature(x, w)
        if ok:
            e.h.set_strong_form(diff_matrix(x))
        else:
            refused(lambda: e.h.set_strong_form(diff_matrix(x)), -1, "LDS")
            refused(lambda: e.h.linear_indicators(None), -1, "hpv_set_strong_form")
    e.populate(c)
    _against_reference("1d after LDS refusal", e, cref)
    _usable("1d after LDS refusal", e)


def _class_model(**kw):
    from hp_vpinns_amd.vpinn import VPINNLinear
    C = la.CLASS
    p, _ = _case("class")
    return VPINNLinear(C["layers"], grid_x=C["grid"], n_quad=C["n_quad"], n_test=C["n_test"], kappa=la.class_kappa, beta=1.0, sigma=0.0,
                       f=la.class_f, X_u_train=np.array([[0.0], [1.0]]), u_train=np.zeros(2), lossb_weight=p["lbw"], activation="sin",
                       LR=1e-3, init_params=p["theta"], **kw)


def test_class_with_the_keyword_adapts():
    from hp_vpinns_amd.adapt import ElementMesh, mark, refine
    p, ref = _case("class")
    m = _class_model(strong_form="elementwise")
    ind = m.element_indicators()
    r = m.strong_residual_at_quad()
    ec = _col_err(ind, ref["ind"])
    er = float(np.abs(r - ref["r"]).max() / np.abs(ref["r"]).max())
    print("class | columns %s | r %.2e" % (np.array2string(ec, precision=2), er))
    assert r.shape == ref["r"].shape and ec.max() < TOL and er < TOL
    mesh = ElementMesh(p["boxes"], p["ntx"])
    want = refine(mesh, mark(ref["ind"], mesh))
    before = m.h.get_state()
    new = m.adapt()
    assert len(new) > len(mesh)
    assert new.boxes.tobytes() == want.boxes.tobytes() and np.array_equal(new.nax, want.nax) and np.array_equal(new.nay, want.nay)
    assert m.h.get_state().tobytes() == before.tobytes()
    assert m.element_indicators().shape == (len(new), 5)               # (the matrices were handed over again with the new mesh)
    m.train(10)
    assert np.all(np.isfinite(m.loss_his[-10:]))
    rows = m.train_adaptive(6, 3, max_elements=len(new) + 1)
    assert len(rows) == 1 and rows[0][0] == 3 and np.isfinite(rows[0][2])
    with pytest.raises(NotImplementedError):
        m.residual(np.zeros((2, 1)))


def test_class_without_the_keyword_refuses_as_before():
    m = _class_model()
    for what in (m.element_indicators, m.adapt, m.strong_residual_at_quad, lambda: m.train_adaptive(10, 5), lambda: m.residual(np.zeros((2, 1)))):
        with pytest.raises(NotImplementedError):
            what()
    with pytest.raises(ValueError):
        _class_model(strong_form="pointwise")


def test_boundary_layer_driver_adapts():
    from hp_vpinns_amd.drivers import linear
    s = dict(linear.SMALLEST, n_iter=40)
    out = linear.run_boundary_layer(**s, adapt_every=20, max_elements=6, verbose=False)
    rows = out["adapt_rows"]
    print("boundary-layer driver:", rows)
    assert len(rows) == 1 and rows[0][0] == 20 and s["n_elements"] < rows[0][1] <= 6
    assert len(out["model"].mesh) == rows[0][1]
    assert np.isfinite(rows[0][2]) and np.all(np.isfinite(out["loss_his"])) and np.isfinite(out["rel_l2"])


def test_nonlinear_class_and_driver_adapt():
    """VPINNNonlinear(strong_form="elementwise") through the Allen-Cahn driver at a tiny setting: the class's indicators against the
    reference at the final parameters, one adaptation round, and the refusal of --adapt-every together with --validate-every"""
    import nonlinear_reference as nr
    from hp_vpinns_amd.drivers import nonlinear
    s = nonlinear.setup("allen-cahn", eps=0.3, n_elements=2, n_quad=6, n_test=3, width=8, depth=2, n_bound=8)
    with pytest.raises(ValueError):
        nonlinear.run(s, n_iter=4, adapt_every=2, validate_every=2, verbose=False)
    out = nonlinear.run(s, n_iter=20, adapt_every=10, max_elements=8, verbose=False)
    rows, m = out["adapt_rows"], out["model"]
    print("allen-cahn driver:", rows)
    assert len(rows) == 1 and rows[0][0] == 10 and 4 < rows[0][1] <= 8 and len(m.mesh) == rows[0][1]
    assert np.isfinite(rows[0][2]) and np.all(np.isfinite(out["loss_his"])) and np.isfinite(out["rel_l2"])
    p = nr.from_model(m)
    n = p["planes"].shape[1]
    p.update(kind="nl", dirs=np.zeros((0, 10, n)), c0=np.zeros(0), f=np.zeros(n))
    assert p["terms"] == ("u3",)
    ref = la.reference(p)
    ind, r = m.element_indicators(), m.strong_residual_at_quad()
    ec = _col_err(ind, ref["ind"])
    er = float(np.abs(r - ref["r"]).max() / np.abs(ref["r"]).max())
    print("allen-cahn class | columns %s | r %.2e" % (np.array2string(ec, precision=2), er))
    assert ec.max() < TOL and er < TOL
    with pytest.raises(NotImplementedError):
        nonlinear.run(s, n_iter=2, verbose=False)["model"].adapt()
