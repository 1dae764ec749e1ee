"""The nonlinear terms on the variable-coefficient class (hpv_set_nonlinear, k_project_nl, VPINNNonlinear) on the device against
tests/nonlinear_reference.py (CPU, fp64; tests/test_nonlinear_host.py proves it); the measured errors are in profiles/nonlinear_terms.md.

Every case: the conditions of the reference module on the reference alone, then loss_and_grad() -- loss triple, gradient per block --,
hpv_get_residuals (inactive entries exactly 0), a second call with the same bits, the kernel's name with its active terms and the pass
structure.  Bounds, exactly those of tests/test_gpu_linear.py: TOL = 1e-9 on the loss triple, the residuals and
the gradient per block, STEP_TOL = 1e-8 on parameters and loss after Adam steps, both imported from tests/test_gpu_generic_point.py."""
import numpy as np
import pytest

import generic_point as gp
import linear_reference as lr
import nonlinear_reference as nr
from cases import rel
from test_gpu_generic_point import STEP_TOL, TOL

pytestmark = pytest.mark.gpu

WORST = {}
_PROBLEMS = {}


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _problem(name):
    """the case's arrays and its reference (loss triple, gradient, R) at the initial parameters, computed once and left unchanged"""
    if name not in _PROBLEMS:
        p = nr.problem(nr.CASES[name])
        fig = nr.conditions(p)                          # the reference alone, first
        _PROBLEMS[name] = (p, nr.reference(p), fig)
    return _PROBLEMS[name]


class Dev:
    """the C-ABI on problem dict `p` (tests/test_gpu_linear.Dev's sequence, then hpv_set_nonlinear); nonlinear=False: a handle that
    never hears of the term; elements=False: stop before hpv_set_elements"""

    def __init__(self, p, nonlinear=True, backend=None, elements=True):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.init import n_params, pad_plan
        from hp_vpinns_amd.testfcn import tables_1d
        self.p, L = p, p["layers"]
        plan = pad_plan(L, 0)
        self.dev_layers, self.idx = plan if plan is not None else (L, None)
        self.n_dev = n_params(self.dev_layers, 0)
        self.h = h = _lib.Handle(_lib.PDE_LINEAR1D if p["dim"] == 1 else _lib.PDE_LINEAR2D, 1, _lib.ACT_SIN if p["act"] == "sin" else _lib.ACT_TANH,
                                 self.dev_layers, lr=1e-3, lossb_weight=p["lbw"], V=0.6, backend=_lib.BACKEND_AUTO if backend is None else backend)
        (xi, wx), yr = p["xr"], p["yr"]
        h.set_quadrature(xi, wx, *(yr if yr is not None else (None, None)))
        h.set_tables(tables_1d(p["ntx"], xi), None if yr is None else tables_1d(p["nty"], yr[0]))
        if not elements:
            return
        h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
        h.set_rhs(p["F"].reshape(-1))
        if p["nax"] is not None:
            if p["dim"] == 1:
                h.set_active_tests(p["nax"])
            else:
                h.set_active_tests_2d(p["nax"], p["nay"])
        h.set_operator(p["planes"])
        if nonlinear:
            h.set_nonlinear(p["nl"])
        if p["data"] is not None:
            h.set_data(*p["data"])
        if p["flux"] is not None:
            import flux_reference as fr
            h.set_flux_data(p["flux"]["X"], fr.coef(p["flux"]), p["flux"]["g"], fr.W_F)
        self.set_params(p["theta"])

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

    def residuals(self):
        p = self.p
        return self.h.residuals((p["ee"] - p["eb"]) * p["ntx"] * p["nty"]).reshape(-1, p["nty"], p["ntx"])

    def everything(self):
        l3, g = self.loss_and_grad()
        return l3, g, self.residuals()


def _rel3(a, b):
    """relative error per entry; an entry whose reference is exactly 0 (lossb without data) is compared absolutely: it must be 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def _kernel(p, terms=None):
    qx, qy = p["xr"][0].size, 1 if p["yr"] is None else p["yr"][0].size
    terms = p["terms"] if terms is None else terms
    shape = "%dx%d/%dx%d" % (qx, qy, p["ntx"], p["nty"])
    return "k_project_nl<%s;%s>" % (shape, ",".join(terms)) if terms else "k_project_lin<%s>" % shape


def _against_reference(tag, d, ref, terms=None):
    """loss_and_grad, the forward-only loss and the residuals of the live handle against (loss triple, gradient, R); the kernel's name"""
    p = d.p
    l3o, go, Ro = ref
    l3m, gm, Rm = d.everything()
    v, ps = d.h.kernel_variant(), d.h.pass_structure()
    lf = d.h.loss_and_grad(False)[0]
    e3, ef = _rel3(l3m, l3o), _rel3(lf, l3o)
    kb, eb = gp.worst_block(gm, go, p["layers"], 0)
    eR = float(np.linalg.norm(Rm - Ro) / np.linalg.norm(Ro))
    print("%s | %s | %s | loss3 %s | worst block %s %.2e (global %.2e) | forward-only %s | residuals %.2e" % (tag, v, ps, e3, kb, eb, rel(gm, go), ef, eR))
    WORST[tag] = (float(e3.max()), float(eb), float(ef.max()), eR)
    assert _kernel(p, terms) in v and ps == "separate", (tag, v, ps)
    assert d.h.lib.hpv_pass_structure(d.h._h) == 0
    assert e3.max() < TOL, (tag, v, "loss triple", l3m, l3o)
    assert eb < TOL, (tag, v, "gradient block", kb, eb)
    assert ef.max() < TOL, (tag, v, "forward-only pass", lf, l3o)
    assert eR < TOL, (tag, v, "residuals", eR)
    assert np.all(Rm[Ro == 0.0] == 0.0), (tag, "inactive residual entries are exactly 0")
    again = d.everything()
    assert all(np.array_equal(x, y) for x, y in zip((l3m, gm, Rm), again)), (tag, "a second call returns the same bits")


@pytest.mark.parametrize("name", list(nr.CASES))
def test_cases_against_the_reference(name):
    p, ref, fig = _problem(name)
    d = Dev(p)
    _against_reference(name, d, ref)
    v = d.h.kernel_variant()
    if name in nr.SMALL:                             # the layer kernels around the new projection
        wide = p["layers"][1] == 24
        assert ("k_fwd_wide<" in v and "H=24>" in v) if wide else "k_fwd_mfma<" in v, v
    print(name, fig)


def test_padding_points_receive_exact_zeros():
    """the 21 x 21 rule's last point per direction has zero weight: the loss is the 20 x 20 rule's, whatever N is there (the reference
    has no such point: its planes are cut to the 20 x 20 points)"""
    p, ref, _ = _problem("lds-21x21-padded")
    q = dict(p, xr=lr.rule(20), yr=lr.rule(20))
    ne = p["ee"] - p["eb"]
    q["planes"] = np.ascontiguousarray(p["planes"].reshape(5, ne, 21, 21)[:, :, :20, :20]).reshape(5, -1)
    q["nl"] = np.ascontiguousarray(p["nl"].reshape(5, ne, 21, 21)[:, :, :20, :20]).reshape(5, -1)
    l3o, go, _ = nr.reference(q)
    l3, g = Dev(p).loss_and_grad()
    assert _rel3(l3, l3o).max() < TOL and gp.block_rel(g, go, p["layers"]) < TOL


def test_generic_backend():
    from hp_vpinns_amd import _lib
    p, ref, _ = _problem("2d-h8-counts-flux")
    d = Dev(p, backend=_lib.BACKEND_GENERIC)
    _against_reference("generic backend", d, ref)
    assert "k_mlp_fwd_generic" in d.h.kernel_variant()


def test_adam_under_graphs_and_a_live_change_of_the_term():
    """three Adam steps against the reference's trajectory, new planes on the live handle, three more: one optimizer over both calls;
    a stale graph or a stale plane shows in the loss after the second call"""
    p, _, _ = _problem("2d-h8-counts-flux")
    d = Dev(p)
    d.h.step(3, False)
    assert d.h.graphs_in_use() and _kernel(p) in d.h.kernel_variant() and d.h.lib.hpv_pass_structure(d.h._h) == 0
    th3 = nr.adam_trajectory(p, 3)
    e3 = rel(d.params(), th3)
    nl2 = p["nl"].copy()
    nl2[2] = lr._signed(np.random.default_rng(78), nl2[2].shape)
    nl2[0] = 0.0                                     # (and the quadratic term leaves: another mask)
    d.h.set_nonlinear(nl2)
    l3 = d.h.step(3, True)
    assert d.h.graphs_in_use() and _kernel(p, ("u3", "exp", "adv")) in d.h.kernel_variant()
    th6 = nr.adam_trajectory(p, 3, nl=p["nl"], nl2=nl2)
    l3o = nr.reference(p, th6, nl=nl2)[0]
    stale = nr.reference(p, th6)[0]
    e = _rel3(l3, l3o)
    print("three Adam steps: parameters %.2e | three more after a live change: parameters %.2e, loss %s (against the old planes: %.2e)"
          % (e3, rel(d.params(), th6), e, abs(l3o[0] - stale[0]) / abs(l3o[0])))
    WORST["adam 3 / 3 + 3"] = (float(e3), float(rel(d.params(), th6)), float(e.max()))
    assert abs(l3o[0] - stale[0]) > 1e3 * STEP_TOL * abs(l3o[0])      # the reference alone tells the two terms apart
    assert e3 < STEP_TOL and e.max() < STEP_TOL and rel(d.params(), th6) < STEP_TOL and rel(th3, th6) > 0


@pytest.mark.parametrize("name", ["2d-h8-shard-data", "1d-sin"])
def test_removal_is_the_linear_handle_bit_for_bit(name):
    p, _, _ = _problem(name)
    fresh = Dev(p, nonlinear=False).everything()
    d = Dev(p)
    with_term = d.everything()
    assert not np.array_equal(with_term[0], fresh[0])
    for how in (None, np.zeros_like(p["nl"])):
        d.h.set_nonlinear(p["nl"])
        d.loss_and_grad()
        assert "k_project_nl" in d.h.kernel_variant()
        d.h.set_nonlinear(how)
        got = d.everything()
        v = d.h.kernel_variant()
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh)), (name, how is None)
        assert _kernel(p, ()) in v and "k_project_nl" not in v
    d.h.set_nonlinear(p["nl"])                       # and back: the term's own bits again
    assert all(np.array_equal(x, y) for x, y in zip(d.everything(), with_term))


def test_refusals_leave_the_handle_usable(monkeypatch):
    from hp_vpinns_amd import _lib
    p, ref, _ = _problem("2d-h8-shard-data")
    d = Dev(p)

    def refused(call, code=-1, message=None):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == code and (message is None or message in str(e.value)), (e.value.code, str(e.value))

    def usable():
        l3, g = d.loss_and_grad()
        assert _rel3(l3, ref[0]).max() < TOL and gp.block_rel(g, ref[1], p["layers"]) < TOL and _kernel(p) in d.h.kernel_variant()
    bad = p["nl"].copy()
    bad[2, 5] = np.nan
    inf = p["nl"].copy()
    inf[4, 0] = np.inf
    for call in (lambda: d.h.set_nonlinear(p["nl"][:, :-1]), lambda: d.h.set_nonlinear(p["nl"][:4]), lambda: d.h.set_nonlinear(bad),
                 lambda: d.h.set_nonlinear(inf)):
        refused(call)
        usable()
    # the strong form stays refused as for the linear class
    X = p["data"][0]
    for call in (lambda: d.h.set_collocation(X, np.zeros(X.shape[0])), lambda: d.h.residual_points(X), lambda: d.h.element_indicators()):
        refused(call)
        usable()
    # before hpv_set_elements: -3
    e = Dev(p, elements=False)
    refused(lambda: e.h.set_nonlinear(p["nl"]), -3)
    # new elements orphan the term: the pass answers -3 and names the call, until the planes are set again ...
    d.h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
    d.h.set_operator(p["planes"])
    refused(lambda: d.h.loss_and_grad(True), -3, "hpv_set_nonlinear has not been called again")
    refused(lambda: d.h.step(1, False), -3, "hpv_set_nonlinear has not been called again")
    d.h.set_nonlinear(p["nl"])
    _against_reference("after new elements", d, ref)
    # ... or removed
    d.h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
    d.h.set_operator(p["planes"])
    refused(lambda: d.h.loss_and_grad(True), -3, "hpv_set_nonlinear")
    d.h.set_nonlinear(None)
    _against_reference("removed after new elements", d, nr.reference(p, nl=np.zeros_like(p["nl"])), terms=())
    # a handle that never had the term is not held up by new elements
    f = Dev(p, nonlinear=False)
    f.h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
    f.h.set_operator(p["planes"])
    assert np.array_equal(f.loss_and_grad()[0], d.loss_and_grad()[0])
    # a Poisson handle has no such term
    import test_gpu_linear as TL
    m, _, _ = TL._existing("p2", monkeypatch)
    l0, g0 = m.loss_and_grad()
    refused(lambda: m.h.set_nonlinear(np.ones((5, 4))))
    refused(lambda: m.h.set_nonlinear(None))
    l1, g1 = m.loss_and_grad()
    assert np.array_equal(l0, l1) and np.array_equal(g0, g1)


def test_python_class_on_the_smallest_bratu_setting():
    """VPINNNonlinear through the driver's setup() at its smallest setting for a few dozen iterations: the loss at the final parameters is
    the reference's for the same problem, set_nonlinear(exponential=...) changes it to the reference's value for the new field"""
    from hp_vpinns_amd.drivers import nonlinear as drv
    kw = dict(drv.SMALLEST)
    s = drv.setup(kw.pop("problem"), **kw)
    out = drv.run(s, n_iter=40, LR=5e-3, verbose=False)
    m = out["model"]
    v = m.h.kernel_variant()
    assert "k_project_nl<8x1/4x1;exp>" in v and m.h.graphs_in_use(), v
    his = out["loss_his"]
    assert his.size == 40 and np.all(np.isfinite(his)) and his[-1] < his[0] and np.isfinite(out["rel_l2"])
    p = nr.from_model(m)
    assert p["terms"] == ("exp",)
    l3, g = m.loss_and_grad()
    l3o, go, _ = nr.reference(p, m.get_params())
    e1 = (float(_rel3(l3, l3o).max()), float(gp.block_rel(g, go, p["layers"])))
    assert max(e1) < TOL, e1
    m.set_nonlinear(exponential=lambda P: 2.0 + P[:, 0] ** 2)
    p2 = nr.from_model(m)
    l3n = m.loss()
    l3p = nr.reference(p2, m.get_params())[0]
    e2 = float(_rel3(l3n, l3p).max())
    print("Bratu, 40 steps: relative L2 error %.3e | loss, gradient block against the reference %s | after set_nonlinear %.2e" % (out["rel_l2"], e1, e2))
    WORST["class"] = e1 + (e2,)
    assert e2 < TOL and abs(l3p[0] - l3o[0]) > 1e-6 * abs(l3o[0])
    m.set_nonlinear(exponential=0.0)                  # the term leaves: the class runs VPINNLinear's kernel
    m.loss_and_grad()
    assert "k_project_lin" in m.h.kernel_variant()
    ch = m.evaluate(s["X_test"][:5])
    assert set(ch) == {"u", "u_x", "u_xx"} and all(np.all(np.isfinite(c)) for c in ch.values())
    m.set_validation(s["X_test"], s["u_test"])
    assert np.isfinite(m.validate()["rel_l2"])
    for what in (lambda: m.residual(s["X_test"]), m.adapt):
        with pytest.raises(NotImplementedError):
            what()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n| case | loss triple | gradient block | forward-only | residuals |")
    for k, e in WORST.items():
        print("| %s | %s |" % (k, " | ".join("%.1e" % x for x in e)))
