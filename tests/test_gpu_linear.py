"""The variable-coefficient linear problems (hpv_set_operator, k_project_lin, VPINNLinear) on the device against
tests/linear_reference.py (CPU, fp64; tests/test_linear_host.py proves it); the measured errors are in profiles/linear_operator.md.

Every case: the conditions of the reference module on the reference alone, then loss_and_grad() -- loss triple, gradient per block --,
the forward-only loss, hpv_get_residuals (inactive entries exactly 0), four Adam steps through hpv_step, the kernel's name and the
pass structure.  Bounds: TOL = 1e-9 on the loss triple and the gradient per block, STEP_TOL = 1e-8 on the
parameters after four Adam steps, both imported from tests/test_gpu_generic_point.py."""
import numpy as np
import pytest

import generic_point as gp
import linear_reference as lr
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
        p = lr.problem(lr.CASES[name])
        fig = lr.conditions(p)                          # the reference alone, first
        _PROBLEMS[name] = (p, lr.reference(p), fig)
    return _PROBLEMS[name]


class Dev:
    """the C-ABI on problem dict `p`: a narrow network is zero-padded onto its device width as the Python classes do (init.pad_plan)"""

    def __init__(self, p, operator=True, pde=None, var_form=1, scheme=0, extra=()):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.init import n_params, pad_plan
        from hp_vpinns_amd.testfcn import tables_1d
        self.p, L = p, p["layers"]
        plan = pad_plan(L, len(extra))
        self.dev_layers, self.idx = plan if plan is not None else (L, None)
        self.n_dev = n_params(self.dev_layers, len(extra))
        if pde is None:
            pde = _lib.PDE_LINEAR1D if p["dim"] == 1 else _lib.PDE_LINEAR2D
        self.h = h = _lib.Handle(pde, var_form, _lib.ACT_SIN if p["act"] == "sin" else _lib.ACT_TANH, self.dev_layers, lr=1e-3,
                                 lossb_weight=p["lbw"], V=0.6, scheme=scheme)
        if scheme:
            return
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
        if operator:
            h.set_operator(p["planes"])
        if p["data"] is not None:
            h.set_data(*p["data"])
        if p["flux"] is not None:
            import flux_reference as fr
            h.set_flux_data(p["flux"]["X"], fr.coef(p["flux"]), p["flux"]["g"], fr.W_F)
        self.set_params(np.concatenate([p["theta"], np.asarray(extra, dtype=np.float64)]))

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


def _rel3(a, b):
    """relative error per entry; an entry whose reference is exactly 0 (lossb without data) is compared absolutely: it must be 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def _against_reference(tag, d, ref, want_kernel=True):
    """loss_and_grad, the forward-only loss and the residuals of the live handle against (loss triple, gradient, R)"""
    p = d.p
    l3o, go, Ro = ref
    l3m, gm = d.loss_and_grad()
    v, ps = d.h.kernel_variant(), d.h.pass_structure()
    lf = d.h.loss_and_grad(False)[0]
    Rm = d.residuals()
    e3, ef = _rel3(l3m, l3o), _rel3(lf, l3o)
    kb, eb = gp.worst_block(gm, go, p["layers"], 0)
    eR = float(np.linalg.norm(Rm - Ro) / np.linalg.norm(Ro))
    print("%s | %s | %s | loss3 %s | worst block %s %.2e (global %.2e) | forward-only %s | residuals %.2e" % (tag, v, ps, e3, kb, eb, rel(gm, go), ef, eR))
    WORST[tag] = (float(e3.max()), float(eb), float(ef.max()), eR)
    if want_kernel:
        qx, qy = p["xr"][0].size, 1 if p["yr"] is None else p["yr"][0].size
        assert "k_project_lin<%dx%d/%dx%d>" % (qx, qy, p["ntx"], p["nty"]) in v and ps == "separate", (tag, v, ps)
        assert d.h.lib.hpv_pass_structure(d.h._h) == 0
    assert e3.max() < TOL, (tag, v, "loss triple", l3m, l3o)
    assert eb < TOL, (tag, v, "gradient block", kb, eb)
    assert ef.max() < TOL, (tag, v, "forward-only pass", lf, l3o)
    assert eR < TOL, (tag, v, "residuals", eR)
    assert np.all(Rm[Ro == 0.0] == 0.0), (tag, "inactive residual entries are exactly 0")


@pytest.mark.parametrize("name", lr.SMALL)
def test_small_shapes_against_the_reference(name):
    p, ref, fig = _problem(name)
    d = Dev(p)
    _against_reference(name, d, ref)
    v = d.h.kernel_variant()
    wide = p["layers"][1] == 24
    assert ("k_fwd_wide<" in v and "H=24>" in v) if wide else "k_fwd_mfma<" in v, v
    d.set_params(p["theta"])
    d.h.step(4, False)
    assert d.h.graphs_in_use() and "k_project_lin" in d.h.kernel_variant() and d.h.lib.hpv_pass_structure(d.h._h) == 0
    pm, po = d.params(), lr.adam_trajectory(p, 4)
    print("%s | four Adam steps: parameters %.2e | %s" % (name, rel(pm, po), fig))
    WORST[name + " adam"] = (float(rel(pm, po)),)
    assert rel(pm, po) < STEP_TOL, (name, "parameters after four Adam steps", rel(pm, po))


@pytest.mark.parametrize("name", ["lds-20x20", "lds-21x21-padded"])
def test_lds_edge(name):
    """one element of 20 x 20 points and 10 x 10 functions, and a 21 x 21 rule whose last point per direction has zero weight"""
    p, ref, _ = _problem(name)
    _against_reference(name, Dev(p), ref)


def _existing(prob, monkeypatch):
    import test_gpu_generic_point as T
    c = lr.SPECIAL[prob]
    monkeypatch.setenv("HPV_FUSE", "n")
    _, m, a, th, _ = T._pair(c, monkeypatch)
    s, _ = T._setup(c)
    return m, lr.from_setup(prob, s, c["L"], th, c["lbw"]), th


@pytest.mark.parametrize("prob", ["p2", "adv", "p1"])
def test_agreement_with_the_existing_paths_on_the_device(prob, monkeypatch):
    """k = 1 against a Poisson-2D var_form 1 handle, kx = -eps, bx = V, by = 1 against an AdvDiff var_form 1 handle (network blocks
    only), 1-D k = -1 against a Poisson-1D var_form 2 handle, each on the same parameters"""
    m, p, th = _existing(prob, monkeypatch)
    l3e, ge = m.loss_and_grad()
    d = Dev(p)
    l3, g = d.loss_and_grad()
    assert "k_project_lin" in d.h.kernel_variant() and "k_project_lin" not in m.h.kernel_variant()
    n = g.size
    which = [0, 2] if prob == "adv" else [0, 1, 2]      # (AdvDiff reports the weighted lossb)
    e3 = _rel3(np.asarray(l3)[which], np.asarray(l3e)[which])
    kb, eb = gp.worst_block(g, np.asarray(ge)[:n], p["layers"], 0)
    print("%s: %s against %s | loss %s | worst block %s %.2e" % (prob, d.h.kernel_variant(), m.h.kernel_variant(), e3, kb, eb))
    WORST["special " + prob] = (float(e3.max()), float(eb))
    assert e3.max() < TOL and eb < TOL


def test_live_change_of_the_operator_between_two_steps():
    """a new sigma between two hpv_step calls: a stale graph or a stale plane shows in the loss after the second call"""
    p, _, _ = _problem("2d-h8-flux")
    d = Dev(p)
    d.h.step(3, False)
    assert d.h.graphs_in_use()
    planes = p["planes"].copy()
    planes[4] = lr._signed(np.random.default_rng(77), planes[4].shape)
    d.h.set_operator(planes)
    l3 = d.h.step(3, True)
    assert d.h.graphs_in_use()
    th3 = lr.adam_trajectory(p, 3)
    th6 = _continue(p, 3, planes)                    # (hpv_set_operator keeps the optimizer: one rule over both calls)
    l3o = lr.reference(p, th6, planes)[0]
    stale = lr.reference(p, th6, p["planes"])[0]
    e = _rel3(l3, l3o)
    print("loss after a live change of sigma: %s (against the old plane: %.2e)" % (e, abs(l3o[0] - stale[0]) / abs(l3o[0])))
    assert abs(l3o[0] - stale[0]) > 1e3 * STEP_TOL * abs(l3o[0])      # the reference alone tells the two fields apart
    assert e.max() < STEP_TOL and rel(d.params(), th6) < STEP_TOL and rel(th3, th6) > 0


def _continue(p, steps, planes2, lr_=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """`steps` TF1-Adam updates under p's planes, then `steps` more under planes2, one optimizer throughout"""
    th = np.array(p["theta"], dtype=np.float64)
    m, v, b1p, b2p = np.zeros_like(th), np.zeros_like(th), b1, b2
    for k in range(2 * steps):
        g = lr.reference(p, th, p["planes"] if k < steps else planes2)[1]
        lr_t = lr_ * np.sqrt(1.0 - b2p) / (1.0 - b1p)
        m, v = b1 * m + (1.0 - b1) * g, b2 * v + (1.0 - b2) * g * g
        th = th - lr_t * m / (np.sqrt(v) + eps)
        b1p, b2p = b1p * b1, b2p * b2
    return th


@pytest.mark.parametrize("name", ["2d-h8-flux", "1d-sin"])
def test_two_passes_return_the_same_bytes(name):
    p, _, _ = _problem(name)
    d = Dev(p)
    r = []
    for _ in range(2):
        l3, g = d.loss_and_grad()
        r.append((l3, g, d.residuals()))
    assert all(np.array_equal(x, y) for x, y in zip(*r)), name


def test_refusals_leave_the_handle_usable(monkeypatch):
    from hp_vpinns_amd import _lib
    p, ref, _ = _problem("2d-h8-shard-data")
    for kw in (dict(scheme=_lib.SCHEME_PINN), dict(var_form=0), dict(var_form=2)):
        with pytest.raises(_lib.HpvError):
            Dev(p, **kw)
    # hpv_step before hpv_set_operator: -3
    d = Dev(p, operator=False)
    with pytest.raises(_lib.HpvError) as ei:
        d.h.step(1, False)
    assert ei.value.code == -3 and "hpv_set_operator" in str(ei.value)
    d.h.set_operator(p["planes"])
    _against_reference("after -3", d, ref)

    def refused(call, code=-1):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == code, (e.value.code, str(e.value))
        l3, g = d.loss_and_grad()
        assert _rel3(l3, ref[0]).max() < TOL and gp.block_rel(g, ref[1], p["layers"]) < TOL
    bad = p["planes"].copy()
    bad[2, 5] = np.nan
    refused(lambda: d.h.set_operator(p["planes"][:, :-1]))
    refused(lambda: d.h.set_operator(bad))
    refused(lambda: d.h.set_operator(None))
    X = p["data"][0]
    refused(lambda: d.h.set_collocation(X, np.zeros(X.shape[0])))
    refused(lambda: d.h.residual_points(X))
    refused(lambda: d.h.element_indicators())
    # hpv_set_elements invalidates the planes
    d.h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
    refused_after = pytest.raises(_lib.HpvError)
    with refused_after as e:
        d.h.loss_and_grad(True)
    assert e.value.code == -3
    d.h.set_operator(p["planes"])
    _against_reference("after new elements", d, ref)
    # a Poisson handle has no operator
    m, _, _ = _existing("p2", monkeypatch)
    l0, g0 = m.loss_and_grad()
    with pytest.raises(_lib.HpvError) as e:
        m.h.set_operator(np.ones((5, 4)))
    assert e.value.code == -1
    l1, g1 = m.loss_and_grad()
    assert np.array_equal(l0, l1) and np.array_equal(g0, g1)
    # the advice for the new values: leave the rule alone
    assert _lib.rule_advice(0, _lib.PDE_LINEAR2D, 1, 2, 20, 11, 5, 5, 16) == (11, 5)
    assert _lib.rule_advice(0, _lib.PDE_LINEAR1D, 1, 2, 20, 33, 7, 1, 4) == (33, 7)


def test_python_class_and_boundary_layer_driver_converge():
    """One run of the 1-D boundary-layer driver at its smallest setting (the class surface: callables, set_operator, checkpoints of the
    base class) against the CPU reference's own Adam trajectory on the same problem for the same number of steps.

    Bound: the reference trajectory's relative L2 error times 2 -- the two trajectories separate within STEP_TOL per step."""
    from hp_vpinns_amd.drivers import linear
    out = linear.run_boundary_layer(**linear.SMALLEST, verbose=False)
    m = out["model"]
    assert "k_project_lin" in m.h.kernel_variant() and m.h.graphs_in_use()
    p = lr.from_model(m, m._init_params)                # the same problem from the same initial parameters
    th = lr.adam_trajectory(p, linear.SMALLEST["n_iter"], lr=m.LR)
    import validation_reference as vr
    X, u = out["X_test"], out["u_test"]
    ur = vr.bare_oracle(p["prob"], p["layers"], th)._predict(X)
    e_ref = float(np.linalg.norm(ur.reshape(-1) - u.reshape(-1)) / np.linalg.norm(u))
    print("boundary layer, %d steps: relative L2 error %.4e on the device, %.4e on the CPU reference's trajectory (parameters %.2e)"
          % (linear.SMALLEST["n_iter"], out["rel_l2"], e_ref, rel(m.get_params(), th)))
    WORST["driver"] = (out["rel_l2"], e_ref)
    assert out["rel_l2"] < 2 * e_ref
    # set_operator on the live model: the loss is the reference's for the new field
    m.set_operator(sigma=lambda P: 1.0 + P[:, 0] ** 2)
    p2 = lr.from_model(m)
    l3 = m.loss()
    l3o = lr.reference(p2, m.get_params())[0]
    assert _rel3(l3, l3o).max() < TOL and abs(l3o[0] - lr.reference(p, m.get_params())[0][0]) > 1e-6 * abs(l3o[0])
    for what in (m.adapt, lambda: m.train_adaptive(10, 5)):
        with pytest.raises(NotImplementedError):
            what()


def test_l_shape_driver_runs():
    from hp_vpinns_amd.drivers import linear
    out = linear.run_l_shape(n_iter=40, n_quad=8, n_test=4, layers=[2, 20, 20, 1], verbose=False)
    m, his = out["model"], out["loss_his"]
    assert "k_project_lin" in m.h.kernel_variant()
    assert np.all(np.isfinite(his)) and his[-1] < his[0] and np.isfinite(out["rel_l2"])
    p = lr.from_model(m)
    l3, g = m.loss_and_grad()
    l3o, go, _ = lr.reference(p, m.get_params())
    assert _rel3(l3, l3o).max() < TOL and gp.block_rel(g, go, p["layers"]) < TOL


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n| case | loss triple | gradient block | forward-only | residuals |")
    for k, e in WORST.items():
        print("| %s | %s |" % (k, " | ".join("%.1e" % x for x in e)))
