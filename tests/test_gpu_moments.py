"""Integral constraints on the device (hpv_set_moments, hpv_read_moments; k_moment_part, k_moment_close, k_moment_adj;
VPINNLinear(constraints=)) against tests/moment_reference.py (CPU, fp64; tests/test_moment_host.py proves it, and asserts for these
exact inputs that the constraint part is 10 % .. 90 % of the gradient norm).  Bounds: TOL = 1e-9 on the loss triple, the moments, the
penalties and the gradient per block, STEP_TOL = 1e-8 after 20 Adam steps, both imported from tests/test_gpu_generic_point.py as
tests/test_gpu_quasilinear.py does.  The measured errors are in profiles/integral_constraints.md.

The C-ABI has no call that returns GBAR, so "the merged data points' entries are untouched" and "a padding point receives exactly 0" are
asserted where they can be: the gradient of the case with merged data points and non-zero weights ("17x17-data-K8") is the reference's,
which an adjoint that reached past Nq would spoil, and the padded rule's loss and gradient are those of the rule without its padding
points."""
import numpy as np
import pytest

import generic_point as gp
import moment_reference as mo
from cases import rel
from test_gpu_generic_point import STEP_TOL, TOL

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _mesh(p):
    from hp_vpinns_amd.adapt import MappedMesh
    return MappedMesh.from_quads(mo.QUADS, p["nax"], p["nay"])


class Dev:
    """the C-ABI on a moment_reference problem: boxes and 1-D elements take the physical planes, mapped elements the product's points and
    its fold (VPINNLinear._fold); the measure planes come from the product's own VPINNLinear._fold_measure.  moments=False: a handle
    that never hears of hpv_set_moments"""

    def __init__(self, p, moments=True):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.init import n_params, pad_plan
        from hp_vpinns_amd.testfcn import tables_1d
        from hp_vpinns_amd.vpinn import VPINNLinear
        self.p, dim = p, p["dim"]
        self.nc = nc = len(p["dirs"])
        plan = pad_plan(p["layers"], nc)
        self.dev_layers, self.idx = plan if plan is not None else (p["layers"], None)
        self.n_dev = n_params(self.dev_layers, nc)
        self.h = h = _lib.Handle(_lib.PDE_LINEAR1D if dim == 1 else _lib.PDE_LINEAR2D, 1, _lib.ACT_SIN if dim == 1 else _lib.ACT_TANH,
                                 self.dev_layers, lr=1e-3, lossb_weight=p["lbw"], **(dict(n_coef=nc) if nc else {}))
        (xi, wx), (yi, wy) = p["xr"], p["yr"]
        ne, nq = p["ee"] - p["eb"], p["X"].shape[1]
        n = ne * nq
        if dim == 1:
            h.set_quadrature(xi, wx, None, None)
            h.set_tables(tables_1d(p["ntx"], xi), None)
        else:
            h.set_quadrature(xi, wx, yi, wy)
            h.set_tables(tables_1d(p["ntx"], xi), tables_1d(p["nty"], yi))
        self.A = None
        self.tensor = p["kind"] == "quads"
        self.hand_elements()
        c = p["coefs"]
        z = lambda k, sh, src=c: src[k].reshape((n,) + sh) if k in src else np.zeros((n,) + sh)
        K = c["K"].reshape(n, dim, dim)
        Kd = K if self.tensor else np.stack([K[:, a, a] for a in range(dim)], 1)
        self.op = VPINNLinear._fold(self.A, self.tensor, Kd, (z("b", (dim,)), z("s", ())))
        self.nl = VPINNLinear._fold(self.A, False, None, (z("a2", ()), z("a3", ()), z("ae", ()), z("g", (dim,))))
        self.has_nl = any(k in c for k in ("a2", "a3", "ae", "g"))
        self.dirs = None
        if nc:                                            # (boxes, a diagonal kappa: K + M = 5 + 5 rows per direction)
            self.dirs = np.stack([np.concatenate([VPINNLinear._fold(None, False, np.zeros((n, dim)), (z("b", (dim,), d), z("s", (), d))),
                                                  np.zeros((5, n))], 0) for d in p["dirs"]], 0)
        w = wx if dim == 1 else np.outer(wy, wx).reshape(-1)
        if self.A is not None:
            jac = self.A[:, 0, 0] * self.A[:, 1, 1] - self.A[:, 0, 1] * self.A[:, 1, 0]
        else:
            b = p["boxes"][p["eb"]:p["ee"]]
            jac = np.repeat(np.prod([(b[:, 2 * a + 1] - b[:, 2 * a]) / 2 for a in range(dim)], axis=0), nq)
        self.m = VPINNLinear._fold_measure(np.stack([t["rho"].reshape(-1) for t in p["mom"]], 0), w, jac)
        self.power = [t["power"] for t in p["mom"]]
        self.target = [t["target"] for t in p["mom"]]
        self.weight = [t["weight"] for t in p["mom"]]
        self.K = len(self.power)
        self.hand_planes(moments)
        h.set_rhs(p["F"].reshape(-1))
        if p["nax"] is not None:
            if dim == 1:
                h.set_active_tests(p["nax"])
            else:
                h.set_active_tests_2d(p["nax"], p["nay"])
        self.hand_norm()
        if p["ansatz"] is not None:
            Xq = p["X"].reshape(-1, 2)
            h.set_ansatz(0, np.concatenate([np.asarray(p["ansatz"]["g"](Xq)).T, np.asarray(p["ansatz"]["d"](Xq)).T], 0))
        if p["data"] is not None:
            h.set_data(*p["data"])
            if p["ansatz"] is not None:
                Xd = p["data"][0]
                h.set_ansatz(1, np.concatenate([np.asarray(p["ansatz"]["g"](Xd)).T, np.asarray(p["ansatz"]["d"](Xd)).T], 0))
        self.set_params(mo.full0(p))

    def hand_elements(self):
        h, p = self.h, self.p
        if p["boxes"] is not None:
            h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
            return
        mesh = _mesh(p)
        xi, yi = p["xr"][0], p["yr"][0]
        h.set_element_points(mesh.quad_points(xi, yi).reshape(len(mesh), -1, 2).transpose(0, 2, 1), p["eb"], p["ee"])
        self.A = mesh.geometry(xi, yi, p["eb"], p["ee"])[1]

    def hand_planes(self, moments=True):
        h = self.h
        (h.set_operator_tensor if self.tensor else h.set_operator)(self.op)
        if self.has_nl:
            h.set_nonlinear(self.nl)
        if self.nc:
            h.set_trainable(self.dirs)
        if moments:
            self.set_moments()

    def hand_norm(self):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.quadrature import gram_factors, gram_rule, gram_stacks
        import mapped_reference as mr
        p, norm = self.p, self.p["norm"]
        if norm is None:
            return
        if norm[0] == "table":
            sx, sy = gram_stacks(p["ntx"]), gram_stacks(p["nty"])
            self.h.set_residual_norm(_lib.NORM_DUAL, norm[1], sx[0], sx[1], sy[0], sy[1])
        else:
            x = gram_rule(p["ntx"], p["nty"])[0]
            Ag = mr.geom_quads(mo.QUADS, x, x)[1]
            self.h.set_residual_gram(gram_factors(2, p["ntx"], p["nty"], p["nax"], p["nay"], Ag, None, norm[1]))

    def set_moments(self, weight=None):
        self.h.set_moments(self.power, self.m, self.target, self.weight if weight is None else weight)

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
        return np.asarray(l3), (g if self.idx is None else g[self.idx])

    def everything(self):
        l3, g = self.loss_and_grad()
        I, pen = self.h.read_moments(self.K) if self.h_has_terms() else (np.zeros(0), np.zeros(0))
        return l3, g, I, pen

    def h_has_terms(self):
        return ";mom=" in self.h.kernel_variant()


def _rel3(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the kernels against the reference: loss, gradient, moments, a forward-only pass, 20 Adam steps -------------------------------------------
@pytest.mark.parametrize("name", list(mo.CASES))
def test_kernels_against_the_reference(name):
    p, t = mo.case(name)
    d = Dev(p)
    l3, g, I, pen = d.everything()
    v = d.h.kernel_variant()
    lf = np.asarray(d.h.loss_and_grad(False)[0])
    If, penf = d.h.read_moments(d.K)
    e3, ef = _rel3(l3, t["triple"]), _rel3(lf, t["triple"])
    kb, eb = gp.worst_block(g[:p["theta"].size], t["grad"][:p["theta"].size], p["layers"], 0)
    ec = float(_rel3(g[p["theta"].size:], t["grad"][p["theta"].size:]).max()) if d.nc else 0.0
    eI, ep = _rel3(I, t["I"]), _rel3(pen, t["pen"])
    print("%s | %s | loss3 %s | worst block %s %.2e (global %.2e, coefficients %.2e) | forward-only %s | I %.2e pen %.2e" % (
        name, v, e3, kb, eb, rel(g, t["grad"]), ec, ef, eI.max(), ep.max()))
    assert ";mom=%d" % d.K in v and d.h.lib.hpv_pass_structure(d.h._h) == 0, v
    assert e3.max() < TOL and ef.max() < TOL, (name, l3, lf, t["triple"])
    assert eb < TOL and ec < TOL, (name, kb, eb, ec)
    assert eI.max() < TOL and ep.max() < TOL, (name, I, t["I"], pen, t["pen"])
    assert np.array_equal(I, If) and np.array_equal(pen, penf), "the forward-only pass forms the same moments, bit for bit"
    assert _same((l3, g, I, pen), d.everything()), "a second call returns the same bits"
    # 20 Adam steps (under graphs), against the reference's trajectory
    d.h.step(20, False)
    th = mo.adam_trajectory(p, 20)
    es = rel(d.params(), th)
    print("%s | 20 steps: parameters %.2e" % (name, es))
    WORST[name] = (float(e3.max()), float(eb), ec, float(eI.max()), float(ep.max()), float(es))
    assert d.h.graphs_in_use() and es < STEP_TOL, (name, es)


def test_graph_and_eager_iterations_agree_bitwise(monkeypatch):
    p, _ = mo.case("5x5-sigma")
    a = Dev(p)
    a.h.step(20, False)
    assert a.h.graphs_in_use()
    monkeypatch.setenv("HPV_NO_GRAPH", "1")
    b = Dev(p)
    b.h.step(20, False)
    assert not b.h.graphs_in_use()
    assert np.array_equal(a.params(), b.params())
    assert _same(a.everything(), b.everything())


@pytest.mark.parametrize("name", ["17x17-data-K8", "5x5-sigma", "1d-7", "6x5-quads-dual-dense"])
def test_set_then_remove_is_never_set_bit_for_bit(name):
    p, _ = mo.case(name)
    f = Dev(p, moments=False)
    fresh = f.loss_and_grad()
    vf = f.h.kernel_variant()
    f.h.step(20, False)
    fresh_th = f.params()
    d = Dev(p)
    with_terms = d.everything()
    assert ";mom=%d" % d.K in d.h.kernel_variant() and not np.array_equal(with_terms[0], fresh[0])
    # weight 0: the penalties are 0 and the adjoint adds 0 * m, so loss and gradient are those of a handle without terms, bit for bit
    # (this says nothing about WHERE the adjoint writes: the gradient against the reference with non-zero weights does)
    d.set_moments(weight=[0.0] * d.K)
    l3, g, I, pen = d.everything()
    assert np.all(pen == 0.0) and np.array_equal(I, with_terms[2]) and np.array_equal(g, fresh[1]) and np.array_equal(l3, fresh[0])
    d.h.set_moments(None, None, None, None)
    got = d.loss_and_grad()
    assert _same(got, fresh) and d.h.kernel_variant() == vf and ";mom" not in vf
    d.h.step(20, False)
    assert np.array_equal(d.params(), fresh_th)
    d.set_params(mo.full0(p))
    d.set_moments()                                       # and back: the terms' own bits again
    assert _same(d.everything(), with_terms)


def test_padding_points_contribute_nothing():
    from test_moment_host import _cut
    p, _ = mo.case("6x5-padded")
    c = mo.terms(_cut(p))
    l3, g, I, pen = Dev(p).everything()
    assert _rel3(l3, c["triple"]).max() < TOL and gp.block_rel(g, c["grad"], p["layers"]) < TOL and _rel3(I, c["I"]).max() < TOL


def test_refusals_leave_the_handle_usable():
    from hp_vpinns_amd import _lib
    p, t = mo.case("6x5-dual-table")
    d = Dev(p)

    def refused(call, code, message):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == code and message in str(e.value), (e.value.code, str(e.value))

    def usable():
        l3, g = d.loss_and_grad()
        assert _rel3(l3, t["triple"]).max() < TOL and gp.block_rel(g, t["grad"], p["layers"]) < TOL and ";mom=2" in d.h.kernel_variant()
    bad_m = d.m.copy()
    bad_m[1, 5] = np.nan
    for call, msg in ((lambda: d.h.set_moments([1, 3], d.m, d.target, d.weight), "term 1 has power 3"),
                      (lambda: d.h.set_moments([0, 1], d.m, d.target, d.weight), "term 0 has power 0"),
                      (lambda: d.h.set_moments([1] * 9, np.tile(d.m[:1], (9, 1)), [0.0] * 9, [1.0] * 9), "n_terms = 9 not in 0..8"),
                      (lambda: d.h.set_moments(d.power, d.m, d.target, [1.0, -0.5]), "negative weight"),
                      (lambda: d.h.set_moments(d.power, d.m, d.target, [1.0, np.inf]), "non-finite weight"),
                      (lambda: d.h.set_moments(d.power, d.m, [np.nan, 0.0], d.weight), "non-finite target"),
                      (lambda: d.h.set_moments(d.power, bad_m, d.target, d.weight), "term 1 holds a non-finite value at point 5"),
                      (lambda: d.h.set_moments(d.power, d.m[:, :-1], d.target, d.weight), "expected 2 planes")):
        refused(call, -1, msg)
        usable()
    refused(lambda: d.h.read_moments(3), -1, "the handle has 2 terms")
    # new elements orphan the planes: the pass answers -3 and names the call, until they are set again or removed
    d.hand_elements()
    d.hand_planes(moments=False)
    d.hand_norm()
    refused(lambda: d.h.loss_and_grad(True), -3, "hpv_set_moments has not been called again")
    refused(lambda: d.h.loss_and_grad(False), -3, "hpv_set_moments has not been called again")
    refused(lambda: d.h.step(1, False), -3, "hpv_set_moments has not been called again")
    d.set_moments()
    usable()
    d.hand_elements()
    d.hand_planes(moments=False)
    d.hand_norm()
    d.h.set_moments(None, None, None, None)
    fresh = Dev(p, moments=False)
    assert np.array_equal(d.loss_and_grad()[0], fresh.loss_and_grad()[0]) and ";mom" not in d.h.kernel_variant()
    d.set_moments()
    usable()
    # before hpv_set_elements; the strong-form scheme; a handle of another class
    e = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, mo.L2)
    refused(lambda: e.set_moments(d.power, d.m, d.target, d.weight), -3, "hpv_set_elements")
    # (no linear handle exists under the strong-form scheme, so none can be given terms: hpv_create refuses it)
    refused(lambda: _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, mo.L2, scheme=_lib.SCHEME_PINN), -1, "variational scheme only")
    o = _lib.Handle(_lib.PDE_POISSON2D, 1, _lib.ACT_TANH, [2, 20, 20, 20, 1])
    refused(lambda: o.set_moments(d.power, d.m, d.target, d.weight), -3, "linear problems")
    refused(lambda: o.set_moments(None, None, None, None), -3, "linear problems")
    # an exchange and the terms exclude each other, both ways round (no peer is needed for the refusal)
    import ctypes as C
    buf = (C.c_char * 128)()
    rc = d.h.lib.hpv_rccl_connect(d.h._h, 1, 0, buf)
    assert rc == -3 and b"no collective before the adjoint" in d.h.lib.hpv_last_error(d.h._h)
    rc = d.h.lib.hpv_p2p_export(d.h._h, 1, 0, buf)
    assert rc == -3 and b"hpv_set_moments" in d.h.lib.hpv_last_error(d.h._h)
    usable()


def test_an_exchange_refuses_new_terms_and_lets_them_be_removed():
    """the other way round: the exchange first (a one-rank world, as tests/test_gpu_generic_point.py connects one), then
    hpv_set_moments -- refused with -3 for n_terms > 0, accepted for n_terms == 0, and the handle passes on as one without terms"""
    from hp_vpinns_amd import _lib
    if int(_lib.load().hpv_rccl_available()) != 1:
        pytest.skip("librccl cannot be loaded: no in-library exchange to connect")
    p, _ = mo.case("6x5-dual-table")
    fresh = Dev(p, moments=False).loss_and_grad()
    d = Dev(p, moments=False)
    d.h.rccl_connect(1, 0, d.h.rccl_unique_id())
    assert d.h.exchange_in_use() == "rccl"
    with pytest.raises(_lib.HpvError) as e:
        d.set_moments()
    assert e.value.code == -3 and "exchange connected" in str(e.value) and "no collective before the adjoint" in str(e.value)
    d.h.set_moments(None, None, None, None)              # removal is harmless: accepted, nothing changes
    d.hand_elements()                                     # ... also after new elements (what set_mesh does on every rank)
    d.hand_planes(moments=False)
    d.hand_norm()
    d.h.set_moments(None, None, None, None)
    got = d.loss_and_grad()
    assert _same(got, fresh) and ";mom" not in d.h.kernel_variant()
    d.h.step(3, False)
    d.h.rccl_disconnect()
    d.set_params(mo.full0(p))
    d.set_moments()                                       # disconnected: the terms are accepted again
    assert ";mom=2" in (d.loss_and_grad(), d.h.kernel_variant())[1]


# ---- the Python class -------------------------------------------------------------------------------------------------------------------------
def _model(constraints, **kw):
    from hp_vpinns_amd.vpinn import VPINNLinear
    gx, gy = np.array([-1.0, 0.3, 1.0]), np.array([-1.0, -0.2, 1.0])
    args = dict(grid_x=gx, grid_y=gy, n_quad=(6, 5), n_test=(3, 2), kappa=lambda P: np.stack([1.0 + 0.3 * P[:, 0], 1.5 - 0.2 * P[:, 1]], 1),
                beta=np.array([0.3, -0.2]), sigma=0.4, f=lambda P: np.sin(P[:, 0]) + P[:, 1], constraints=constraints,
                X_u_train=np.array([[-1.0, 0.0], [1.0, 0.5], [0.2, -1.0]]), u_train=np.array([0.1, -0.2, 0.3]), lossb_weight=3.0,
                init_params=gp.generic_theta(mo.L2, 9890))
    args.update(kw)
    return VPINNLinear(mo.L2, **args)


CONS = [dict(name="mean", kind="mean", target=0.3, weight=2.0), dict(name="norm", kind="l2", target=1.0, weight=0.5),
        dict(name="defl", kind="moment", density=lambda P: np.sin(2.0 * P[:, 0]) * P[:, 1], power=1, target=0.0, weight=4.0)]


def test_class_constraints_live_change_mesh_change_and_checkpoint(tmp_path):
    m = _model(CONS)
    l3, g = m.loss_and_grad()
    c = m.constraints()
    assert set(c) == {"mean", "norm", "defl"} and ";mom=3" in m.h.kernel_variant()
    # the integrals, restated: weight x half widths x density x u^p at the model's own quadrature points
    P = m._geometry(m._mesh, 0, 4)[0]
    u = m.predict(P).reshape(-1)
    w = np.tile(np.outer(m._rule[1][1], m._rule[0][1]).reshape(-1), 4)
    b = m._mesh.boxes
    J = np.repeat((b[:, 1] - b[:, 0]) / 2 * (b[:, 3] - b[:, 2]) / 2, 30)
    want = [np.sum(w * J * u), np.sum(w * J * u * u), np.sum(w * J * np.sin(2.0 * P[:, 0]) * P[:, 1] * u)]
    for (name, tgt, wt), I in zip((("mean", 0.3, 2.0), ("norm", 1.0, 0.5), ("defl", 0.0, 4.0)), want):
        assert abs(c[name][0] - I) < TOL * max(1.0, abs(I)) and abs(c[name][1] - wt * (I - tgt) ** 2) < TOL * max(1.0, c[name][1])
    plain = _model(None)
    l3p, gp_ = plain.loss_and_grad()
    pen = sum(v[1] for v in c.values())
    assert abs((l3[2] - l3p[2]) - pen) < TOL * max(1.0, pen) and ";mom" not in plain.h.kernel_variant()
    # a live change keeps parameters and optimizer state; removal is the plain model bit for bit
    m.train(5)
    st = m.h.get_state().copy()
    m.set_constraints(CONS[:1])
    assert np.array_equal(m.h.get_state(), st) and ";mom=1" in (m.loss_and_grad(), m.h.kernel_variant())[1]
    m.set_constraints(None)
    plain.set_params(m.get_params())
    assert _same(m.loss_and_grad(), plain.loss_and_grad()) and m.constraints() == {}
    # checkpoints carry the terms with the unfolded density values
    m.set_constraints(CONS)
    ref = m.loss_and_grad()
    m.save_checkpoint(tmp_path / "c")
    n = _model(None)
    n.load_checkpoint(tmp_path / "c")
    assert _same(n.loss_and_grad(), ref) and n.constraints() == m.constraints()
    # a mesh change re-evaluates callables and refuses arrays: the restored "moment" entry is one, the restored "mean" / "l2" are not
    from hp_vpinns_amd.adapt import ElementMesh
    assert [k.get("kind") for k in n._constraints] == ["mean", "l2", "moment"] and isinstance(n._constraints[2]["density"], np.ndarray)
    with pytest.raises(ValueError, match="hand it over again"):
        n.set_mesh(ElementMesh.from_grid(np.array([-1.0, 0.0, 1.0]), np.array([-1.0, 1.0])))
    n.set_constraints(n._constraints[:2])
    n.set_mesh(ElementMesh(ElementMesh.from_grid(np.array([-1.0, 0.0, 1.0]), np.array([-1.0, 1.0])).boxes, 3, 2))
    assert ";mom=2" in (n.loss_and_grad(), n.h.kernel_variant())[1]
    th = m.get_params().copy()
    m.set_mesh(ElementMesh(ElementMesh.from_grid(np.array([-1.0, 0.0, 0.5, 1.0]), np.array([-1.0, 1.0])).boxes, 3, 2))
    c2 = m.constraints() if m.loss_and_grad() else None
    assert np.array_equal(m.get_params(), th) and ";mom=3" in m.h.kernel_variant()
    assert abs(c2["mean"][0] - c["mean"][0]) < 0.5 and np.isfinite(c2["defl"][0])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n| case | loss triple | gradient block | coefficients | I | pen | 20 steps |")
    for k, e in WORST.items():
        print("| %s | %s |" % (k, " | ".join("%.1e" % x for x in e)))


def test_class_without_constraints_under_an_exchange_and_the_several_gpu_refusal(monkeypatch):
    """a model that never had constraints changes its mesh with the in-library exchange connected (every rank of a multi-GPU run does),
    and constraints on a model of a larger world are a ValueError that gives the reason"""
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.adapt import ElementMesh
    if int(_lib.load().hpv_rccl_available()) != 1:
        pytest.skip("librccl cannot be loaded: no in-library exchange to connect")
    new = ElementMesh(ElementMesh.from_grid(np.array([-1.0, 0.0, 0.5, 1.0]), np.array([-1.0, 1.0])).boxes, 3, 2)
    ref = _model(None)
    ref.set_mesh(new)
    m = _model(None)
    m.h.rccl_connect(1, 0, m.h.rccl_unique_id())
    assert m.h.exchange_in_use() == "rccl"
    m.set_mesh(new)
    m.set_constraints(None)
    assert _same(m.loss_and_grad(), ref.loss_and_grad()) and m.constraints() == {}
    with pytest.raises(_lib.HpvError, match="exchange connected"):
        m.set_constraints(CONS)
    assert m.constraints() == {} and _same(m.loss_and_grad(), ref.loss_and_grad())      # rolled back: model and handle agree
    m.h.rccl_disconnect()
    monkeypatch.setattr(m, "world", 2)
    with pytest.raises(ValueError, match="no collective before the adjoint"):
        m.set_constraints(CONS)
    assert m.constraints() == {}
