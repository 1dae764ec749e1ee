"""The strong residual in divergence form on the device (hpv_set_strong_form_div, hpv_linear_indicators, k_div_indicators;
VPINNLinear / VPINNNonlinear(strong_form="divergence")) against tests/divform_reference.py (CPU, fp64; tests/test_divform_host.py
proves it).  TOL = 1e-9 as in tests/test_gpu_linadapt.py: relative per indicator column, relative to max|r| on r.  Networks are
[d, 8, 8, 1] unless stated.  The measured errors are in profiles/divergence_form.md."""
import numpy as np
import pytest

import divform_reference as dv
import generic_point as gp
import linadapt_reference as la
import linear_reference as lr
import mapped_reference as mr
from cases import rel

pytestmark = pytest.mark.gpu

TOL = 1e-9
L2 = [2, 8, 8, 1]
NT = (4, 3)
TERMS = ("u2", "u3", "exp", "adv")
BOXES = np.asarray(lr.BOXES2[:3])
# three convex quadrilaterals with no two sides parallel (those of tests/test_gpu_mapped.py), two boxes of the (r, theta) plane
QUADS = np.array([[[-1.0, -1.0], [-0.1, -0.9], [-0.25, 0.05], [-0.9, -0.2]],
                  [[-0.1, -0.9], [1.0, -1.0], [0.8, -0.15], [-0.25, 0.05]],
                  [[-0.9, -0.2], [-0.25, 0.05], [-0.4, 1.0], [-1.0, 0.8]]])
POLAR = np.array([[1.0, 1.4, 0.0, 0.9], [1.4, 2.0, 0.0, 0.9]])
COUNTS3, COUNTS2 = ([4, 2, 3], [1, 3, 2]), ([4, 3], [2, 3])
_CACHE = {}


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _f_phys(X):
    return np.sin(2.3 * X[..., 0] + 0.7) * np.cosh(0.8 * X[..., 1]) + 0.4


def _box_ansatz():
    def g(P):
        x, y = P[:, 0], P[:, 1]
        return np.stack([np.sin(x) * y, np.cos(x) * y, np.sin(x)], 1)

    def d(P):
        x, y = P[:, 0], P[:, 1]
        a, b = 1.0 - x * x, 1.0 - y * y
        return np.stack([a * b, -2.0 * x * b, -2.0 * y * a], 1)
    return dict(g=g, d=d)


def _mesh(geom):
    from hp_vpinns_amd.adapt import ElementMesh, MappedMesh
    if geom == "boxes":
        return ElementMesh(BOXES, *COUNTS3)
    return MappedMesh.from_quads(QUADS, *COUNTS3) if geom == "quads" else MappedMesh(POLAR, *COUNTS2, map=mr.polar_map)


def _mcase(geom, q=(6, 5), diagonal=False, dirs=True, ansatz=None, zero=False, shard=None, seed=0):
    """(p, f physical (n_owned, NQ), reference) of a mapped_reference problem with all four nonlinear terms and (dirs) two trainable
    directions, the first a tensor kappa (kxy only; kxx on a diagonal handle); computed once and left unchanged"""
    key = (geom, q, diagonal, dirs, ansatz, zero, shard, seed)
    if key not in _CACHE:
        rx, ry = lr.rule(q[0]), lr.rule(q[1])
        X, A = {"boxes": lambda: mr.geom_boxes(BOXES, rx[0], ry[0]), "quads": lambda: mr.geom_quads(QUADS, rx[0], ry[0]),
                "polar": lambda: mr.geom_polar(POLAR, rx[0], ry[0])}[geom]()
        ne, nq = X.shape[0], q[0] * q[1]
        rng = np.random.default_rng(8800 + seed + sum(map(ord, geom)))
        coefs = mr.random_coefs(rng, ne, nq, () if zero else TERMS, diagonal=diagonal)
        dd = []
        if dirs:
            K = np.zeros((ne, nq, 2, 2))
            K[:, :, 0, 0 if diagonal else 1] = mr._signed(rng, (ne, nq))
            dd = [dict(K=K), dict(s=mr._signed(rng, (ne, nq)), a3=mr._signed(rng, (ne, nq)), g=mr._signed(rng, (ne, nq, 2)))]
        hb = {None: None, "box": _box_ansatz(), "polar": __import__("hp_vpinns_amd.drivers.linear", fromlist=["x"]).annulus_hard_bc()}[ansatz]
        p = mr.problem(L2, 8800 + seed, X, A, rx, ry, NT, coefs, counts=COUNTS3 if ne == 3 else COUNTS2, dirs=dd, c0=[0.7, -0.4] if dd else [],
                       ansatz=hb, boxes=BOXES if geom == "boxes" else None, shard=shard)
        p["geom"] = geom
        if zero:
            p["theta"] = np.zeros_like(p["theta"])
        f = _f_phys(X[p["eb"]:p["ee"]])
        _CACHE[key] = (p, f, dv.reference(p, f))
    return _CACHE[key]


class MDev:
    """the C-ABI on a mapped_reference problem: boxes take the physical planes, mapped elements the product's points (adapt.MappedMesh),
    its fold (VPINNLinear._fold) and 1 / det A; then hpv_set_strong_form_div unless div=False"""

    def __init__(self, p, tensor=True, div=True, backend=None):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.init import n_params, pad_plan
        from hp_vpinns_amd.quadrature import diff_matrix
        from hp_vpinns_amd.testfcn import tables_1d
        from hp_vpinns_amd.vpinn import VPINNLinear
        self.p, nc = p, len(p["dirs"])
        plan = pad_plan(p["layers"], nc)
        self.dev_layers, self.idx = plan if plan is not None else (p["layers"], None)
        self.n_dev = n_params(self.dev_layers, nc)
        kw = {} if backend is None else dict(backend=backend)
        self.h = h = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, self.dev_layers, lr=1e-3, lossb_weight=p["lbw"], n_coef=nc, **kw)
        (xi, wx), (yi, wy) = p["xr"], p["yr"]
        eb, ee = p["eb"], p["ee"]
        ne = ee - eb
        n = ne * xi.size * yi.size
        h.set_quadrature(xi, wx, yi, wy)
        h.set_tables(tables_1d(p["ntx"], xi), tables_1d(p["nty"], yi))
        A = self.inv_det = None
        if p["boxes"] is not None:
            h.set_element_boxes(p["boxes"], eb, ee)
        else:
            mesh = _mesh(p["geom"])
            self.Xall = mesh.quad_points(xi, yi).reshape(len(mesh), -1, 2).transpose(0, 2, 1)
            h.set_element_points(self.Xall, eb, ee)
            A = mesh.geometry(xi, yi, eb, ee)[1]
            self.inv_det = 1.0 / (A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0])
        h.set_rhs(p["F"].reshape(-1))
        h.set_active_tests_2d(p["nax"], p["nay"])

        def planes(c):
            z = dict(K=np.zeros((ne, n // ne, 2, 2)), b=np.zeros((ne, n // ne, 2)), s=np.zeros((ne, n // ne)))
            z.update({k: v[eb:ee] for k, v in c.items()})
            K = z["K"].reshape(n, 2, 2) if tensor else np.stack([z["K"][..., 0, 0].reshape(n), z["K"][..., 1, 1].reshape(n)], 1)
            op = VPINNLinear._fold(A, tensor, K, (z["b"].reshape(n, 2), z["s"].reshape(n)))
            g = z["g"].reshape(n, 2) if "g" in z else np.zeros((n, 2))
            return op, VPINNLinear._fold(A, False, None, tuple(z[k].reshape(n) if k in z else np.zeros(n) for k in ("a2", "a3", "ae")) + (g,))
        self.op, self.nl = planes(p["coefs"])
        self.dirs = np.stack([np.concatenate(planes(d), 0) for d in p["dirs"]], 0) if nc else None
        self.tensor = tensor
        self.hand_planes()
        self.D = (diff_matrix(xi), diff_matrix(yi))
        if div:
            h.set_strong_form_div(*self.D, self.inv_det)
        self.set_params(mr.full0(p))

    def hand_planes(self):
        h, p = self.h, self.p
        (h.set_operator_tensor if self.tensor else h.set_operator)(self.op)
        if any(k in p["coefs"] for k in ("a2", "a3", "ae", "g")):
            h.set_nonlinear(self.nl)
        if self.dirs is not None:
            h.set_trainable(self.dirs)
        if p["ansatz"] is not None:
            X = p["X"][p["eb"]:p["ee"]].reshape(-1, 2)
            fld = lambda c: np.asarray(c(X)) if callable(c) else np.concatenate([np.full((X.shape[0], 1), float(c)), np.zeros((X.shape[0], 2))], 1)
            h.set_ansatz(0, np.concatenate([fld(p["ansatz"]["g"]).T, fld(p["ansatz"]["d"]).T], 0))

    def set_params(self, th):
        t = np.asarray(th, dtype=np.float64)
        if self.idx is not None:
            t = np.zeros(self.n_dev)
            t[self.idx] = th
        self.h.set_params(t)

    def loss_and_grad(self):
        l3, g = self.h.loss_and_grad(True)
        return np.asarray(l3), (g if self.idx is None else g[self.idx])


def _col_err(ind, ref):
    return np.array([rel(ind[:, c], ref[:, c]) if np.any(ref[:, c] != 0.0) else float(np.abs(ind[:, c]).max()) for c in range(5)])


def _check(tag, h, fq, ref):
    ind, r = h.linear_indicators(fq, want_r=True)
    ec = _col_err(ind, ref["ind"])
    er = float(np.abs(r.reshape(ref["r"].shape) - ref["r"]).max() / np.abs(ref["r"]).max())
    print("%s | backend %d | columns %s | r %.2e (max|r| %.3g)" % (tag, h.backend_in_use(), np.array2string(ec, precision=2), er, np.abs(ref["r"]).max()))
    assert ec.max() < TOL, (tag, "indicator columns", ec)
    assert er < TOL, (tag, "strong residual", er)
    return ind, r


# ---- linadapt_reference problems: 1-D and diagonal boxes ----------------------------------------------------------------------------------
LCASES = {
    # 1-D, 3 unequal elements, rule 7, counts (4, 3, 2); all four terms; directions in k and in a3
    "1d-7": la._c("1d-7", [1, 8, 8, 1], la.BOXES1[:3], 7, 4, 9601, counts=([4, 3, 2], None), terms=TERMS, dirs=[[0], [4]]),
    # diagonal boxes, rule 6 x 5, tests 4 x 3; all four terms; directions in kx and in s
    "2d-6x5": la._c("2d-6x5", L2, la.BOXES2[:3], (6, 5), NT, 9602, terms=TERMS, dirs=[[0], [4]]),
    # 272 points: the thread loop wraps with a tail; per-element counts
    "2d-17x16": la.CASES["2d-17x16-counts"],
    "1d-80": la._c("1d-80", [1, 8, 8, 1], la.BOXES1[:2], 80, 7, 9603, terms=("u3",)),
}


def _lcase(name):
    if name not in _CACHE:
        p = la.problem(LCASES[name])
        _CACHE[name] = (p, dv.reference_lin(p))
    return _CACHE[name]


def _ldev(p, backend=None):
    """the handle of tests/test_gpu_linadapt.Dev's sequence, with the divergence form in place of the elementwise one"""
    from test_gpu_linadapt import Dev
    d = Dev(p, strong=False, backend=backend)
    d.h.set_strong_form_div(*d.D)
    return d


@pytest.mark.parametrize("name", list(LCASES))
def test_boxes_1d_and_diagonal_against_the_reference(name):
    p, ref = _lcase(name)
    d = _ldev(p)
    ind, r = _check(name, d.h, p["f"], ref)
    if p["dim"] == 1:
        assert np.all(ind[:, 4] == 0.0)
    ind2, r2 = d.h.linear_indicators(p["f"], want_r=True)
    assert ind2.tobytes() == ind.tobytes() and r2.tobytes() == r.tobytes()
    assert d.h.linear_indicators(p["f"]).tobytes() == ind.tobytes()


@pytest.mark.parametrize("geom", ["boxes", "quads", "polar"])
def test_tensor_and_mapped_elements_against_the_reference(geom):
    """a non-symmetric K per point, all four nonlinear terms, two trainable directions (one in kxy only) on three boxes, three bilinear
    quadrilaterals and two polar elements; two calls return the same bytes"""
    p, f, ref = _mcase(geom)
    d = MDev(p)
    ind, r = _check("tensor " + geom, d.h, dv.device_f(p, f), ref)
    ind2, r2 = d.h.linear_indicators(dv.device_f(p, f), want_r=True)
    assert ind2.tobytes() == ind.tobytes() and r2.tobytes() == r.tobytes()
    l3, g = d.loss_and_grad()
    l3o, go, _ = mr.reference(p)
    assert rel(l3, l3o) < TOL and gp.worst_block(g, go, L2, 2)[1] < TOL      # (the pass is what it was)


def test_smallest_rule():
    """qx = 2: the smallest differentiation matrix (two Lobatto nodes, D = [[-1/2, 1/2], [-1/2, 1/2]]); no trainable directions"""
    p, f, ref = _mcase("quads", q=(2, 3), dirs=False)
    d = MDev(p)
    _check("2 x 3", d.h, dv.device_f(p, f), ref)


@pytest.mark.parametrize("geom,ansatz", [("boxes", "box"), ("polar", "polar")])
def test_ansatz(geom, ansatz):
    """u = G + D N: r equals the reference fed the post-ansatz u, u_x, u_y (no second derivative of G or D exists anywhere)"""
    p, f, ref = _mcase(geom, ansatz=ansatz)
    d = MDev(p)
    _check("ansatz " + geom, d.h, dv.device_f(p, f), ref)
    raw = dict(p, ansatz=None)
    assert np.abs(dv.strong(raw, f) - ref["r"]).max() > 1e-3 * np.abs(ref["r"]).max()      # (the ansatz matters in this case)


@pytest.mark.parametrize("geom", ["boxes", "quads"])
def test_zero_network_known_answer(geom):
    """theta = 0: column 1 is sum_q w f^2 det A per element, the quadrature of int f^2 dx"""
    p, f, ref = _mcase(geom, dirs=False, zero=True)
    d = MDev(p)
    ind, r = _check("zero network " + geom, d.h, dv.device_f(p, f), ref)
    A = p["A"]
    want = np.sum(np.outer(p["yr"][1], p["xr"][1]).reshape(1, -1) * f ** 2 * (A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]), axis=1)
    assert rel(ind[:, 1], want) < TOL and rel(r.reshape(f.shape), -f) < TOL


def test_shard_and_generic_backend():
    """a shard [1, 3) returns rows 1..2 of the full table; backend="generic" against the same reference"""
    from hp_vpinns_amd import _lib
    p, f, ref = _mcase("quads")
    full = MDev(p).h.linear_indicators(dv.device_f(p, f))
    ps, fs, refs = _mcase("quads", shard=(1, 3))
    ind, _ = _check("shard [1, 3)", MDev(ps).h, dv.device_f(ps, fs), refs)
    assert ind.shape == (2, 5) and rel(ind, full[1:3]) < TOL
    g = MDev(p, backend=_lib.BACKEND_GENERIC)
    assert g.h.backend_in_use() == _lib.BACKEND_GENERIC
    _check("generic backend", g.h, dv.device_f(p, f), ref)


def test_contracts():
    """the two kinds exclude each other; hpv_set_strong_form refuses tensor, mapped and ansatz handles with -1 as ever; new points
    orphan inv_det (-3) until it is handed again; NaN / non-positive inv_det and a rule beyond 64 KiB of LDS are refused; after every
    refusal loss_and_grad still matches its reference"""
    from hp_vpinns_amd import _lib
    p, f, ref = _mcase("quads")
    d = MDev(p)
    h = d.h
    l3o, go, _ = mr.reference(p)

    def usable():
        l3, g = d.loss_and_grad()
        assert rel(l3, l3o) < TOL and gp.worst_block(g, go, L2, 2)[1] < TOL

    def refused(call, code=-1, word=None):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == code, (e.value.code, str(e.value))
        if word:
            assert word in str(e.value), str(e.value)
        usable()
    refused(lambda: h.set_strong_form(*d.D), -1)                                   # a mapped tensor handle, as ever
    bad = d.inv_det.copy()
    bad[7] = np.nan
    refused(lambda: h.set_strong_form_div(*d.D, bad), -1, "inv_det")
    bad[7] = -1.0
    refused(lambda: h.set_strong_form_div(*d.D, bad), -1, "inv_det")
    bad[7] = 0.0
    refused(lambda: h.set_strong_form_div(*d.D, bad), -1, "inv_det")
    refused(lambda: h.set_strong_form_div(*d.D, None), -1, "inv_det")              # required on unit elements
    refused(lambda: h.set_strong_form_div(*d.D, d.inv_det[:-1]), -1, "inv_det")
    refused(lambda: h.set_strong_form_div(d.D[0][:, :-1], d.D[1], d.inv_det), -1)
    _check("contracts: after the refusals", h, dv.device_f(p, f), ref)             # what was given earlier stays
    # new points orphan the matrices and inv_det
    h.set_element_points(d.Xall)                                                   # (allowed while the divergence form is active)
    h.set_rhs(p["F"].reshape(-1))
    d.hand_planes()
    refused(lambda: h.linear_indicators(dv.device_f(p, f)), -3, "hand the strong form over again")
    refused(lambda: h.set_strong_form(*d.D), -1)
    h.set_strong_form_div(*d.D, d.inv_det)
    _check("contracts: handed again", h, dv.device_f(p, f), ref)
    h.set_strong_form_div(None, None, None)                                        # removed: refused as a handle that never opted in
    refused(lambda: h.linear_indicators(dv.device_f(p, f)), -1)
    # boxes: inv_det must be absent; the two kinds exclude each other; tensor and ansatz handles refuse the elementwise kind
    pb, fb, refb = _mcase("boxes", diagonal=True)
    b = MDev(pb, tensor=False)
    hb = b.h
    l3b, gb, _ = mr.reference(pb)

    def refused_b(call, word=None):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == -1 and (word is None or word in str(e.value)), (e.value.code, str(e.value))
        l3, g = b.loss_and_grad()
        assert rel(l3, l3b) < TOL and gp.worst_block(g, gb, L2, 2)[1] < TOL
    refused_b(lambda: hb.set_strong_form_div(*b.D, np.ones(3 * 30)), "inv_det")
    refused_b(lambda: hb.set_strong_form(*b.D), "exclude each other")
    _check("contracts: diagonal boxes", hb, fb.reshape(-1), refb)
    hb.set_strong_form_div(None, None, None)
    hb.set_strong_form(*b.D)
    refused_b(lambda: hb.set_strong_form_div(*b.D), "exclude each other")
    refused_b(lambda: hb.set_ansatz(0, np.ones((6, 3 * 30))))                      # the elementwise kind keeps its refusal of an ansatz
    hb.set_strong_form(None, None)
    hb.set_ansatz(0, np.concatenate([np.zeros((3, 90)), np.ones((1, 90)), np.zeros((2, 90))]))      # u = 0 + 1 * N
    refused_b(lambda: hb.set_strong_form(*b.D), "ansatz")
    hb.set_strong_form_div(*b.D)
    _check("contracts: trivial ansatz", hb, fb.reshape(-1), refb)
    hb.set_ansatz(0, None)
    pt, ft, reft = _mcase("boxes")
    t = MDev(pt, div=False)
    with pytest.raises(_lib.HpvError) as e:
        t.h.set_strong_form(*t.D)
    assert e.value.code == -1 and "u_xy" in str(e.value)
    # a rule whose workgroup would need more than 64 KiB of LDS: 46 x 46 is 8 * (2 * 46 * 47 + 2 * 46 * 47 + 16) = 69 312 B (with one test
    # function per direction the projection kernel itself still fits)
    from hp_vpinns_amd.quadrature import diff_matrix
    from hp_vpinns_amd.testfcn import tables_1d
    big = lr.rule(46)
    assert la.lds_bytes(2, 46, 46) > 64 * 1024 > la.lds_bytes(2, 17, 16)
    pl, refl = _lcase("2d-6x5")
    dl = _ldev(pl)
    hl = dl.h
    hl.set_rhs(None)                                                               # (F of the old tables would be checked against the new)
    hl.set_quadrature(big[0], big[1], big[0], big[1])
    hl.set_tables(tables_1d(1, big[0]), tables_1d(1, big[0]))
    hl.set_element_boxes(BOXES[:1])
    with pytest.raises(_lib.HpvError) as e:
        hl.set_strong_form_div(diff_matrix(big[0]), diff_matrix(big[0]))
    assert e.value.code == -1 and "LDS" in str(e.value)
    dl.populate(pl, strong=False)                                                  # the handle stays usable
    hl.set_strong_form_div(*dl.D)
    _check("contracts: after the LDS refusal", hl, pl["f"], refl)
    l3, _ = dl.loss_and_grad()
    lossv = la.ir.var_part(pl, grad=False)["lossv"]
    assert abs(l3[2] - lossv) < TOL * lossv


def test_training_is_not_disturbed():
    """four Adam steps with and without a linear_indicators call in between: bitwise equal parameters (captured graphs untouched)"""
    p, f, _ = _mcase("quads")
    a, b = MDev(p), MDev(p)
    a.h.step(4, False)
    b.h.step(2, False)
    b.h.linear_indicators(dv.device_f(p, f), want_r=True)
    b.h.step(2, False)
    assert a.h.get_params().tobytes() == b.h.get_params().tobytes()
    assert a.h.get_state().tobytes() == b.h.get_state().tobytes()


# ---- the classes and the drivers -------------------------------------------------------------------------------------------------------------
def test_dual_norm_column_0():
    """metric="physical" on quadrilaterals and "energy" on boxes (dense Gram factors): column 0 is the forward-only pass's loss_e --
    it sums to lossv -- while column 2 stays the plain sum of R^2"""
    from hp_vpinns_amd.vpinn import VPINNLinear
    Kc = np.array([[1.3, 0.4], [0.2, 0.9]])
    for mesh, metric in ((_mesh("quads"), "physical"), (_mesh("boxes"), "energy")):
        m = VPINNLinear(L2, mesh=mesh, n_quad=(6, 5), kappa=Kc, beta=np.array([0.5, -1.1]), sigma=1.0, f=lambda P: _f_phys(P),
                        residual_norm=dict(kind="dual", metric=metric, mass=0.5), strong_form="divergence", init_params=gp.generic_theta(L2, 8900))
        ind = m.element_indicators()
        lossv = float(np.asarray(m.loss())[2])
        R = m.h.residuals(len(mesh) * 12).reshape(len(mesh), -1)
        print("dual %s: sum of column 0 %.12e, lossv %.12e" % (metric, ind[:, 0].sum(), lossv))
        assert abs(ind[:, 0].sum() - lossv) < TOL * lossv
        assert rel(ind[:, 2], np.sum(R ** 2, axis=1)) < TOL and np.all(ind[:, 0] != ind[:, 2] / (mesh.nax * mesh.nay))
        assert np.all(ind[:, 1] > 0.0)


def test_class_adapts_on_a_mapped_mesh():
    """VPINNLinear(mesh=MappedMesh, strong_form="divergence", hard_bc=..).adapt() grows the mesh, parameters and Adam state stay bit
    for bit, the loss on the new mesh matches mapped_reference; the residual at the quadrature points matches the reference;
    strong_form None and "elementwise" refuse as before"""
    from test_gpu_mapped import _model_problem
    from hp_vpinns_amd.adapt import MappedMesh
    from hp_vpinns_amd.drivers import linear
    from hp_vpinns_amd.vpinn import VPINNLinear
    Kc = np.array([[1.3, 0.4], [-0.7, 0.9]])
    kw = dict(n_quad=(6, 5), kappa=lambda P: Kc[None] * (1.0 + 0.3 * P[:, 0] * P[:, 1])[:, None, None], beta=np.array([0.5, -1.1]),
              sigma=lambda P: 1.0 + P[:, 0], f=linear._annulus_f, init_params=gp.generic_theta(L2, 8901))
    mesh = MappedMesh(POLAR, *COUNTS2, map=mr.polar_map)
    m = VPINNLinear(L2, mesh=mesh, hard_bc=linear.annulus_hard_bc(), strong_form="divergence", **kw)
    m.train(3)
    p = _model_problem(m)
    fq = linear._annulus_f(p["X"].reshape(-1, 2)).reshape(p["X"].shape[:2])
    ref = dv.reference(p, fq)
    ind = m.element_indicators()
    r = m.strong_residual_at_quad()
    assert _col_err(ind, ref["ind"]).max() < TOL and np.abs(r - ref["r"]).max() < TOL * np.abs(ref["r"]).max()
    st = m.h.get_state()
    new = m.adapt(theta=0.6)
    assert len(new) > len(mesh) and isinstance(m.mesh, MappedMesh) and len(m.mesh) == len(new)
    assert m.h.get_state().tobytes() == st.tobytes()
    l3 = np.asarray(m.loss())
    l3o = mr.reference(_model_problem(m))[0]
    assert rel(l3, l3o) < TOL
    assert m.element_indicators().shape == (len(new), 5)
    rows = m.train_adaptive(6, 3, max_elements=len(new) + 3)
    assert len(rows) == 1 and np.isfinite(rows[0][2])
    with pytest.raises(NotImplementedError):
        m.residual(np.zeros((1, 2)))
    for sf, exc in ((None, ValueError), ("elementwise", ValueError)):
        with pytest.raises(exc):
            VPINNLinear(L2, mesh=mesh, strong_form=sf, **kw).adapt()
    with pytest.raises(ValueError, match="do not go together"):
        VPINNLinear(L2, mesh=_mesh("boxes"), n_quad=(6, 5), hard_bc=_box_ansatz(), strong_form="elementwise")
    with pytest.raises(NotImplementedError):
        VPINNLinear(L2, mesh=_mesh("boxes"), n_quad=(6, 5)).element_indicators()


def test_nonlinear_class_with_hard_bc_adapts_in_1d():
    """VPINNNonlinear(hard_bc=.., strong_form="divergence") in 1-D: adapt() grows the mesh and leaves the state bit for bit"""
    from hp_vpinns_amd.drivers.linear import graded_grid, interval_hard_bc
    from hp_vpinns_amd.vpinn import VPINNNonlinear
    m = VPINNNonlinear([1, 8, 8, 1], grid_x=graded_grid(3), n_quad=9, n_test=4, kappa=-0.2, beta=1.0, f=lambda P: 1.0 + 0.8 * np.sin(20.0 * P[:, 0]),
                       cubic=-0.5, advection=0.3, hard_bc=interval_hard_bc(0.0, 1.0, 0.0, 0.0), strong_form="divergence", activation="sin", seed=5)
    m.train(3)
    st, l0 = m.h.get_state(), np.asarray(m.loss())
    ind = m.element_indicators()
    assert ind.shape == (3, 5) and np.all(ind[:, 1] > 0.0) and np.all(ind[:, 4] == 0.0)
    assert m.strong_residual_at_quad().shape == (3, 1, 9)
    assert np.array_equal(np.asarray(m.loss()), l0)
    new = m.adapt()
    assert len(new) > 3 and m.h.get_state().tobytes() == st.tobytes() and np.all(np.isfinite(m.loss()))
    m.set_hard_bc()                                                               # the ansatz may go and come back under this kind
    m.set_hard_bc(**interval_hard_bc(0.0, 1.0, 0.0, 0.0))
    assert m.element_indicators().shape == (len(new), 5)


def test_drivers_adapt():
    """annulus --adapt-every and boundary-layer --hard-bc --adapt-every at small width: more elements at the end, a finite loss"""
    from hp_vpinns_amd.drivers import linear
    out = linear.run_annulus(**dict(linear.ANNULUS_SMALLEST, n_iter=300), adapt_every=100, max_elements=10, verbose=False)
    assert 4 < len(out["model"].mesh) <= 10 and len(out["adapt_rows"]) == 2 and np.isfinite(out["model"].loss()).all()
    out = linear.run_boundary_layer(**dict(linear.SMALLEST, n_iter=300), adapt_every=100, max_elements=8, hard_bc=True, verbose=False)
    assert 3 < len(out["model"].mesh) <= 8 and np.isfinite(out["model"].loss()).all() and out["bnd_err"] == 0.0
    out = linear.run_anisotropic(n_elements=2, n_quad=8, n_test=4, n_iter=200, layers=(2, 8, 8, 1), adapt_every=100, max_elements=8, verbose=False)
    assert 4 < len(out["model"].mesh) <= 8 and np.isfinite(out["model"].loss()).all()
