"""Quasilinear diffusion div(mu(u, |grad u|^2) K grad u) on the device (hpv_set_quasilinear; the _q instantiations of k_project_nl,
the QUASI instantiation of k_div_indicators; VPINNNonlinear(diffusivity=)) against tests/quasilinear_reference.py (CPU, fp64;
tests/test_quasilinear_host.py proves it).  Bounds: TOL = 1e-9 on the loss triple, R and the gradient per block, STEP_TOL = 1e-8 after
Adam steps, both imported from tests/test_gpu_generic_point.py as tests/test_gpu_nonlinear.py does.  The measured errors are in
profiles/quasilinear.md.

The C-ABI has no call that returns GBAR, so "GBAR at a padding point is exactly 0" is asserted where it can be: on the reference's
channel adjoints, and on the device through loss and gradient being those of the rule WITHOUT the padding points."""
import re

import numpy as np
import pytest

import dualdense_reference as dd
import generic_point as gp
import mapped_reference as mr
import linear_reference as lr
import quasilinear_reference as qr
from cases import rel
from test_gpu_generic_point import STEP_TOL, TOL

pytestmark = pytest.mark.gpu

L1, L2 = [1, 8, 8, 1], [2, 8, 8, 1]
BOXES1 = np.array([[0.0, 0.3], [0.3, 0.55], [0.55, 1.0]])
# a non-uniform 2 x 2 grid
BOXES_B = np.array([[-1.0, 0.3, -1.0, -0.2], [0.3, 1.0, -1.0, -0.2], [-1.0, 0.3, -0.2, 1.0], [0.3, 1.0, -0.2, 1.0]])
BOXES_C = np.array([[-1.0, 0.2, -1.0, 1.0], [0.2, 1.0, -1.0, 1.0]])
# two convex quadrilaterals with no two sides parallel
QUADS = np.array([[[-1.0, -1.0], [-0.1, -0.9], [-0.25, 0.05], [-0.9, -0.2]],
                  [[-0.1, -0.9], [1.0, -1.0], [0.8, -0.15], [-0.25, 0.05]]])
# name: (geometry, q, nt, counts, pad)
SHAPES = {
    "A": ("1d", 5, 3, [3, 2, 3], 0),
    "B": ("boxes", (5, 4), (3, 2), ([3, 2, 3, 1], [2, 2, 1, 2]), 0),
    "C": ("boxes-c", (17, 16), (9, 8), None, 0),
    "D": ("quads", (6, 5), (4, 3), ([4, 3], [2, 3]), 0),
    "E": ("boxes", (6, 5), (3, 2), ([3, 2, 3, 1], [2, 2, 1, 2]), 1),
}
# name: (use_u, use_grad, r, pointwise terms)
VARIANTS = {
    "u": (True, False, 0.0, ()),
    "grad-": (False, True, -0.5, ()),
    "grad+": (False, True, 0.5, ()),
    "both": (True, True, -0.5, ()),
    "both+terms": (True, True, 0.5, ("u3", "adv")),
}
WORST = {}
_CACHE = {}


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _box_ansatz():
    def g(P):
        x, y = P[:, 0], P[:, 1]
        return np.stack([np.sin(x) * y, np.cos(x) * y, np.sin(x)], 1)

    def d(P):
        x, y = P[:, 0], P[:, 1]
        a, b = 1.0 - x * x, 1.0 - y * y
        return np.stack([a * b, -2.0 * x * b, -2.0 * y * a], 1)
    return dict(g=g, d=d)


def _geometry(kind, rx, ry):
    if kind == "1d":
        return qr.geom_1d(BOXES1, rx[0]) + (BOXES1,)
    if kind == "quads":
        return mr.geom_quads(QUADS, rx[0], ry[0]) + (None,)
    b = BOXES_C if kind == "boxes-c" else BOXES_B
    return mr.geom_boxes(b, rx[0], ry[0]) + (b,)


def _problem(shape, variant, norm=None, ansatz=False):
    """the case's arrays; norm: None | ("table", mass) | ("dense", mass, S).  Computed once and left unchanged."""
    key = (shape, variant, norm if norm is None else norm[:2], ansatz)
    if key in _CACHE:
        return _CACHE[key]
    kind, q, nt, counts, pad = SHAPES[shape]
    use_u, use_grad, r, terms = VARIANTS[variant]
    seed = 9700 + 10 * sorted(SHAPES).index(shape) + sorted(VARIANTS).index(variant)
    rng = np.random.default_rng(seed)
    dim = 1 if kind == "1d" else 2
    rx = lr.rule((q if dim == 1 else q[0]) - pad, pad)
    ry = lr.rule(q[1] - pad, pad) if dim == 2 else None
    X, A, boxes = _geometry(kind, rx, ry)
    ne, nq = X.shape[:2]
    if dim == 2:
        coefs = mr.random_coefs(rng, ne, nq, terms, diagonal=kind != "quads")
    else:
        coefs = dict(K=mr._signed(rng, (ne, nq, 1, 1)), b=mr._signed(rng, (ne, nq, 1)), s=mr._signed(rng, (ne, nq)))
        if "u3" in terms:
            coefs["a3"] = mr._signed(rng, (ne, nq))
        if "adv" in terms:
            coefs["g"] = mr._signed(rng, (ne, nq, 1))
    qp = qr.quasi_planes(rng, ne, nq, use_u, use_grad, r)
    p = qr.problem(dim, L1 if dim == 1 else L2, seed, X, A, (rx, ry), nt, coefs, qp, counts=counts, data=7 if shape == "B" else 0,
                   ansatz=_box_ansatz() if ansatz else None, boxes=boxes)
    p["kind"] = kind
    if norm is not None and norm[0] == "table":
        p["gram"] = qr.gram_table(p, norm[1])
    elif norm is not None:
        geom = (lambda x, y: mr.geom_quads(QUADS, x, y)) if kind == "quads" else (lambda x, y: mr.geom_boxes(boxes, x, y))
        p["gram"] = qr.gram_dense(p, geom, norm[1], norm[2])
    _CACHE[key] = (p, qr.reference(p))
    return _CACHE[key]


def _mesh(p):
    from hp_vpinns_amd.adapt import MappedMesh
    return MappedMesh.from_quads(QUADS, p["nax"], p["nay"])


class Dev:
    """the C-ABI on a quasilinear_reference problem: boxes and 1-D elements take the physical planes, mapped elements the product's
    points and its fold (VPINNLinear._fold); the quasilinear planes go in plain everywhere.  quasi=False: a handle that never hears of
    hpv_set_quasilinear"""

    def __init__(self, p, quasi=True, backend=None):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.init import n_params, pad_plan
        from hp_vpinns_amd.testfcn import tables_1d
        from hp_vpinns_amd.vpinn import VPINNLinear
        self.p, dim = p, p["dim"]
        plan = pad_plan(p["layers"], 0)
        self.dev_layers, self.idx = plan if plan is not None else (p["layers"], None)
        self.n_dev = n_params(self.dev_layers, 0)
        kw = {} if backend is None else dict(backend=backend)
        self.h = h = _lib.Handle(_lib.PDE_LINEAR1D if dim == 1 else _lib.PDE_LINEAR2D, 1, _lib.ACT_SIN if dim == 1 else _lib.ACT_TANH,
                                 self.dev_layers, lr=1e-3, lossb_weight=p["lbw"], **kw)
        (xi, wx), (yi, wy) = p["xr"], p["yr"]
        ne = p["ee"] - p["eb"]
        n = ne * p["X"].shape[1]
        if dim == 1:
            h.set_quadrature(xi, wx, None, None)
            h.set_tables(tables_1d(p["ntx"], xi), None)
        else:
            h.set_quadrature(xi, wx, yi, wy)
            h.set_tables(tables_1d(p["ntx"], xi), tables_1d(p["nty"], yi))
        self.A = self.inv_det = None
        self.tensor = p["kind"] == "quads"
        self.hand_elements()
        h.set_rhs(p["F"].reshape(-1))
        if p["nax"] is not None:
            if dim == 1:
                h.set_active_tests(p["nax"])
            else:
                h.set_active_tests_2d(p["nax"], p["nay"])
        c = p["coefs"]
        z = lambda k, sh: c[k].reshape((n,) + sh) if k in c else np.zeros((n,) + sh)
        K = c["K"].reshape(n, dim, dim)
        Kd = K if self.tensor else np.stack([K[:, a, a] for a in range(dim)], 1)
        self.op = VPINNLinear._fold(self.A, self.tensor, Kd, (z("b", (dim,)), z("s", ())))
        self.nl = VPINNLinear._fold(self.A, False, None, (z("a2", ()), z("a3", ()), z("ae", ()), z("g", (dim,))))
        self.has_nl = any(k in c for k in ("a2", "a3", "ae", "g"))
        self.qp, self.qr = qr.device_planes(p)
        self.hand_planes(quasi)
        if p["ansatz"] is not None:
            Xq = p["X"].reshape(-1, 2)
            h.set_ansatz(0, np.concatenate([np.asarray(p["ansatz"]["g"](Xq)).T, np.asarray(p["ansatz"]["d"](Xq)).T], 0))
        if p["data"] is not None:
            h.set_data(*p["data"])
            if p["ansatz"] is not None:
                Xd = p["data"][0]
                h.set_ansatz(1, np.concatenate([np.asarray(p["ansatz"]["g"](Xd)).T, np.asarray(p["ansatz"]["d"](Xd)).T], 0))
        self.set_params(p["theta"])

    def hand_elements(self):
        h, p = self.h, self.p
        if p["boxes"] is not None:
            h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
            return
        mesh = _mesh(p)
        xi, yi = p["xr"][0], p["yr"][0]
        h.set_element_points(mesh.quad_points(xi, yi).reshape(len(mesh), -1, 2).transpose(0, 2, 1), p["eb"], p["ee"])
        self.A = mesh.geometry(xi, yi, p["eb"], p["ee"])[1]
        self.inv_det = 1.0 / (self.A[:, 0, 0] * self.A[:, 1, 1] - self.A[:, 0, 1] * self.A[:, 1, 0])

    def hand_planes(self, quasi=True):
        h = self.h
        (h.set_operator_tensor if self.tensor else h.set_operator)(self.op)
        if self.has_nl:
            h.set_nonlinear(self.nl)
        if quasi:
            h.set_quasilinear(self.qp, self.qr)

    def strong_form_div(self):
        from hp_vpinns_amd.quadrature import diff_matrix
        p = self.p
        self.h.set_strong_form_div(diff_matrix(p["xr"][0]), diff_matrix(p["yr"][0]) if p["dim"] == 2 else None, self.inv_det)

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

    def residuals(self):
        p = self.p
        return self.h.residuals((p["ee"] - p["eb"]) * p["ntx"] * p["nty"]).reshape(-1, p["nty"], p["ntx"])

    def everything(self):
        l3, g = self.loss_and_grad()
        return l3, g, self.residuals()


def _rel3(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def _against_reference(tag, d, ref):
    p = d.p
    l3o, go, Ro = ref
    l3m, gm, Rm = d.everything()
    v = d.h.kernel_variant()
    lf = d.h.loss_and_grad(False)[0]
    e3, ef = _rel3(l3m, l3o), _rel3(lf, l3o)
    kb, eb = gp.worst_block(gm, go, p["layers"], 0)
    eR = float(np.linalg.norm(Rm - Ro) / np.linalg.norm(Ro))
    print("%s | %s | loss3 %s | worst block %s %.2e (global %.2e) | forward-only %s | residuals %.2e" % (tag, v, e3, kb, eb, rel(gm, go), ef, eR))
    WORST[tag] = (float(e3.max()), float(eb), float(ef.max()), eR)
    assert "k_project_nl<" in v and ";quasi" in v and d.h.lib.hpv_pass_structure(d.h._h) == 0, (tag, v)
    assert e3.max() < TOL, (tag, v, "loss triple", l3m, l3o)
    assert eb < TOL, (tag, v, "gradient block", kb, eb)
    assert ef.max() < TOL, (tag, v, "forward-only pass", lf, l3o)
    assert eR < TOL, (tag, v, "residuals", eR)
    assert np.all(Rm[Ro == 0.0] == 0.0), (tag, "inactive residual entries are exactly 0")
    again = d.everything()
    assert all(np.array_equal(x, y) for x, y in zip((l3m, gm, Rm), again)), (tag, "a second call returns the same bits")


# ---- the kernel against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_against_the_reference(shape, variant):
    p, ref = _problem(shape, variant)
    d = Dev(p)
    _against_reference("%s/%s" % (shape, variant), d, ref)
    v = d.h.kernel_variant()
    assert (";tensor" in v) == (shape == "D")
    terms = VARIANTS[variant][3]
    assert (";u3,adv;quasi" in v) if terms else re.search(r"k_project_nl<\d+x\d+/\d+x\d+;quasi", v), v


def _cut(p):
    """p of shape E without its padding points: the last point per direction leaves the rule and every per-point array"""
    (xi, wx), (yi, wy) = p["xr"], p["yr"]
    qx, qy, ne = xi.size, yi.size, p["X"].shape[0]
    cut = lambda a: np.ascontiguousarray(a.reshape((ne, qy, qx) + a.shape[2:])[:, :qy - 1, :qx - 1]).reshape((ne, (qy - 1) * (qx - 1)) + a.shape[2:])
    q = dict(p, xr=(xi[:-1], wx[:-1]), yr=(yi[:-1], wy[:-1]), X=cut(p["X"]), A=cut(p["A"]), coefs={k: cut(v) for k, v in p["coefs"].items()})
    q["q"] = dict(p["q"], m=cut(p["q"]["m"]), delta=cut(p["q"]["delta"]))
    return q


@pytest.mark.parametrize("variant", ["both", "both+terms"])
def test_padding_points_contribute_nothing(variant):
    p, ref = _problem("E", variant)
    assert p["xr"][1][-1] == 0.0 and p["yr"][1][-1] == 0.0
    adj = qr.channel_adjoints(p)
    (qx, qy), ne = (p["xr"][0].size, p["yr"][0].size), p["X"].shape[0]
    gu, gd = adj["gbar_u"].reshape(ne, qy, qx), adj["gbar_du"].reshape(ne, qy, qx, 2)
    assert np.all(gu[:, -1] == 0.0) and np.all(gu[:, :, -1] == 0.0) and np.all(gd[:, -1] == 0.0) and np.all(gd[:, :, -1] == 0.0)
    assert np.any(gu[:, :-1, :-1] != 0.0)
    l3o, go, Ro = qr.reference(_cut(p))
    l3, g, R = Dev(p).everything()
    assert _rel3(l3, l3o).max() < TOL and gp.block_rel(g, go, p["layers"]) < TOL and rel(R, Ro) < TOL


@pytest.mark.parametrize("shape,norm,mark", [("B", ("table", 0.5), ";dual>"), ("D", ("dense", 0.5, None), ";dual=dense>"),
                                             ("B", ("dense", 0.25, dd.S_energy), ";dual=dense>")], ids=["table-B", "dense-physical-D", "dense-energy-B"])
@pytest.mark.parametrize("variant", ["both", "both+terms"])
def test_dual_norms(shape, norm, mark, variant):
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.quadrature import gram_factors, gram_rule, gram_stacks
    p, ref = _problem(shape, variant, norm)
    d = Dev(p)
    if norm[0] == "table":
        sx, sy = gram_stacks(p["ntx"]), gram_stacks(p["nty"])
        d.h.set_residual_norm(_lib.NORM_DUAL, norm[1], sx[0], sx[1], sy[0], sy[1])
    else:
        x = gram_rule(p["ntx"], p["nty"])[0]
        if shape == "D":
            Xg, Ag = mr.geom_quads(QUADS, x, x)
        else:
            Xg, Ag = mr.geom_boxes(p["boxes"], x, x)
        S = None if norm[2] is None else norm[2](Xg.reshape(-1, 2)).reshape(Xg.shape[0], -1, 2, 2)
        d.h.set_residual_gram(gram_factors(2, p["ntx"], p["nty"], p["nax"], p["nay"], Ag, S, norm[1]))
    _against_reference("%s/%s/%s" % (shape, variant, mark), d, ref)
    assert mark in d.h.kernel_variant()


def test_generic_backend():
    from hp_vpinns_amd import _lib
    p, ref = _problem("B", "both+terms")
    d = Dev(p, backend=_lib.BACKEND_GENERIC)
    _against_reference("generic backend", d, ref)
    assert "k_mlp_fwd_generic" in d.h.kernel_variant()


# ---- the variant string, removal, lifecycle ---------------------------------------------------------------------------------------------------
def test_variant_names_the_term_exactly_when_a_bit_is_set():
    p, _ = _problem("B", "both")
    d = Dev(p, quasi=False)
    d.loss_and_grad()
    assert ";quasi" not in d.h.kernel_variant() and "k_project_lin<" in d.h.kernel_variant()
    one = np.zeros_like(d.qp)
    one[0], one[3] = 1.0, 1.0
    for planes, r, want in ((d.qp, d.qr, True), (one, 0.0, False), (one, -0.5, True), (d.qp, 0.0, True), (None, 0.0, False), (None, 0.7, False)):
        d.h.set_quasilinear(planes, r)
        d.loss_and_grad()
        v = d.h.kernel_variant()
        assert (";quasi" in v) == want and ("k_project_nl<" in v) == want, (r, want, v)
    # exponent 0: delta is neither checked nor read
    mu = d.qp.copy()
    d.h.set_quasilinear(mu, 0.0)
    a = d.everything()
    mu[3] = -7.0
    d.h.set_quasilinear(mu, 0.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, d.everything()))


@pytest.mark.parametrize("shape,variant", [("B", "both+terms"), ("A", "both"), ("D", "u")])
def test_removal_is_the_untouched_handle_bit_for_bit(shape, variant):
    p, _ = _problem(shape, variant)
    f = Dev(p, quasi=False)
    fresh = f.everything()
    f.h.step(20, False)
    fresh_th = f.params()
    one = np.zeros((4, p["X"].shape[0] * p["X"].shape[1]))
    one[0] = 1.0
    one[3] = -3.0                                     # (exponent 0: delta is not looked at)
    for how in ((None, 0.0), (one, 0.0)):
        d = Dev(p)
        with_term = d.everything()
        assert ";quasi" in d.h.kernel_variant() and not np.array_equal(with_term[0], fresh[0])
        d.h.set_quasilinear(*how)
        got = d.everything()
        v = d.h.kernel_variant()
        assert all(np.array_equal(x, y) for x, y in zip(got, fresh)), (shape, how[0] is None)
        assert ";quasi" not in v and v == f.h.kernel_variant()
        d.h.step(20, False)
        assert np.array_equal(d.params(), fresh_th)
        d.set_params(p["theta"])
        d.h.set_quasilinear(d.qp, d.qr)              # and back: the term's own bits again
        assert all(np.array_equal(x, y) for x, y in zip(d.everything(), with_term))


def test_two_identical_calls_give_identical_bits():
    p, _ = _problem("C", "both+terms")
    a, b = Dev(p), Dev(p)
    ea = a.everything()
    b.h.set_quasilinear(b.qp, b.qr)
    b.h.set_quasilinear(b.qp, b.qr)
    assert all(np.array_equal(x, y) for x, y in zip(ea, b.everything()))
    a.h.step(5, False)
    b.h.step(5, False)
    assert np.array_equal(a.params(), b.params())


def test_hard_bc_with_the_term():
    """u = G + D N on shape B: the ansatz is applied before mu, which sees the physical u and grad u"""
    p, ref = _problem("B", "both+terms", ansatz=True)
    d = Dev(p)
    _against_reference("B/both+terms/ansatz", d, ref)
    assert ";ansatz" in d.h.kernel_variant()
    plain = _problem("B", "both+terms")[1]
    assert abs(plain[0][0] - ref[0][0]) > 1e-3 * abs(ref[0][0])


def _f_phys(X):
    return np.sin(2.3 * X[..., 0] + 0.7) * np.cosh(0.8 * X[..., 1]) + 0.4


@pytest.mark.parametrize("shape", ["B", "D"])
@pytest.mark.parametrize("variant", ["both", "both+terms"])
def test_divergence_form_indicators(shape, variant):
    p, ref = _problem(shape, variant)
    f = _f_phys(p["X"])
    r = qr.strong(p, f)
    ind = qr.indicators(p, r, qr.terms(p))
    r1 = qr.strong(dict(p, q=dict(p["q"], use_u=False, use_grad=False)), f)
    assert np.abs(r - r1).max() > 1e-2 * np.abs(r).max()                     # the reference alone tells mu from 1
    d = Dev(p)
    d.strong_form_div()
    det = np.linalg.det(p["A"])
    fq = (f if p["boxes"] is not None else f * det).reshape(-1)
    got, rd = d.h.linear_indicators(fq, want_r=True)
    ec = np.array([rel(got[:, c], ind[:, c]) for c in range(5)])
    er = float(np.abs(rd.reshape(r.shape) - r).max() / np.abs(r).max())
    print("%s/%s divergence form | columns %s | r %.2e" % (shape, variant, np.array2string(ec, precision=2), er))
    WORST["div %s/%s" % (shape, variant)] = (float(ec.max()), er)
    assert ec.max() < TOL and er < TOL, (ec, er)
    again = d.h.linear_indicators(fq, want_r=True)
    assert np.array_equal(again[0], got) and np.array_equal(again[1], rd)
    l3, g, R = d.everything()                                                # the pass after it is the reference's still
    assert _rel3(l3, ref[0]).max() < TOL and gp.block_rel(g, ref[1], p["layers"]) < TOL


def test_refusals_leave_the_handle_usable():
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.quadrature import diff_matrix
    p, ref = _problem("B", "both+terms")
    d = Dev(p)

    def refused(call, code, message):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == code and message in str(e.value), (e.value.code, str(e.value))

    def usable():
        l3, g = d.loss_and_grad()
        assert _rel3(l3, ref[0]).max() < TOL and gp.block_rel(g, ref[1], p["layers"]) < TOL and ";quasi" in d.h.kernel_variant()
    bad = {}
    for name, row, v in (("m1", 1, np.nan), ("delta", 3, np.inf), ("delta", 3, 0.0), ("delta", 3, -1.0)):
        b = d.qp.copy()
        b[row, 5] = v
        bad[(name, v)] = b
    for call, msg in ((lambda: d.h.set_quasilinear(d.qp[:, :-1], d.qr), "expected 4 planes"), (lambda: d.h.set_quasilinear(d.qp[:3], d.qr), "expected 4 planes"),
                      (lambda: d.h.set_quasilinear(bad[("m1", np.nan)], d.qr), "plane m1 holds a non-finite value at point 5"),
                      (lambda: d.h.set_quasilinear(bad[("delta", np.inf)], d.qr), "plane delta holds a non-finite value at point 5"),
                      (lambda: d.h.set_quasilinear(d.qp, np.nan), "exponent"), (lambda: d.h.set_quasilinear(d.qp, np.inf), "exponent"),
                      (lambda: d.h.set_quasilinear(bad[("delta", 0.0)], d.qr), "delta = 0 at point 5"),
                      (lambda: d.h.set_quasilinear(bad[("delta", -1.0)], d.qr), "delta = -1 at point 5")):
        refused(call, -1, msg)
        usable()
    # the elementwise strong residual refuses while the term is set; the handle passes on
    d.h.set_strong_form(diff_matrix(p["xr"][0]), diff_matrix(p["yr"][0]))
    refused(lambda: d.h.linear_indicators(None), -3, "hpv_set_quasilinear")
    usable()
    d.h.set_strong_form(None, None)
    # hpv_set_trainable on a handle with the term
    refused(lambda: d.h.set_trainable(np.zeros((1, 10, d.qp.shape[1]))), -3, "hpv_set_quasilinear")
    usable()
    # new elements orphan the planes: the pass answers -3 and names the call, until they are set again or removed
    d.hand_elements()
    d.hand_planes(quasi=False)
    refused(lambda: d.h.loss_and_grad(True), -3, "hpv_set_quasilinear has not been called again")
    refused(lambda: d.h.step(1, False), -3, "hpv_set_quasilinear has not been called again")
    refused(lambda: d.h.set_trainable(np.zeros((1, 10, d.qp.shape[1]))), -3, "hpv_set_quasilinear")
    d.h.set_quasilinear(d.qp, d.qr)
    usable()
    d.hand_elements()
    d.hand_planes(quasi=False)
    d.h.set_quasilinear(None)
    l3, _ = d.loss_and_grad()
    fresh = Dev(p, quasi=False)
    assert np.array_equal(l3, fresh.loss_and_grad()[0]) and ";quasi" not in d.h.kernel_variant()
    d.h.set_quasilinear(d.qp, d.qr)
    usable()
    # before hpv_set_elements
    e = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, L2)
    refused(lambda: e.set_quasilinear(d.qp, d.qr), -3, "hpv_set_elements")
    # a handle with trainable coefficients
    t = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, L2, n_coef=1)
    refused(lambda: t.set_quasilinear(d.qp, d.qr), -3, "trainable coefficients")
    # a handle of another class
    o = _lib.Handle(_lib.PDE_POISSON2D, 1, _lib.ACT_TANH, [2, 20, 20, 20, 1])
    refused(lambda: o.set_quasilinear(d.qp, d.qr), -3, "linear problems")
    refused(lambda: o.set_quasilinear(None), -3, "linear problems")


# ---- the Python class ---------------------------------------------------------------------------------------------------------------------
def _model(diffusivity, **kw):
    from hp_vpinns_amd.vpinn import VPINNNonlinear
    gx, gy = np.array([-1.0, 0.3, 1.0]), np.array([-1.0, -0.2, 1.0])
    args = dict(grid_x=gx, grid_y=gy, n_quad=(5, 4), n_test=(3, 2), kappa=lambda P: np.stack([1.0 + 0.3 * P[:, 0], 1.5 - 0.2 * P[:, 1]], 1),
                beta=np.array([0.3, -0.2]), sigma=0.4, cubic=-0.5, f=lambda P: np.sin(P[:, 0]) + P[:, 1], diffusivity=diffusivity,
                X_u_train=np.array([[-1.0, 0.0], [1.0, 0.5], [0.2, -1.0]]), u_train=np.array([0.1, -0.2, 0.3]), lossb_weight=3.0,
                init_params=gp.generic_theta(L2, 9790))
    args.update(kw)
    return VPINNNonlinear(L2, **args)


def test_adam_under_graphs_and_a_live_change_of_the_term():
    """ten Adam steps, set_nonlinear(diffusivity=...) on the live model, ten more: one optimizer over both calls, against the
    reference's trajectory; a stale graph or a stale plane shows in the parameters and in the loss after the second call"""
    d1 = dict(poly=(1.0, lambda P: 0.3 * P[:, 0], 1.0), shift=lambda P: 1.0 + 0.2 * P[:, 1] ** 2, power=-0.5)
    d2 = dict(poly=(1.2, 0.0, 0.5), shift=0.7, power=0.5)
    m = _model(d1)
    p1 = qr.from_model(m)
    m.train(10)
    assert m.h.graphs_in_use() and ";quasi" in m.h.kernel_variant()
    th10 = qr.adam_trajectory(p1, 10)
    e10 = rel(m.get_params(), th10)
    m.set_nonlinear(diffusivity=d2)
    p2 = qr.from_model(m, p1["theta"])
    m.train(10)
    assert m.h.graphs_in_use() and ";quasi" in m.h.kernel_variant()
    th20 = qr.adam_trajectory(p1, 10, q=p1["q"], q2=p2["q"])
    l3 = np.asarray(m.loss())
    l3o, stale = qr.reference(p2, th20)[0], qr.reference(p1, th20)[0]
    e20, el = rel(m.get_params(), th20), _rel3(l3, l3o)
    print("ten Adam steps: parameters %.2e | ten more after a live change: parameters %.2e, loss %s" % (e10, e20, el))
    WORST["adam 10 / 10 + 10"] = (float(e10), float(e20), float(el.max()))
    assert abs(l3o[0] - stale[0]) > 1e3 * STEP_TOL * abs(l3o[0])
    assert e10 < STEP_TOL and e20 < STEP_TOL and el.max() < STEP_TOL
    m.set_nonlinear(diffusivity={})                   # the defaults: mu == 1, the term leaves
    m.loss_and_grad()
    assert ";quasi" not in m.h.kernel_variant()


def test_class_divergence_form_and_adapt_keeps_the_parameters():
    m = _model(dict(poly=(1.0, 0.0, 1.0), shift=1.0, power=-0.5), strong_form="divergence", X_u_train=None, u_train=None)
    p = qr.from_model(m)
    f = m._f(p["X"].reshape(-1, 2)).reshape(p["X"].shape[:2])
    r = qr.strong(p, f)
    ind = qr.indicators(p, r)
    got, rd = m.element_indicators(), m.strong_residual_at_quad()
    assert rel(got[:, 1], ind[:, 1]) < TOL and np.abs(rd.reshape(r.shape) - r).max() < TOL * np.abs(r).max()
    th = m.get_params().copy()
    n0 = len(m._mesh)
    m.adapt()
    print("adapt: %d -> %d elements" % (n0, len(m._mesh)))
    assert np.array_equal(m.get_params(), th) and len(m._mesh) > n0
    m.loss_and_grad()                                 # (the planes were handed over again on the new mesh)
    assert ";quasi" in m.h.kernel_variant()


def test_class_refusals():
    with pytest.raises(ValueError, match="trainable"):
        _model(dict(poly=(1.0, 0.0, 1.0)), trainable=[dict(name="c", init=1.0, sigma=1.0)])
    with pytest.raises(ValueError, match="elementwise"):
        _model(dict(poly=(1.0, 0.0, 1.0)), strong_form="elementwise")
    with pytest.raises(ValueError, match="shift"):
        _model(dict(shift=lambda P: P[:, 0], power=-0.5))
    m = _model(dict(poly=(1.0, 0.0, 1.0)))
    l3 = np.asarray(m.loss())
    with pytest.raises(ValueError, match="shift"):
        m.set_nonlinear(diffusivity=dict(shift=0.0, power=0.5))
    assert np.array_equal(np.asarray(m.loss()), l3)    # refused before anything changed


def test_python_class_on_the_smallest_minimal_surface_setting():
    from hp_vpinns_amd.drivers import nonlinear as drv
    from hp_vpinns_amd.vpinn import VPINNNonlinear
    kw = dict(drv.SMALLEST_QUASI)
    s = drv.setup(kw.pop("problem"), **kw)
    m = VPINNNonlinear(s["layers"], LR=2e-3, seed=1234, **s["model"])
    p = qr.from_model(m)
    l3, g = m.loss_and_grad()
    l3o, go, _ = qr.reference(p)
    # (the whole gradient, not per block: Scherk's data are odd under (x, y) -> (y, x) with u -> -u and so is the initial network's
    #  error, which leaves the output bias a gradient of rounding size -- a block the per-block measure rightly calls ill-posed)
    e = (float(_rel3(l3, l3o).max()), float(rel(g, go)))
    v = m.h.kernel_variant()
    assert "k_project_nl<6x6/3x3;quasi>" in v, v
    assert max(e) < TOL, e
    m.train(200)
    his = np.asarray(m.loss_his)
    err = m.rel_l2_error(s["X_test"], s["u_test"])
    print("minimal surface, 200 steps: loss %.3e -> %.3e, relative L2 error %.3e | loss, gradient against the reference %s" % (his[0], his[-1], err, e))
    WORST["class"] = e
    assert his.size == 200 and np.all(np.isfinite(his)) and his[-1] < his[0] and np.isfinite(err)
    assert m.h.graphs_in_use() and np.all(np.isfinite(m.predict(s["X_test"][:5])))
    m.set_validation(s["X_test"], s["u_test"])
    assert np.isfinite(m.validate()["rel_l2"])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n| case | errors |")
    for k, e in WORST.items():
        print("| %s | %s |" % (k, " | ".join("%.1e" % x for x in e)))
