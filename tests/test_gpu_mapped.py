"""The full diffusion tensor and mapped elements (hpv_set_operator_tensor, hpv_set_element_points, the TENSOR instantiations of
k_project_lin / _nl / _id, adapt.MappedMesh, VPINNLinear) on the device against tests/mapped_reference.py (CPU, fp64, the residual in
PHYSICAL terms; tests/test_mapped_host.py proves it).  The measured errors are in profiles/mapped_elements.md.

Every case: loss_and_grad() -- loss triple, gradient per block (the trainable scalars are a block) --, the forward-only loss,
hpv_get_residuals (inactive entries exactly 0), four Adam steps through hpv_step, the kernel's name.  Bounds:
TOL = 1e-9 on the loss triple, the gradient per block, the forward-only pass and the residuals, STEP_TOL = 1e-8 on the parameters
after four Adam steps, both imported from tests/test_gpu_generic_point.py.  Shapes: 3 elements, rule 6 x 5, tests 4 x 3 with unequal
per-element counts, network [2, 6, 5, 1]; one case with a 17 x 16 rule (the point loops wrap the 256 threads).

The device inputs of the mapped cases come from the PRODUCT: adapt.MappedMesh.geometry and VPINNLinear._fold; the reference never
forms K_eff."""
import numpy as np
import pytest

import generic_point as gp
import linear_reference as lr
import mapped_reference as mr
from cases import rel
from test_gpu_generic_point import STEP_TOL, TOL
from test_mapped_host import COUNTS, POLAR, QUADS, TERMS

pytestmark = pytest.mark.gpu

L = [2, 6, 5, 1]
NT = (4, 3)
BOXES = np.asarray(lr.BOXES2[:3])
MASS = 0.5
WORST = {}
_CACHE = {}


def _dirs(rng, ne, nq, nl):
    """two directions: the first in kxy ONLY; the second in s (and, with the nonlinear terms, a3 and g)"""
    K = np.zeros((ne, nq, 2, 2))
    K[:, :, 0, 1] = mr._signed(rng, (ne, nq))
    d2 = dict(s=mr._signed(rng, (ne, nq)))
    if nl:
        d2.update(a3=mr._signed(rng, (ne, nq)), g=mr._signed(rng, (ne, nq, 2)))
    return [dict(K=K), d2]


def _case(geom, kernel, q=(6, 5), dual=False, shard=None, seed=0):
    """(p, reference at the initial parameters, the Adam trajectory's end), computed once and left unchanged"""
    key = (geom, kernel, q, dual, shard)
    if key not in _CACHE:
        rx, ry = lr.rule(q[0]), lr.rule(q[1])
        X, A = {"boxes": lambda: mr.geom_boxes(BOXES, rx[0], ry[0]), "quads": lambda: mr.geom_quads(QUADS, rx[0], ry[0]),
                "polar": lambda: mr.geom_polar(POLAR, rx[0], ry[0])}[geom]()
        rng = np.random.default_rng(7300 + seed + sum(map(ord, geom + kernel)))
        nq = q[0] * q[1]
        nl = kernel in ("nl", "id")
        coefs = mr.random_coefs(rng, 3, nq, TERMS if nl else ())
        dirs = _dirs(rng, 3, nq, nl) if kernel == "id" else []
        p = mr.problem(L, 7300 + seed, X, A, rx, ry, NT, coefs, counts=COUNTS, dirs=dirs, c0=[0.7, -0.4] if dirs else [], data=11, flux=7,
                       mass=MASS if dual else None, boxes=BOXES if geom == "boxes" else None, shard=shard)
        p["geom"] = geom
        _CACHE[key] = (p, mr.reference(p), mr.adam_trajectory(p, 4))
    return _CACHE[key]


def _product_inputs(p):
    """the points and the folded planes of the owned elements as the PRODUCT makes them: (X (n, 2, NQ) of all elements, A (owned))"""
    from hp_vpinns_amd.adapt import MappedMesh
    mesh = MappedMesh.from_quads(QUADS, *COUNTS) if p["geom"] == "quads" else MappedMesh(POLAR, *COUNTS, map=mr.polar_map)
    xi, yi = p["xr"][0], p["yr"][0]
    X = mesh.quad_points(xi, yi).reshape(len(mesh), -1, 2).transpose(0, 2, 1)
    return X, mesh.geometry(xi, yi, p["eb"], p["ee"])[1]


class Dev:
    """the C-ABI on problem dict `p`: boxes take the PHYSICAL planes (hpv_set_element_boxes), mapped elements the product's points and
    its folded planes (hpv_set_element_points); a narrow network is zero-padded onto its device width as the Python classes do"""

    def __init__(self, p, tensor=True, operator=True, trainable=True):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.init import n_params, pad_plan
        from hp_vpinns_amd.quadrature import gram_stacks
        from hp_vpinns_amd.testfcn import tables_1d
        from hp_vpinns_amd.vpinn import VPINNLinear
        self.p, nc = p, len(p["dirs"])
        plan = pad_plan(p["layers"], nc)
        self.dev_layers, self.idx = plan if plan is not None else (p["layers"], None)
        self.n_dev = n_params(self.dev_layers, nc)
        self.h = h = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, self.dev_layers, lr=1e-3, lossb_weight=p["lbw"], n_coef=nc)
        (xi, wx), (yi, wy) = p["xr"], p["yr"]
        eb, ee = p["eb"], p["ee"]
        n = (ee - eb) * xi.size * yi.size
        h.set_quadrature(xi, wx, yi, wy)
        h.set_tables(tables_1d(p["ntx"], xi), tables_1d(p["nty"], yi))
        if p["boxes"] is not None:
            h.set_element_boxes(p["boxes"], eb, ee)
            A = None
        else:
            X, A = _product_inputs(p)
            h.set_element_points(X, eb, ee)
        h.set_rhs(p["F"].reshape(-1))
        h.set_active_tests_2d(p["nax"], p["nay"])

        def planes(c, nl):
            z = dict(K=np.zeros((ee - eb, n // (ee - eb), 2, 2)), b=np.zeros((ee - eb, n // (ee - eb), 2)), s=np.zeros((ee - eb, n // (ee - eb))))
            z.update({k: v[eb:ee] for k, v in c.items()})
            K = z["K"].reshape(n, 2, 2) if tensor else np.stack([z["K"][..., 0, 0].reshape(n), z["K"][..., 1, 1].reshape(n)], 1)
            op = VPINNLinear._fold(A, tensor, K, (z["b"].reshape(n, 2), z["s"].reshape(n)))
            g = z["g"].reshape(n, 2) if "g" in z else np.zeros((n, 2))
            return op, VPINNLinear._fold(A, False, None, tuple(z[k].reshape(n) if k in z else np.zeros(n) for k in ("a2", "a3", "ae")) + (g,))
        self.op, self.nl = planes(p["coefs"], True)
        self.dirs = np.stack([np.concatenate(planes(d, True), 0) for d in p["dirs"]], 0) if nc else None
        if operator:
            (h.set_operator_tensor if tensor else h.set_operator)(self.op)
        if any(k in p["coefs"] for k in ("a2", "a3", "ae", "g")):
            h.set_nonlinear(self.nl)
        if nc and trainable and operator:
            h.set_trainable(self.dirs)
        if p["mass"] is not None:
            sx, sy = gram_stacks(p["ntx"]), gram_stacks(p["nty"])
            h.set_residual_norm(_lib.NORM_DUAL, p["mass"], sx[0], sx[1], sy[0], sy[1])
        h.set_data(*p["data"])
        h.set_flux_data(p["flux"]["X"], np.concatenate([p["flux"]["a"][:, None], p["flux"]["b"]], 1), p["flux"]["g"], mr.fr.W_F)
        self.set_params(mr.full0(p))

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
            assert np.all(g[pad] == 0.0)
            g = g[self.idx]
        return np.asarray(l3), g

    def residuals(self):
        p = self.p
        return self.h.residuals((p["ee"] - p["eb"]) * p["ntx"] * p["nty"]).reshape(-1, p["nty"], p["ntx"])


def _rel3(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def _against_reference(tag, d, ref, want=None):
    p = d.p
    l3o, go, Ro = ref
    l3m, gm = d.loss_and_grad()
    v = d.h.kernel_variant()
    lf = d.h.loss_and_grad(False)[0]
    Rm = d.residuals()
    e3, ef = _rel3(l3m, l3o), _rel3(lf, l3o)
    kb, eb = gp.worst_block(gm, go, p["layers"], len(p["dirs"]))
    eR = float(np.linalg.norm(Rm - Ro) / np.linalg.norm(Ro))
    print("%s | %s | loss3 %s | worst block %s %.2e (global %.2e) | forward-only %s | residuals %.2e" % (tag, v, e3, kb, eb, rel(gm, go), ef, eR))
    WORST[tag] = (float(e3.max()), float(eb), float(ef.max()), eR)
    if want:
        assert want in v and d.h.lib.hpv_pass_structure(d.h._h) == 0, (tag, v, want)
    assert e3.max() < TOL, (tag, v, "loss triple", l3m, l3o)
    assert eb < TOL, (tag, v, "gradient block", kb, eb)
    assert ef.max() < TOL, (tag, v, "forward-only pass", lf, l3o)
    assert eR < TOL, (tag, v, "residuals", eR)
    assert np.all(Rm[Ro == 0.0] == 0.0), (tag, "inactive residual entries are exactly 0")


def _variant(kernel, q, dual, nc=0):
    terms = ";u2,u3,exp,adv" if kernel in ("nl", "id") else ""
    return "k_project_%s<%dx%d/%dx%d%s;tensor%s%s>" % (kernel, q[0], q[1], NT[0], NT[1], terms, ";nc=%d" % nc if nc else "", ";dual" if dual else "")


def _full_check(tag, geom, kernel, q=(6, 5), dual=False):
    p, ref, th4 = _case(geom, kernel, q, dual)
    d = Dev(p)
    _against_reference(tag, d, ref, _variant(kernel, q, dual, len(p["dirs"])))
    d.set_params(mr.full0(p))
    d.h.step(4, False)
    e = rel(d.params(), th4)
    print("%s | four Adam steps: parameters %.2e" % (tag, e))
    WORST[tag + " adam"] = (float(e),)
    assert e < STEP_TOL, (tag, "parameters after four Adam steps", e)


@pytest.mark.parametrize("dual", [False, True], ids=["l2", "dual"])
@pytest.mark.parametrize("kernel", ["lin", "nl", "id"])
def test_tensor_operator_on_boxes(kernel, dual):
    """a non-symmetric K per point on three boxes of unequal size: k_project_lin, k_project_nl with all four terms, k_project_id with
    nc = 2 and one direction in kxy only; each also under the dual norm"""
    _full_check("boxes %s%s" % (kernel, " dual" if dual else ""), "boxes", kernel, dual=dual)


@pytest.mark.parametrize("kernel", ["lin", "nl", "id"])
def test_bilinear_quads_through_the_mapped_mesh(kernel):
    """three non-parallelogram quadrilaterals: the points of adapt.MappedMesh and the product's fold on the device, the physical
    residual on the CPU"""
    _full_check("quads %s" % kernel, "quads", kernel)


def test_rule_17x16_wraps_the_threads():
    _full_check("quads nl 17x16", "quads", "nl", q=(17, 16))


def test_polar_elements_lin():
    _full_check("polar lin", "polar", "lin")


def test_discrimination_the_reference_tells_quads_from_their_bounding_boxes():
    """a device that ignored the map -- the quads' bounding boxes with the same physical coefficients -- is another problem for the
    reference, by more than 1e3 * TOL"""
    p, ref, _ = _case("quads", "lin")
    bb = np.stack([QUADS[:, :, 0].min(1), QUADS[:, :, 0].max(1), QUADS[:, :, 1].min(1), QUADS[:, :, 1].max(1)], 1)
    Xb, Ab = mr.geom_boxes(bb, p["xr"][0], p["yr"][0])
    t = mr.terms(p, X=Xb, A=Ab)
    dl, dR = abs(t["lossv"] - ref[0][2]) / abs(ref[0][2]), rel(t["R"], ref[2])
    print("quads against their bounding boxes: lossv %.2e, residuals %.2e" % (dl, dR))
    assert dl > 1e3 * TOL and dR > 1e3 * TOL
    # ... and the unfolded planes on the mapped points (the fold forgotten) likewise
    t = mr.terms(p, A=mr.unit_geometry(p["X"]))
    assert abs(t["lossv"] - ref[0][2]) / abs(ref[0][2]) > 1e3 * TOL


def test_diagonal_tensor_agrees_with_the_diagonal_operator():
    """kxy = kyx = 0 through hpv_set_operator_tensor against hpv_set_operator on the same handle kind, within TOL (not bitwise: the
    contraction of the two extra products may differ)"""
    p, _, _ = _case("boxes", "nl")
    q = dict(p, coefs=dict(p["coefs"]))
    q["coefs"]["K"] = p["coefs"]["K"].copy()
    q["coefs"]["K"][..., 0, 1] = q["coefs"]["K"][..., 1, 0] = 0.0
    ref = mr.reference(q)
    dt, dd = Dev(q), Dev(q, tensor=False)
    _against_reference("diagonal K as a tensor", dt, ref, "k_project_nl<6x5/4x3;u2,u3,exp,adv;tensor>")
    _against_reference("diagonal K", dd, ref, "k_project_nl<6x5/4x3;u2,u3,exp,adv>")
    (l3t, gt), (l3d, gd) = dt.loss_and_grad(), dd.loss_and_grad()
    assert _rel3(l3t, l3d).max() < TOL and gp.block_rel(gt, gd, L) < TOL


def test_shard_owns_its_rows_and_its_share():
    """a handle owning elements [1, 3) of 3 returns exactly those residual rows and that share of lossv"""
    pf, reff, _ = _case("quads", "nl")
    ps, refs, _ = _case("quads", "nl", shard=(1, 3))
    assert np.array_equal(refs[2], reff[2][1:3])
    d = Dev(ps)
    _against_reference("quads nl shard [1,3)", d, refs, "k_project_nl<")
    full = Dev(pf)
    full.loss_and_grad()
    assert rel(d.residuals(), full.residuals()[1:3]) < TOL
    assert abs(d.loss_and_grad()[0][2] - mr.terms(pf)["loss_e"][1:3].sum()) < TOL * reff[0][2]


def test_two_passes_return_the_same_bytes():
    p, _, _ = _case("quads", "id")
    d = Dev(p)
    r = []
    for _ in range(2):
        l3, g = d.loss_and_grad()
        r.append((l3, g, d.residuals()))
    assert all(np.array_equal(x, y) for x, y in zip(*r))


def test_contracts():
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.quadrature import diff_matrix, gram_stacks
    p, ref, _ = _case("boxes", "id")
    d = Dev(p)
    h = d.h
    _against_reference("contracts: start", d, ref, "k_project_id<6x5/4x3;u2,u3,exp,adv;tensor;nc=2>")

    def refused(call, code=-1, usable=True):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == code, (e.value.code, str(e.value))
        if usable:
            l3, g = d.loss_and_grad()
            assert _rel3(l3, ref[0]).max() < TOL and gp.block_rel(g, ref[1], L, 2) < TOL
    bad = d.op.copy()
    bad[1, 3] = np.inf
    refused(lambda: h.set_operator_tensor(d.op[:, :-1]))
    refused(lambda: h.set_operator_tensor(d.op[:5]))
    refused(lambda: h.set_operator_tensor(bad))
    refused(lambda: h.set_operator_tensor(None))
    refused(lambda: h.set_trainable(d.dirs[:, :10]))                      # [5 + 5] on a tensor handle
    # the strong form and the indicators are refused while the operator is a tensor
    Dx, Dy = diff_matrix(p["xr"][0]), diff_matrix(p["yr"][0])
    refused(lambda: h.set_strong_form(Dx, Dy))
    refused(lambda: h.linear_indicators())
    # switching the kind invalidates the directions: -3 until they are set again; the diagonal names come back exactly
    diag = np.concatenate([d.op[[0, 3]], d.op[4:]], 0)
    h.set_operator(diag)
    refused(lambda: h.loss_and_grad(True), -3, usable=False)
    refused(lambda: h.set_trainable(d.dirs), -1, usable=False)            # [7 + 5] on a diagonal handle
    dd = np.concatenate([d.dirs[:, [0, 3]], d.dirs[:, 4:]], 1)
    h.set_trainable(dd)
    q = dict(p, coefs=dict(p["coefs"], K=p["coefs"]["K"] * np.eye(2)), dirs=[dict(dr, K=dr["K"] * np.eye(2)) if "K" in dr else dr for dr in p["dirs"]])
    refq = mr.reference(q)
    _against_reference("contracts: back on the diagonal kernels", d, refq)
    fresh = Dev(q, tensor=False)
    fresh.loss_and_grad()
    d.loss_and_grad()
    assert d.h.kernel_variant() == fresh.h.kernel_variant() and "tensor" not in d.h.kernel_variant() and "k_project_id<6x5/4x3;u2,u3,exp,adv;nc=2>" in d.h.kernel_variant()
    (l3a, ga), (l3b, gb) = d.loss_and_grad(), fresh.loss_and_grad()
    assert _rel3(l3a, l3b).max() < TOL and gp.block_rel(ga, gb, L, 2) < TOL
    h.set_strong_form(Dx, Dy)                                             # (allowed again)
    h.set_strong_form(None, None)
    h.set_operator_tensor(d.op)
    refused(lambda: h.loss_and_grad(True), -3, usable=False)
    h.set_trainable(d.dirs)
    _against_reference("contracts: tensor again", d, ref, ";tensor;nc=2>")
    # hpv_set_element_points: kinds of handles, preconditions, the dual norm and the strong form
    X = mr.geom_quads(QUADS, p["xr"][0], p["yr"][0])[0].transpose(0, 2, 1)
    Xn = X.copy()
    Xn[2, 1, 4] = np.nan
    refused(lambda: h.set_element_points(Xn))
    refused(lambda: h.set_element_points(X, 2, 1))
    refused(lambda: h.set_element_points(X, 0, 4))
    sx, sy = gram_stacks(NT[0]), gram_stacks(NT[1])
    h.set_residual_norm(_lib.NORM_DUAL, MASS, sx[0], sx[1], sy[0], sy[1])
    refused(lambda: h.set_element_points(X), usable=False)
    h.set_residual_norm(_lib.NORM_L2)
    _against_reference("contracts: after the refusals", d, ref)
    h.set_element_points(X)
    refused(lambda: h.loss_and_grad(True), -3, usable=False)              # new elements orphan every plane
    refused(lambda: h.set_residual_norm(_lib.NORM_DUAL, MASS, sx[0], sx[1], sy[0], sy[1]), usable=False)
    refused(lambda: h.set_strong_form(Dx, Dy), usable=False)
    f = np.arange(3 * 30, dtype=np.float64) / 7.0 + 1.0
    from hp_vpinns_amd.testfcn import tables_1d
    ax, ay = tables_1d(NT[0], p["xr"][0])[0] * p["xr"][1][None, :], tables_1d(NT[1], p["yr"][0])[0] * p["yr"][1][None, :]
    Fa = h.assemble_rhs(f, 3 * 12).reshape(3, 3, 4)
    assert rel(Fa, np.einsum("kj,ri,eji->ekr", ay, ax, f.reshape(3, 5, 6))) < 1e-13      # J = 1: sum_q w f phi phi
    h.set_element_boxes(BOXES)                                            # ... and back to boxes
    h.set_operator_tensor(d.op)
    h.set_nonlinear(d.nl)
    h.set_trainable(d.dirs)
    _against_reference("contracts: boxes again", d, ref)
    # other kinds of handles
    h1 = _lib.Handle(_lib.PDE_LINEAR1D, 1, _lib.ACT_SIN, [1, 8, 8, 1])
    for call in (lambda: h1.set_operator_tensor(np.ones((7, 4))), lambda: h1.set_element_points(np.ones((1, 2, 4)))):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == -1
    h2 = _lib.Handle(_lib.PDE_POISSON2D, 1, _lib.ACT_TANH, [2, 8, 8, 1])
    for call in (lambda: h2.set_operator_tensor(np.ones((7, 4))), lambda: h2.set_element_points(np.ones((1, 2, 4)))):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == -1


# ---- the Python classes -----------------------------------------------------------------------------------------------------------------
def _model_problem(m, theta=None):
    """the physical problem dict of a live VPINNLinear on a polar MappedMesh (one rank): geometry restated by mapped_reference, the
    model's coefficient callables evaluated at the physical points, F = sum_q w d f phi phi by numpy"""
    from hp_vpinns_amd.testfcn import tables_1d
    from hp_vpinns_amd.vpinn import _coef_field, _kappa_field
    mesh = m._mesh
    rx, ry = m._rule
    X, A = mr.geom_polar(mesh.boxes, rx[0], ry[0])
    ne, nq = X.shape[0], X.shape[1]
    P = X.reshape(-1, 2)
    k = _kappa_field(m._op["kappa"], P, 2)
    K = k.reshape(ne, nq, 2, 2) if k.ndim == 3 else (k[:, :, None] * np.eye(2)).reshape(ne, nq, 2, 2)
    coefs = dict(K=K, b=_coef_field(m._op["beta"], P, 2, "beta", True).reshape(ne, nq, 2), s=_coef_field(m._op["sigma"], P, 2, "sigma", False).reshape(ne, nq))
    ntx, nty = int(mesh.nax.max()), int(mesh.nay.max())
    p = mr.problem(m.layers, 0, X, A, rx, ry, (ntx, nty), coefs, counts=(mesh.nax, mesh.nay))
    f = _coef_field(m._f, P, 2, "f", False).reshape(ne, ry[0].size, rx[0].size)
    ax, ay = tables_1d(ntx, rx[0])[0] * rx[1][None, :], tables_1d(nty, ry[0])[0] * ry[1][None, :]
    p["F"] = np.einsum("kj,ri,eji->ekr", ay, ax, np.linalg.det(A).reshape(f.shape) * f)
    p.update(theta=m.get_params() if theta is None else np.asarray(theta, dtype=np.float64), lbw=float(m.lossb_weight), ansatz=m._hard_bc,
             data=None if m.X_u_train is None else (m.X_u_train, m.utrain))
    if m._flux is not None:
        Xf, cf, g, w = m._flux
        assert w == mr.fr.W_F
        p["flux"] = dict(X=np.asarray(Xf), a=np.asarray(cf)[:, 0], b=np.asarray(cf)[:, 1:], g=np.asarray(g))
    return p


def test_polar_elements_with_hard_bc_data_and_flux_and_the_class_surface(tmp_path):
    """VPINNLinear on polar elements with an ansatz, Dirichlet data and a flux term together, a tensor kappa on top of the map;
    set_mesh box -> mapped -> box on the live model with the state untouched; the refusals of the class"""
    from hp_vpinns_amd.adapt import ElementMesh, MappedMesh
    from hp_vpinns_amd.drivers import linear
    from hp_vpinns_amd.vpinn import VPINNLinear
    rng = np.random.default_rng(7400)
    mesh = MappedMesh(POLAR, *COUNTS, map=mr.polar_map)
    Kc = np.array([[1.3, 0.4], [-0.7, 0.9]])
    Xd = mr.polar_map(np.stack([rng.uniform(1, 2, 11), rng.uniform(0, np.pi / 2, 11)], 1))[0]
    kw = dict(n_quad=(6, 5), kappa=lambda P: Kc[None] * (1.0 + 0.3 * P[:, 0] * P[:, 1])[:, None, None], beta=np.array([0.5, -1.1]),
              sigma=lambda P: 1.0 + P[:, 0], f=linear._annulus_f, X_u_train=Xd, u_train=rng.uniform(-1, 1, 11), lossb_weight=mr.LBW,
              init_params=gp.generic_theta(L, 7400))
    m = VPINNLinear(L, mesh=mesh, hard_bc=linear.annulus_hard_bc(), **kw)
    Xf = mr.polar_map(np.stack([rng.uniform(1, 2, 7), rng.uniform(0, np.pi / 2, 7)], 1))[0]
    m.set_flux_data(Xf, g=rng.uniform(-1, 1, 7), a=mr._signed(rng, 7), b=mr._signed(rng, (7, 2)), weight=mr.fr.W_F)
    p = _model_problem(m)
    l3, g = m.loss_and_grad()
    l3o, go, _ = mr.reference(p)
    e3, (kb, eb) = _rel3(l3, l3o), gp.worst_block(g, go, L, 0)
    print("polar, hard_bc + data + flux | %s | loss3 %s | worst block %s %.2e" % (m.h.kernel_variant(), e3, kb, eb))
    WORST["polar class"] = (float(e3.max()), float(eb))
    assert "k_project_lin<6x5/4x3;tensor;ansatz>" in m.h.kernel_variant()
    assert e3.max() < TOL and eb < TOL
    m.train(4)
    e = rel(m.get_params(), mr.adam_trajectory(p, 4))
    WORST["polar class adam"] = (float(e),)
    assert e < STEP_TOL
    # predict applies the ansatz: zero on the inner arc
    assert np.all(m.predict(np.array([[1.0, 0.0], [0.0, 1.0]])) == 0.0)
    # checkpoints
    m.save_checkpoint(tmp_path / "ck")
    st = m.h.get_state()
    m.train(2)
    m.load_checkpoint(tmp_path / "ck")
    assert np.array_equal(m.h.get_state(), st)
    # refusals of the class, each a ValueError that says why
    for bad, word in ((dict(residual_norm="dual"), "dual"), (dict(strong_form="elementwise"), "strong")):
        with pytest.raises(ValueError, match=word):
            VPINNLinear(L, mesh=mesh, **kw, **bad)
    with pytest.raises(ValueError, match="u_xy"):
        VPINNLinear(L, grid_x=[-1, 0, 1], grid_y=[-1, 1], n_quad=(6, 5), n_test=(4, 3), kappa=Kc, strong_form="elementwise")
    for call in (lambda: m.set_residual_norm("dual"), m.adapt, lambda: m.train_adaptive(4, 2)):
        with pytest.raises(ValueError):
            call()
    l3b = m.loss()
    assert np.all(np.isfinite(l3b))
    # box -> mapped -> box on a live model: the state is untouched, the kernels follow
    b = VPINNLinear(L, mesh=ElementMesh(BOXES, *COUNTS), n_quad=(6, 5), kappa=1.0, f=1.0, init_params=gp.generic_theta(L, 7401))
    b.train(3)
    lb, vb, st = b.loss(), b.h.kernel_variant(), b.h.get_state()
    assert "tensor" not in vb
    b.set_mesh(MappedMesh.from_quads(QUADS, *COUNTS))
    assert np.array_equal(b.h.get_state(), st)
    b.loss_and_grad()                                   # (the name is that of the last pass with a gradient)
    assert "k_project_lin<6x5/4x3;tensor>" in b.h.kernel_variant()
    b.set_mesh(ElementMesh(BOXES, *COUNTS))
    assert np.array_equal(b.h.get_state(), st)
    b.loss_and_grad()
    assert np.array_equal(b.loss(), lb) and b.h.kernel_variant() == vb


def test_annulus_driver_trains():
    """The annulus driver at its smallest setting ([2, 8, 8, 1], 4 polar elements) against the CPU reference's own Adam trajectory on the
    same problem for the same number of steps.  Bound, as tests/test_gpu_linear.py: the reference trajectory's relative L2 error
    times 2 -- the two trajectories separate within STEP_TOL per step."""
    import validation_reference as vr
    from hp_vpinns_amd.drivers import linear
    out = linear.run_annulus(**linear.ANNULUS_SMALLEST, verbose=False)
    m = out["model"]
    assert "k_project_lin<8x8/4x4;tensor>" in m.h.kernel_variant() and m.h.graphs_in_use()
    p = _model_problem(m, m._init_params)
    th = mr.adam_trajectory(p, linear.ANNULUS_SMALLEST["n_iter"], lr_=m.LR)
    X, u = out["X_test"], out["u_test"]
    ur = vr.bare_oracle("p2", p["layers"], th)._predict(X)
    e_ref = float(np.linalg.norm(ur.reshape(-1) - u.reshape(-1)) / np.linalg.norm(u))
    line = "annulus, %d steps: relative L2 error %.4e on the device, %.4e on the CPU reference's trajectory (parameters %.2e)" % (
        linear.ANNULUS_SMALLEST["n_iter"], out["rel_l2"], e_ref, rel(m.get_params(), th))
    print(line)
    WORST["annulus driver"] = (out["rel_l2"], e_ref)
    assert out["rel_l2"] < 2 * e_ref


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n| case | loss triple | gradient block | forward-only | residuals |")
    for k, e in WORST.items():
        print("| %s | %s |" % (k, " | ".join("%.1e" % x for x in e)))
