"""The dual-norm residual loss through dense Gram factors (hpv_set_residual_gram; k_project_lin_dense, k_project_nl_dense,
k_project_id<.., 2> and their TENSOR siblings: csrc/hpv_dual_dense.h) on the device against the dense-solve reference of
tests/dualdense_reference.py.  tests/test_dualdense_host.py proves every box case on the CPU; profiles/dual_norm_dense.md holds the
measured figures.

Boxes (the machinery of tests/test_gpu_dualnorm.py, non-TENSOR kernels, an energy product with a 2 x 2 SPD field S(x)): the shapes at
which the dense path can go wrong -- NR = 33 in 1-D, 10 x 7 functions (more rows than lanes, NR no multiple of 4), one function,
per-element counts down to 1 x 2 (inactive rows inside the triangle), a shard [1, 3) (the offset into W), y appended behind `red`
(5 x 4 functions on 3 x 2 points), boxes of aspect ratio 24; lin, nl and id (nc = 2); one case under the generic ansatz.
Quadrilaterals (tests/test_gpu_mapped.py's, TENSOR kernels, the physical H^1 product): lin, nl, id, and a shard.
Bounds: TOL = 1e-9 device against reference on the loss triple, the gradient per block, the forward-only pass and
the residuals; STEP_TOL = 1e-8 on the parameters after Adam steps."""
import numpy as np
import pytest

import dualdense_reference as dd
import generic_point as gp
import linop_sweep as ls
import mapped_reference as mr
import test_gpu_mapped as tm
from cases import rel
from test_gpu_ansatz import _against_reference, _rel3
from test_gpu_dualnorm import DualDev, _code, _model_problem
from test_gpu_generic_point import STEP_TOL, TOL
from test_gpu_linop_sweep import _mask
from test_mapped_host import COUNTS, QUADS

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in dd.cases()}
_PROBLEMS = {}
MASS_Q = 0.5


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _problem(name):
    """the case's arrays, its dense-solve reference (loss triple, gradient, R) and the product's factors, computed once"""
    if name not in _PROBLEMS:
        p = dd.problem(CASES[name])
        _PROBLEMS[name] = (p, dd.reference(p), dd.box_factors(p))
    return _PROBLEMS[name]


def _dense_dev(p, W, **kw):
    d = DualDev(p, dual=False, **kw)
    d.h.set_residual_gram(W)
    return d


KERNEL = {"lin": "k_project_lin<", "nl": "k_project_nl<", "id": "k_project_id<"}


@pytest.mark.parametrize("name", list(CASES))
def test_box_case_against_the_dense_solve_reference(name):
    c = CASES[name]
    p, ref, W = _problem(name)
    _, qx, qy, ntx, nty = ls.shape(c)
    appended = ntx * nty > 3 * qy * (qx | 1)
    assert appended == (c["row"] == "append")
    d = _dense_dev(p, W)
    first = d.loss_and_grad()
    v = _against_reference(name, d, ref, validation=d.has_val)
    assert "%s%dx%d/%dx%d" % (KERNEL[c["variant"]], qx, qy, ntx, nty) in v and v.count(";dual=dense>") == 1 and ";tensor" not in v, v
    assert (";ansatz;dual=dense>" in v) == (p["ans"] is not None) and d.h.lib.hpv_pass_structure(d.h._h) == 0, v
    Ro = ref[2]
    Rm = d.h.residuals(Ro.size).reshape(Ro.shape)
    eR = float(np.linalg.norm(Rm - Ro) / np.linalg.norm(Ro))
    m = _mask(p)
    print("%s | y %s | residuals %.2e | loss %.2e | block %.2e" % (name, "appended" if appended else "aliased", eR,
          float(_rel3(first[0], ref[0]).max()), float(gp.worst_block(first[1], ref[1], p["layers"], d.nc)[1])))
    assert eR < TOL, (name, "residuals", eR)
    assert np.all(Rm[~m] == 0.0), (name, "masked residual entries are exactly 0")
    again = d.loss_and_grad()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), (name, "a second pass differs from the first")


# ---- quadrilaterals ----------------------------------------------------------------------------------------------------------------------
_QUAD = {}


def _quad_factors(eb, ee, mass):
    from hp_vpinns_amd.adapt import MappedMesh
    from hp_vpinns_amd.quadrature import gram_factors, gram_rule
    mesh = MappedMesh.from_quads(QUADS, *COUNTS)
    x = gram_rule(*tm.NT)[0]
    A = mesh.geometry(x, x, eb, ee)[1].reshape(ee - eb, x.size ** 2, 2, 2)
    return gram_factors(2, tm.NT[0], tm.NT[1], mesh.nax[eb:ee], mesh.nay[eb:ee], A, None, mass, first=eb)


def _quad_case(kernel, shard=None):
    """(p with the mass set, the reference's terms under the physical H^1 product, the product's factors)"""
    key = (kernel, shard)
    if key not in _QUAD:
        p = dict(tm._case("quads", kernel, shard=shard)[0], mass=MASS_Q)
        _QUAD[key] = (p, dd.mapped_terms(p, QUADS), _quad_factors(p["eb"], p["ee"], MASS_Q))
    return _QUAD[key]


def _quad_dev(p, W):
    d = tm.Dev(dict(p, mass=None))                       # (no tables: kind 1 is refused on mapped elements)
    d.h.set_residual_gram(W)
    return d


@pytest.mark.parametrize("kernel", ["lin", "nl", "id"])
def test_quadrilaterals_in_the_physical_metric(kernel):
    p, t, W = _quad_case(kernel)
    d = _quad_dev(p, W)
    nc = len(p["dirs"])
    terms = ";u2,u3,exp,adv" if kernel in ("nl", "id") else ""
    want = "k_project_%s<6x5/4x3%s;tensor%s;dual=dense>" % (kernel, terms, ";nc=%d" % nc if nc else "")
    tm._against_reference("quads %s dense" % kernel, d, (t["triple"], t["grad"], t["R"]), want)
    a, b = d.loss_and_grad(), d.loss_and_grad()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_quadrilateral_shards_add_up():
    """elements [1, 3) of 3: those rows of W, that share of lossv; with [0, 1) the whole"""
    pf, tf, Wf = _quad_case("nl")
    ps, ts, Ws = _quad_case("nl", shard=(1, 3))
    assert np.array_equal(Ws, Wf[1:3])
    d = _quad_dev(ps, Ws)
    tm._against_reference("quads nl dense shard [1,3)", d, (ts["triple"], ts["grad"], ts["R"]), ";dual=dense>")
    p0 = dict(pf, eb=0, ee=1)
    d0 = _quad_dev(p0, Wf[:1])
    whole = _quad_dev(pf, Wf)
    lv = [x.loss_and_grad()[0][2] for x in (d0, d, whole)]
    assert abs(lv[0] + lv[1] - lv[2]) < TOL * abs(lv[2]) and abs(lv[1] - tf["loss_e"][1:3].sum()) < TOL * abs(lv[2])


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------
def test_eight_adam_steps():
    p, ref, W = _problem("counts-nl")
    d = _dense_dev(p, W)
    d.h.step(8, False)
    e = float(rel(d.params(), dd.adam_trajectory(p, 8)))
    print("boxes, counts-nl: eight Adam steps, parameters %.2e" % e)
    assert e < STEP_TOL
    pq, _, Wq = _quad_case("lin")
    dq = _quad_dev(pq, Wq)
    dq.h.step(8, False)
    e = float(rel(dq.params(), dd.mapped_adam(pq, QUADS, 8)))
    print("quads lin: eight Adam steps, parameters %.2e" % e)
    assert e < STEP_TOL


# ---- kind 0, indicators, lifecycle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["lin", "nl", "id"])
def test_kind_zero_restores_the_plain_handle_bit_for_bit(variant):
    from hp_vpinns_amd import _lib
    p, _, W = _problem("counts-" + variant)
    plain = DualDev(p, dual=False)
    l0, g0 = plain.loss_and_grad()
    R0 = plain.h.residuals(W.shape[0] * W.shape[1])
    assert ";dual" not in plain.h.kernel_variant()
    d = _dense_dev(p, W)
    ld, _ = d.loss_and_grad()
    assert ";dual=dense>" in d.h.kernel_variant() and not np.array_equal(ld, l0)
    d.h.set_residual_norm(_lib.NORM_L2)
    l1, g1 = d.loss_and_grad()
    assert d.h.kernel_variant() == plain.h.kernel_variant()
    assert l1.tobytes() == l0.tobytes() and g1.tobytes() == g0.tobytes() and d.h.residuals(R0.size).tobytes() == R0.tobytes()
    assert np.asarray(plain.h.loss_and_grad(False)[0]).tobytes() == np.asarray(d.h.loss_and_grad(False)[0]).tobytes()


def test_indicators_column_zero_is_the_dense_dual_loss():
    from hp_vpinns_amd.quadrature import diff_matrix
    p, ref, W = _problem("counts-lin")
    d = _dense_dev(p, W, validation=False)
    d.h.set_strong_form(diff_matrix(p["xr"][0]), diff_matrix(p["yr"][0]))
    ind = d.h.linear_indicators(None)
    le = dd.loss_e(dd.grams(p, dd.S_of(p)), p, ref[2])[0]
    e = float(np.abs(ind[:, 0] - le).max() / np.abs(le).max())
    print("indicators, column 0 against the reference's per-element dense dual loss: %.2e" % e)
    assert e < TOL


def test_lifecycle():
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.quadrature import gram_stacks
    from hp_vpinns_amd.testfcn import tables_1d
    p, ref, W = _problem("counts-lin")
    d = _dense_dev(p, W)
    _against_reference("counts-lin", d, ref)
    NR = p["ntx"] * p["nty"]
    nax, nay = dd._counts(p)
    assert (nax[1], nay[1]) == (1, 2)                    # element 1 keeps the full indices 0 and ntx only

    def bad(e, i, j, v):
        B = W.copy()
        B[e, i, j] = v
        return B
    refused = [("wrong n", lambda: d.h.set_residual_gram(W[:2])), ("NULL", lambda: d.h.set_residual_gram(None)),
               ("non-finite", lambda: d.h.set_residual_gram(bad(0, 3, 1, np.nan))),
               ("above the diagonal", lambda: d.h.set_residual_gram(bad(0, 1, 3, 0.5))),
               ("an inactive row", lambda: d.h.set_residual_gram(bad(1, 1, 0, 0.5))),
               ("an inactive column", lambda: d.h.set_residual_gram(bad(1, p["ntx"], 1, 0.5))),
               ("a diagonal entry <= 0", lambda: d.h.set_residual_gram(bad(2, 0, 0, 0.0)))]
    for what, call in refused:
        code, msg = _code(call)
        assert code == -1, (what, code, msg)
        l3, _ = d.loss_and_grad()                        # the handle keeps what it had
        assert _rel3(l3, ref[0]).max() < TOL and ";dual=dense>" in d.h.kernel_variant(), what
    # the factors belong to the tables, the elements and the counts: each drops them, and a pass refuses until they are given again
    drops = [("hpv_set_tables", lambda: d.h.set_tables(tables_1d(p["ntx"], p["xr"][0]), tables_1d(p["nty"], p["yr"][0])), False),
             ("hpv_set_element_boxes", lambda: d.h.set_element_boxes(p["boxes"], p["eb"], p["ee"]), True),
             ("hpv_set_active_tests_2d", lambda: d.h.set_active_tests_2d(p["nax"], p["nay"]), False)]
    for what, call, planes in drops:
        call()
        if planes:                                       # (new elements orphan the planes too: hand them over again first)
            d.set_planes()
        code, msg = _code(d.loss_and_grad)
        assert code == -3 and "hpv_set_residual_gram" in msg, (what, code, msg)
        assert _code(lambda: d.h.loss_and_grad(False))[0] == -3
        d.h.set_residual_gram(W)
        l3, _ = d.loss_and_grad()
        assert _rel3(l3, ref[0]).max() < TOL, what
    # kind 1 replaces kind 2 and the other way round
    sx, sy = gram_stacks(p["ntx"]), gram_stacks(p["nty"])
    d.h.set_residual_norm(_lib.NORM_DUAL, 0.0, sx[0], sx[1], sy[0], sy[1])
    d.loss_and_grad()
    assert d.h.kernel_variant().endswith(";dual>") or ";dual>" in d.h.kernel_variant()
    d.h.set_residual_gram(W)
    l3, _ = d.loss_and_grad()
    assert _rel3(l3, ref[0]).max() < TOL and ";dual=dense>" in d.h.kernel_variant()
    # another class; before the tables and elements
    other = _lib.Handle(_lib.PDE_POISSON2D, 1, _lib.ACT_TANH, [2, 20, 20, 20, 1])
    code, msg = _code(lambda: other.set_residual_gram(W))
    assert code == -3 and "linear problems" in msg, (code, msg)
    fresh = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, [2, 8, 8, 1])
    code, msg = _code(lambda: fresh.set_residual_gram(W))
    assert code == -3 and "hpv_set_tables" in msg, (code, msg)


def test_mapped_handle_lifecycle():
    """on mapped elements kind 1 stays refused; under kind 2 hpv_set_element_points is accepted and marks the factors stale"""
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.quadrature import gram_stacks
    p, t, W = _quad_case("lin")
    d = _quad_dev(p, W)
    sx, sy = gram_stacks(tm.NT[0]), gram_stacks(tm.NT[1])
    code, msg = _code(lambda: d.h.set_residual_norm(_lib.NORM_DUAL, 0.0, sx[0], sx[1], sy[0], sy[1]))
    assert code == -1 and "mapped" in msg, (code, msg)
    l3, _ = d.loss_and_grad()
    assert _rel3(l3, t["triple"]).max() < TOL
    X, _ = tm._product_inputs(p)
    d.h.set_element_points(X, p["eb"], p["ee"])
    d.h.set_operator_tensor(d.op)
    code, msg = _code(d.loss_and_grad)
    assert code == -3 and "hpv_set_residual_gram" in msg, (code, msg)
    d.h.set_residual_gram(W)
    l3, _ = d.loss_and_grad()
    assert _rel3(l3, t["triple"]).max() < TOL


def test_y_past_the_lds_limit_is_refused():
    """3 x 3 points with 60 x 60 functions: hpv_set_tables admits it (39 200 B); with the 3 600 doubles of y appended it is past 64 KiB"""
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.testfcn import tables_1d
    import linear_reference as lr
    h = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, [2, 8, 8, 1])
    (xi, wx) = lr.rule(3)
    h.set_quadrature(xi, wx, xi, wx)
    h.set_tables(tables_1d(60, xi), tables_1d(60, xi))
    h.set_element_boxes(np.array([[-1.0, 1.0, -1.0, 1.0]]), 0, 1)
    code, msg = _code(lambda: h.set_residual_gram(np.zeros(4)))
    assert code == -1 and "LDS" in msg, (code, msg)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def _annulus(n=2):
    from hp_vpinns_amd.adapt import MappedMesh
    r, t = np.linspace(1.0, 2.0, n + 1), np.linspace(0.0, np.pi / 2, n + 1)
    boxes = np.array([[r[i], r[i + 1], t[j], t[j + 1]] for i in range(n) for j in range(n)])
    return MappedMesh(boxes, 4, 4, map=mr.polar_map)


def _f(P):
    return -2.0 * np.pi ** 2 * np.sin(np.pi * P[:, 0]) * np.sin(np.pi * P[:, 1])


def _kappa(P):
    return dd.S_energy(P)


def _variant(m):
    """the kernels of a reverse-mode pass of the model (a forward-only pass leaves the name alone)"""
    m.loss_and_grad()
    return m.h.kernel_variant()


def _model(**kw):
    from hp_vpinns_amd.vpinn import VPINNLinear
    t = np.linspace(-1.0, 1.0, 9)
    Xb = np.concatenate([np.stack([t, -np.ones(9)], 1), np.stack([t, np.ones(9)], 1), np.stack([-np.ones(9), t], 1), np.stack([np.ones(9), t], 1)])
    kw.setdefault("grid_x", np.array([-1.0, 0.1, 1.0]))
    kw.setdefault("grid_y", np.array([-1.0, 0.1, 1.0]))
    if "mesh" in kw:
        kw.pop("grid_x"), kw.pop("grid_y")
    return VPINNLinear([2, 8, 8, 1], n_quad=6, n_test=4, f=_f, X_u_train=Xb, u_train=np.zeros(36), lossb_weight=3.0, seed=7, **kw)


def test_training_on_a_quarter_annulus_in_the_physical_metric():
    m = _model(mesh=_annulus(), residual_norm=dict(kind="dual", metric="physical"))
    assert m.residual_norm == dict(kind="dual", mass=0.0, metric="physical", gram_points=None)
    m.train(50)
    his = np.asarray(m.loss_his)
    assert ";dual=dense>" in m.h.kernel_variant() and ";tensor" in m.h.kernel_variant()
    assert his.size == 50 and np.all(np.isfinite(his)) and his[-1] < his[0], (his[0], his[-1])


def _energy_reference(m, mass=0.0):
    """the model's box problem under the energy product of dd.S_energy (dualnorm_reference's route with the dense Gram matrices)"""
    p = _model_problem(m, mass)
    p["metric"] = "energy"
    return dd.reference(p)


def test_metrics_on_a_live_model_and_set_operator():
    from hp_vpinns_amd.vpinn import VPINNLinear
    m = _model(kappa=np.array([2.0, 0.5]))               # a diagonal kappa: the non-TENSOR kernels
    m.set_params(gp.generic_theta([2, 8, 8, 1], 14931))
    l2 = m.loss()
    m.set_residual_norm("dual")
    lr_ = m.loss()
    assert ";dual>" in _variant(m)
    m.set_residual_norm(dict(kind="dual", metric="physical"))      # on boxes the inner product of "reference": the tables, the same bits
    assert np.asarray(m.loss()).tobytes() == np.asarray(lr_).tobytes() and ";dual>" in _variant(m)
    m.set_residual_norm(dict(kind="dual", metric="energy"))
    le = m.loss()
    assert ";dual=dense>" in _variant(m) and not np.array_equal(np.asarray(le), np.asarray(lr_))
    # kappa = diag(2, 0.5): G_e is assembled from it; against the reference with S = that constant
    p = _model_problem(m, 0.0)
    Gs = dd.grams(p, lambda P: np.tile(np.diag([2.0, 0.5]), (P.shape[0], 1, 1)))
    with dd._dense(Gs, p):
        ref = dd.dn.reference(p)
    assert _rel3(le, ref[0]).max() < TOL, (le, ref[0])
    # set_operator(kappa=) re-hands the factors: the full SPD field of the reference, now through the TENSOR kernels
    m.set_operator(kappa=_kappa)
    l3 = m.loss()
    assert ";tensor" in _variant(m) and ";dual=dense>" in _variant(m)
    p = _model_problem_tensor(m)
    assert _rel3(l3, p).max() < TOL, (l3, p)
    with pytest.raises(ValueError, match="positive definite"):
        m.set_operator(kappa=np.array([[1.0, 2.0], [2.0, 1.0]]))
    assert np.asarray(m.loss()).tobytes() == np.asarray(l3).tobytes()      # refused before anything changed
    with pytest.raises(ValueError, match="trainable kappa"):
        VPINNLinear([2, 8, 8, 1], grid_x=np.array([-1.0, 1.0]), grid_y=np.array([-1.0, 1.0]), n_quad=6, n_test=4,
                    trainable=[dict(name="k", init=1.0, kappa=1.0)], residual_norm=dict(kind="dual", metric="energy"))
    m.set_residual_norm("l2")
    m.set_operator(kappa=np.array([2.0, 0.5]))
    assert np.asarray(m.loss()).tobytes() == np.asarray(l2).tobytes()


def _model_problem_tensor(m):
    """the loss triple of the model on its boxes with the full tensor dd.S_energy as kappa AND as the energy product's weight, by
    mapped_reference.terms (boxes are the map diag(Jx, Jy)) under the dense Gram matrices"""
    from hp_vpinns_amd.testfcn import tables_1d
    mesh = m._mesh
    (xi, wx), (yi, wy) = m._rule
    X, A = mr.geom_boxes(mesh.boxes, xi, yi)
    ne, nq = X.shape[0], X.shape[1]
    coefs = dict(K=dd.S_energy(X.reshape(-1, 2)).reshape(ne, nq, 2, 2), b=np.zeros((ne, nq, 2)), s=np.zeros((ne, nq)))
    p = mr.problem([2, 8, 8, 1], 0, X, A, (xi, wx), (yi, wy), (4, 4), coefs, mass=0.0, boxes=mesh.boxes)
    p["theta"] = m.get_params()
    p["lbw"] = 3.0
    ax, by = tables_1d(4, xi)[0] * wx[None, :], tables_1d(4, yi)[0] * wy[None, :]
    J = np.prod((mesh.boxes[:, 1::2] - mesh.boxes[:, 0::2]) / 2, axis=1)
    p["F"] = J[:, None, None] * np.einsum("kj,ri,eji->ekr", by, ax, _f(X.reshape(-1, 2)).reshape(ne, yi.size, xi.size))
    p["data"] = (m.X_u_train, m.utrain)
    Gs = dd.grams(p, dd.S_energy)
    with dd._dense(Gs, p):
        return mr.terms(p)["triple"]


def test_set_mesh_between_boxes_and_mapped_and_checkpoints(tmp_path):
    from hp_vpinns_amd.adapt import ElementMesh
    m = _model(residual_norm=dict(kind="dual", metric="physical", mass=2.0))
    boxes = m.mesh.copy()
    l_box = m.loss()
    assert ";dual>" in _variant(m)
    m.set_mesh(_annulus())
    l_map = m.loss()
    assert ";dual=dense>" in _variant(m) and np.all(np.isfinite(np.asarray(l_map)))
    m.save_checkpoint(tmp_path / "ck")
    other = _model(mesh=_annulus(), residual_norm="l2")
    other.load_checkpoint(tmp_path / "ck")
    assert other.residual_norm == dict(kind="dual", mass=2.0, metric="physical", gram_points=None)
    assert np.asarray(other.loss()).tobytes() == np.asarray(l_map).tobytes()
    m.set_mesh(boxes)
    assert isinstance(m.mesh, ElementMesh) and ";dual>" in _variant(m)
    assert np.asarray(m.loss()).tobytes() == np.asarray(l_box).tobytes()
    with pytest.raises(ValueError, match='metric="physical"'):
        _model(mesh=_annulus(), residual_norm="dual")
