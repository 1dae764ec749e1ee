"""The dual-norm (Riesz) residual loss (hpv_set_residual_norm; k_project_lin_dual, k_project_nl_dual, k_project_id<.., true>:
csrc/hpv_dual_norm.h) on the device against the dense-solve reference of tests/dualnorm_reference.py, over its case table: the rows of
tests/linop_sweep.py at which the new loops change their trip count or the scratch layout is tightest, two rows whose scratch is
appended instead of aliased, per-element counts on boxes of aspect ratio up to 24, mass 0 and 3.  tests/test_dualnorm_host.py proves
every case on the CPU; profiles/dual_norm.md holds the measured figures.

Every case: loss triple, forward-only loss, gradient per block (the d c block included) and the validation sums within TOL = 1e-9
(test_gpu_ansatz._against_reference, unchanged, as tests/test_gpu_linop_sweep.py applies it); hpv_get_residuals -- the RAW residual --
within TOL and exactly 0 where the counts mask; a second pass bit-equal to the first; ";dual>" in the variant string."""
import numpy as np
import pytest

import dualnorm_reference as dn
import generic_point as gp
import linear_reference as lr
import linop_sweep as ls
from cases import rel
from test_gpu_ansatz import Dev, _against_reference, _rel3
from test_gpu_generic_point import STEP_TOL, TOL
from test_gpu_linop_sweep import _mask

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in dn.cases()}
_PROBLEMS = {}


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _problem(name):
    """the case's arrays and its dense-solve reference (loss triple, gradient, R), computed once and left unchanged"""
    if name not in _PROBLEMS:
        p = dn.problem(CASES[name])
        _PROBLEMS[name] = (p, dn.reference(p))
    return _PROBLEMS[name]


class DualDev(Dev):
    """test_gpu_ansatz.Dev with the dual norm of p['mass'] set behind the tables (dual=False: the plain handle)"""

    def __init__(self, p, dual=True, **kw):
        self.dual = dual
        super().__init__(p, **kw)

    def populate(self, p, *a, **kw):
        super().populate(p, *a, **kw)
        if self.dual:
            self.set_dual()

    def set_dual(self, mass=None, lam_scale=1.0):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.quadrature import gram_stacks
        p = self.p
        sx = gram_stacks(p["ntx"])
        sy = gram_stacks(p["nty"]) if p["dim"] == 2 else (None, None)
        self.h.set_residual_norm(_lib.NORM_DUAL, p["mass"] if mass is None else mass, sx[0], sx[1] * lam_scale, sy[0], sy[1])

    def set_l2(self):
        from hp_vpinns_amd import _lib
        self.h.set_residual_norm(_lib.NORM_L2)


KERNEL = {"lin": "k_project_lin<", "nl": "k_project_nl<", "id": "k_project_id<"}


@pytest.mark.parametrize("name", list(CASES))
def test_case_against_the_dense_solve_reference(name):
    c = CASES[name]
    p, ref = _problem(name)
    _, qx, qy, ntx, nty = ls.shape(c)
    nbytes, aliased = dn.lds_bytes(qx, qy, ntx, nty)
    assert nbytes <= ls.LDS_LIMIT                      # (hpv_dual_lds_bytes admits every row, ldsmax included: its scratch is aliased)
    d = DualDev(p)
    first = d.loss_and_grad()
    v = _against_reference(name, d, ref, validation=d.has_val)
    assert "%s%dx%d/%dx%d" % (KERNEL[c["variant"]], qx, qy, ntx, nty) in v and ";dual>" in v, v
    assert (";ansatz;dual>" in v) == (p["ans"] is not None) and d.h.lib.hpv_pass_structure(d.h._h) == 0, v
    Ro = ref[2]
    Rm = d.h.residuals(Ro.size).reshape(Ro.shape)
    eR = float(np.linalg.norm(Rm - Ro) / np.linalg.norm(Ro))
    m = _mask(p)
    print("%s | scratch %s | residuals %.2e | loss %.2e | block %.2e" % (name, "aliased" if aliased else "appended", eR,
          float(_rel3(first[0], ref[0]).max()), float(gp.worst_block(first[1], ref[1], p["layers"], d.nc)[1])))
    assert eR < TOL, (name, "residuals", eR)
    assert np.all(Rm[~m] == 0.0), (name, "masked residual entries are exactly 0")
    again = d.loss_and_grad()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), (name, "a second dual pass differs from the first")


@pytest.mark.parametrize("variant", ["lin", "nl", "id"])
def test_kind_zero_restores_the_plain_handle_bit_for_bit(variant):
    p, _ = _problem("nr272-" + variant)
    plain = DualDev(p, dual=False)
    l0, g0 = plain.loss_and_grad()
    R0 = plain.h.residuals(p["ntx"] * p["nty"] * (p["ee"] - p["eb"]))
    assert ";dual" not in plain.h.kernel_variant()
    d = DualDev(p)
    ld, gd = d.loss_and_grad()
    assert ";dual>" in d.h.kernel_variant() and not np.array_equal(ld, l0)
    d.set_l2()
    l1, g1 = d.loss_and_grad()
    R1 = d.h.residuals(R0.size)
    assert d.h.kernel_variant() == plain.h.kernel_variant()
    assert l1.tobytes() == l0.tobytes() and g1.tobytes() == g0.tobytes() and R1.tobytes() == R0.tobytes()
    lf0, lf1 = plain.h.loss_and_grad(False)[0], d.h.loss_and_grad(False)[0]
    assert np.asarray(lf0).tobytes() == np.asarray(lf1).tobytes()


def test_indicators_column_zero_is_the_dual_loss():
    from hp_vpinns_amd.quadrature import diff_matrix
    p, ref = _problem("counts-lin")
    d = DualDev(p, validation=False)
    d.h.set_strong_form(diff_matrix(p["xr"][0]), diff_matrix(p["yr"][0]))
    ind = d.h.linear_indicators(None)
    le = dn.dense_route(p, ref[2])[0]
    e = float(np.abs(ind[:, 0] - le).max() / np.abs(le).max())
    print("indicators, column 0 against the reference's per-element dual loss: %.2e" % e)
    assert e < TOL
    d.set_l2()
    ind2 = d.h.linear_indicators(None)
    assert ind2[:, 1:].tobytes() == ind[:, 1:].tobytes()
    plain = DualDev(p, dual=False, validation=False)
    plain.h.set_strong_form(diff_matrix(p["xr"][0]), diff_matrix(p["yr"][0]))
    assert plain.h.linear_indicators(None).tobytes() == ind2.tobytes()


def _code(call):
    from hp_vpinns_amd import _lib
    with pytest.raises(_lib.HpvError) as e:
        call()
    return e.value.code, str(e.value)


def test_lifecycle():
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.quadrature import gram_stacks
    from hp_vpinns_amd.testfcn import tables_1d
    p, ref = _problem("counts-lin")
    d = DualDev(p)
    _against_reference("counts-lin", d, ref)
    # the tables belong to the test-function tables: hpv_set_tables drops them, and a pass refuses until the setter is called again
    d.h.set_tables(tables_1d(p["ntx"], p["xr"][0]), tables_1d(p["nty"], p["yr"][0]))
    code, msg = _code(d.loss_and_grad)
    assert code == -3 and "hpv_set_residual_norm" in msg, (code, msg)
    code, _ = _code(lambda: d.h.loss_and_grad(False))
    assert code == -3
    d.set_dual()
    _against_reference("counts-lin after hpv_set_tables and the setter", d, ref)
    # refused, and the handle keeps what it had
    code, msg = _code(lambda: d.set_dual(mass=-1.0))
    assert code == -1 and "mass" in msg, (code, msg)
    code, msg = _code(lambda: d.set_dual(lam_scale=-1.0))
    assert code == -1 and "lam" in msg, (code, msg)
    code, msg = _code(lambda: d.set_dual(lam_scale=0.0))
    assert code == -1
    code, msg = _code(lambda: d.h.set_residual_norm(2))
    assert code == -1
    sx = gram_stacks(p["ntx"])
    code, msg = _code(lambda: d.h.set_residual_norm(_lib.NORM_DUAL, 0.0, sx[0], sx[1], None, None))      # 2-D without the y tables
    assert code == -1
    l3, g = d.loss_and_grad()
    assert _rel3(l3, ref[0]).max() < TOL and ";dual>" in d.h.kernel_variant()
    # another class
    other = _lib.Handle(_lib.PDE_POISSON2D, 1, _lib.ACT_TANH, [2, 20, 20, 20, 1])
    code, msg = _code(lambda: other.set_residual_norm(_lib.NORM_DUAL, 0.0, sx[0], sx[1], sx[0], sx[1]))
    assert code == -3 and "linear problems" in msg, (code, msg)
    # before hpv_set_tables
    fresh = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, [2, 8, 8, 1])
    code, msg = _code(lambda: fresh.set_residual_norm(_lib.NORM_DUAL, 0.0, sx[0], sx[1], sx[0], sx[1]))
    assert code == -3 and "hpv_set_tables" in msg, (code, msg)


def test_scratch_past_the_lds_limit_is_refused():
    """a 1-D shape hpv_set_tables admits, whose scratch does not fit the G region: appended, it is past 64 KiB -- refused with -1 on
    the host, and the handle goes on under l2"""
    qx, _, ntx, _ = dn.REFUSED_1D
    c = ls._case("refused", dict(L=ls.L1, boxes=lr.BOXES1[:1], q=qx, nt=ntx, data=1, flux=0), "lin", None, 12991)
    p = dn.problem(dict(c, mass=0.0))
    d = DualDev(p, dual=False, validation=False)
    l0, g0 = d.loss_and_grad()
    code, msg = _code(d.set_dual)
    assert code == -1 and "LDS" in msg, (code, msg)
    l1, g1 = d.loss_and_grad()
    assert np.array_equal(l0, l1) and np.array_equal(g0, g1) and ";dual" not in d.h.kernel_variant()


def _poisson_model(**kw):
    from hp_vpinns_amd.vpinn import VPINNLinear
    g = np.array([-1.0, 0.1, 1.0])

    def f(P):
        return -2.0 * np.pi ** 2 * np.sin(np.pi * P[:, 0]) * np.sin(np.pi * P[:, 1])
    t = np.linspace(-1.0, 1.0, 9)
    Xb = np.concatenate([np.stack([t, -np.ones(9)], 1), np.stack([t, np.ones(9)], 1), np.stack([-np.ones(9), t], 1), np.stack([np.ones(9), t], 1)])
    return VPINNLinear([2, 8, 8, 1], grid_x=g, grid_y=g, n_quad=6, n_test=4, kappa=1.0, f=f, X_u_train=Xb, u_train=np.zeros(36),
                       lossb_weight=3.0, seed=7, **kw)


def _model_problem(m, mass):
    """linear_reference.from_model as the problem dict dualnorm_reference.reference takes (no nonlinear term, no coefficients, no ansatz)"""
    import ident_reference as ir
    p = lr.from_model(m)
    K, M = ir.n_planes(p["dim"])
    nq = p["planes"].shape[1]
    p.update(nl=np.zeros((M, nq)), terms=(), dirs=np.zeros((0, K + M, nq)), c0=np.zeros(0), full=p["theta"].copy(), ans=None, kind=None, mass=mass)
    return p


def test_training_under_the_dual_norm():
    """50 Adam steps on 2 x 2 elements, (6,6)/(4,4), Poisson with a manufactured solution: the model's loss and gradient and its first
    20 steps against the dense-solve reference and its TF1-Adam trajectory; the history is finite and ends below where it started"""
    m = _poisson_model(residual_norm=dict(kind="dual", mass=3.0))
    assert m.residual_norm == dict(kind="dual", mass=3.0)
    m.set_params(gp.generic_theta([2, 8, 8, 1], 12931))      # (a fresh model's zero biases leave gradient blocks at rounding level)
    p = _model_problem(m, 3.0)
    ref = dn.reference(p)
    l3, g = m.loss_and_grad()
    assert ";dual>" in m.h.kernel_variant()
    eb = float(gp.worst_block(np.asarray(g), ref[1], p["layers"], 0)[1])
    print("model against the reference: loss %s, worst block %.2e" % (_rel3(l3, ref[0]), eb))
    assert _rel3(l3, ref[0]).max() < TOL and eb < TOL
    m.train(20)
    e = float(rel(m.get_params(), dn.adam_trajectory(p, 20)))
    print("20 Adam steps under the dual norm: parameters %.2e" % e)
    assert e < STEP_TOL
    m.train(30)
    his = np.asarray(m.loss_his)
    assert his.size == 50 and np.all(np.isfinite(his)) and his[-1] < his[0], (his[0], his[-1])


def test_set_residual_norm_and_checkpoint_round_trip(tmp_path):
    m = _poisson_model()
    assert m.residual_norm == "l2"
    l2 = m.loss()
    m.set_residual_norm("dual")
    ld = m.loss()
    assert not np.array_equal(np.asarray(l2), np.asarray(ld))
    ref = dn.reference(_model_problem(m, 0.0))
    assert _rel3(ld, ref[0]).max() < TOL
    m.save_checkpoint(tmp_path / "ck")
    other = _poisson_model()
    other.load_checkpoint(tmp_path / "ck")
    assert other.residual_norm == dict(kind="dual", mass=0.0)
    assert np.asarray(other.loss()).tobytes() == np.asarray(ld).tobytes()
    m.set_residual_norm("l2")
    assert np.asarray(m.loss()).tobytes() == np.asarray(l2).tobytes()
