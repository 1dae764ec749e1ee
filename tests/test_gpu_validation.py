"""Device-side validation on the GPU: hpv_eval_points / hpv_residual_points / hpv_validate / the validation history and
hpv_step_validate, through the public classes (evaluate, residual, set_validation, validate, train_validated).

Inputs sit at generic points: generic_point.generic_theta (every weight and bias perturbed), points drawn inside the domain, the
handles of tests/shape_matrix.py (warped grids, seeded right-hand sides).  Expected values: tests/validation_reference.py (the
oracle classes' own net_* through torch autograd, fp64), itself checked against finite differences in test_validation_host.py.

Bounds.  The forward kernels behind `evaluate` are the ones tests/shape_matrix.py covers, and the bound per channel is the one its
`conditions` applies per block -- shape_matrix.BLOCK_AGREE, a relative 2-norm, imported, not restated (profiles/shape_matrix.md: the
measured errors of those kernels are 1e-16 .. 2e-14).  A residual combines k channels and gets k times that.  A case is well posed
when no channel (residual) is negligible next to the others -- asserted on the reference alone, like generic_point.BLOCK_FLOOR.
The raw sums of `validate` are compared with numpy sums over the channel values `evaluate` returned for the same points to 1e-12
relative: every term is non-negative and either side's summation error is below n 2^-53 (6e-13 at the largest n here, 5 000);
max |u^ - u| must be EQUAL, and two calls bitwise equal.  History rows and the final optimizer state are compared bitwise with the
same chunks of hpv_step + hpv_validate on a second handle: the chunk structure is the same and validation only reads."""
import os
import subprocess
import sys

import numpy as np
import pytest

import generic_point as gp
import shape_matrix as sm
import validation_reference as vr
from cases import rel

pytestmark = pytest.mark.gpu

TOL = sm.BLOCK_AGREE
SUM_TOL = 1e-12
WELL_POSED = 1e-3       # a channel's (the residual's) norm against the largest channel norm (the sum of its terms' norms)
N_POINTS = (1, 63, 257)


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH"):
        monkeypatch.delenv(k, raising=False)


def _own_case(name, prob, kind, vf, layers, seed, scale=0.3):
    return dict(name=name, prob=prob, kind=kind, vf=vf, layers=list(layers), seed=seed, scale=scale, env={},
                n_extra=1 if prob == "adv" else 0)


_MATRIX = {c["name"]: c for c in sm.matrix_cases()}
# name -> (case, keyword arguments of the product class, the kernel family the forward runs on)
EVAL_CASES = {
    "p1-[1,20,20,20,1]-sin": (_MATRIX["p1-vf2-H20-L3"], {}, "mfma"),
    "p2-[2,20,20,20,1]": (_MATRIX["p2-vf1-H20-L3"], {}, "mfma"),
    "p2-[2,32,32,32,1]-wide": (_MATRIX["p2-vf1-H32-L3"], {}, "mfma"),
    "p2-[2,7,9,1]-generic": (_own_case("p2-generic", "p2", "var", 1, [2, 7, 9, 1], 8101), dict(backend="generic"), "generic"),
    "adv-[2,20,20,20,1]": (_own_case("adv-vf0", "adv", "var", 0, [2, 20, 20, 20, 1], 8102), {}, "mfma"),
    # (a strong-form handle picks its training kernels at the first pass and reports the generic backend until then)
    "adv-pinn-[2,20,20,20,1]": (_MATRIX["adv-pinn-H20-L3"], {}, None),
}


def _model(c, **kw):
    inp = sm.inputs(c)
    return sm.product(c, inp, **kw), inp


def _pts(c, n, salt=0):
    return sm._uniform(np.random.default_rng(c["seed"] + 77 * n + salt), n, c["prob"])


@pytest.mark.parametrize("name", list(EVAL_CASES), ids=list(EVAL_CASES))
def test_evaluate_against_autograd(name):
    c, kw, family = EVAL_CASES[name]
    m, inp = _model(c, **kw)
    assert family is None or m.backend() == family, (name, m.backend())
    names = vr.NAMES[c["prob"]]
    for n in N_POINTS:
        X = _pts(c, n)
        want = vr.channels(c["prob"], c["layers"], inp["th"], X)
        got = m.evaluate(X)
        assert tuple(got) == names
        biggest = max(np.linalg.norm(v) for v in want.values())
        for k in names:
            assert got[k].shape == (n, 1)
            assert np.linalg.norm(want[k]) >= WELL_POSED * biggest, ("ill-posed case", name, n, k)
            e = rel(got[k], want[k])
            print("%s n=%d %s: %.2e" % (name, n, k, e))
            assert e < TOL, (name, n, k, e)
        assert np.array_equal(m.evaluate(X)["u_x"], got["u_x"])          # the batch is reused at equal n
    X = _pts(c, 63)
    assert rel(m.predict(X), m.evaluate(X)["u"]) < TOL          # (predict runs the value-only kernel)


RES_CASES = {"p1": ("p1-[1,20,20,20,1]-sin", 1), "p2": ("p2-[2,20,20,20,1]", 2), "adv": ("adv-[2,20,20,20,1]", 3),
             "adv-pinn": ("adv-pinn-[2,20,20,20,1]", 3)}


def _residual_terms(prob, ch, eps, f):
    if prob == "p1":
        return [ch["u_xx"], f]
    if prob == "p2":
        return [ch["u_xx"], ch["u_yy"], f]
    return [ch["u_t"], sm.V * ch["u_x"], eps * ch["u_xx"], f]


@pytest.mark.parametrize("key", list(RES_CASES), ids=list(RES_CASES))
def test_residual_against_autograd(key):
    name, k_channels = RES_CASES[key]
    c, kw, _ = EVAL_CASES[name]
    m, inp = _model(c, **kw)
    prob, th = c["prob"], np.array(inp["th"])
    thetas = [th]
    if prob == "adv":      # the residual follows the epsilon the device holds
        th2 = th.copy(); th2[-1] = 0.37
        thetas.append(th2)
    for t in thetas:
        m.set_params(t)
        for n in N_POINTS:
            X = _pts(c, n, salt=3)
            f = np.random.default_rng(c["seed"] + n).standard_normal((n, 1))
            for ff in ([f, None] if prob == "adv" else [f]):
                want = vr.residual(prob, c["layers"], t, X, ff, V=sm.V)
                ch = vr.channels(prob, c["layers"], t, X)
                terms = _residual_terms(prob, ch, t[-1], np.zeros((n, 1)) if ff is None else ff)
                assert np.linalg.norm(want) >= WELL_POSED * sum(np.linalg.norm(v) for v in terms), ("ill-posed case", key, n)
                got = m.residual(X, ff)
                assert got.shape == (n, 1)
                e = rel(got, want)
                print("%s eps=%.2f n=%d f=%s: %.2e" % (key, t[-1] if prob == "adv" else 0.0, n, "given" if ff is not None else "None", e))
                assert e < k_channels * TOL, (key, n, e)


@pytest.mark.parametrize("with_du", [False, True], ids=["u", "u+du"])
@pytest.mark.parametrize("n", [1, 63, 1500, 5000])
def test_validate_raw_sums(n, with_du):
    """n = 1 500 crosses one workgroup's stride, n = 5 000 runs the reduction on several workgroups (one per 2 048 points)."""
    c, kw, _ = EVAL_CASES["p2-[2,20,20,20,1]"]
    m, inp = _model(c, **kw)
    X = _pts(c, n, salt=5)
    rng = np.random.default_rng(9000 + n)
    u = rng.standard_normal((n, 1))
    du = rng.standard_normal((n, 2)) if with_du else None
    m.set_validation(X, u, du)
    r1 = m.validate()
    r2 = m.validate()
    assert np.array_equal(r1["raw"], r2["raw"]), (r1["raw"], r2["raw"])
    ch = m.evaluate(X)
    want = vr.norms(ch["u"], u, np.hstack([ch["u_x"], ch["u_y"]]) if with_du else None, du)
    raw = r1["raw"]
    print("n=%d du=%s raw %s numpy %s" % (n, with_du, raw, want))
    assert raw[5] == n
    assert raw[2] == want[2], ("max |u^ - u|", raw[2], want[2])
    for i in (0, 1) + ((3, 4) if with_du else ()):
        assert abs(raw[i] - want[i]) <= SUM_TOL * want[i], (i, raw[i], want[i])
    if not with_du:
        assert raw[3] == 0.0 and raw[4] == 0.0 and r1["rel_h1"] is None
    else:
        assert np.isfinite(r1["rel_h1"]) and abs(r1["rel_h1"] - np.sqrt(want[3] / want[4])) < 1e-11
    assert abs(r1["rel_l2"] - np.sqrt(want[0] / want[1])) < 1e-11 and r1["max_abs"] == want[2]
    assert abs(r1["rel_l2"] - m.rel_l2_error(X, u)) < 1e-9          # the host route it replaces


# ---- history semantics ---------------------------------------------------------------------------------------------------------
def _small_p2():
    """the smallest grid that still trains: 2 x 2 elements of 10 x 10 points, 5 x 5 test functions, [2, 20, 20, 20, 1]"""
    from hp_vpinns_amd.drivers import poisson2d
    s = poisson2d.setup(N_el_x=2, N_el_y=2, N_test_x=5, N_test_y=5, N_quad=10, N_bound=20, with_test_grid=False)
    layers = [2, 20, 20, 20, 1]
    th = gp.generic_theta(layers, 8200)
    rng = np.random.default_rng(8201)
    Xv = rng.uniform(-1, 1, (300, 2))
    uv = poisson2d.u_ext(Xv[:, 0:1], Xv[:, 1:2])

    def make():
        m = poisson2d.build_model(s, layers, var_form=1, init_params=th)
        m.set_validation(Xv, uv)
        return m
    return make


def history_case(n_iters, every, want_graphs):
    """rows of hpv_step_validate on handle A == hpv_step(every) + hpv_validate on handle B, bitwise; so is the final state"""
    make = _small_p2()
    a, b = make(), make()
    rows = a.h.step_validate(n_iters, every)
    assert rows.shape == (n_iters // every, 6)
    want = []
    for _ in range(n_iters // every):
        b.h.step(every, False)
        want.append(b.h.validate())
    if n_iters % every:
        b.h.step(n_iters % every, False)
    want = np.array(want).reshape(-1, 6)
    assert np.array_equal(rows, want), (rows, want)
    assert np.array_equal(a.h.get_state(), b.h.get_state())
    assert a.h.updates_applied() == n_iters == b.h.updates_applied()
    assert a.h.graphs_in_use() == want_graphs == b.h.graphs_in_use()
    assert a.h.kernel_variant() == b.h.kernel_variant() and a.h.pass_structure() == b.h.pass_structure()
    assert np.all(rows[:, 5] == 300) and np.all(rows[:, 0] > 0)
    if rows.shape[0] > 1:
        assert not np.array_equal(rows[0], rows[-1])      # (the parameters moved between the samples)
    return rows


@pytest.mark.parametrize("n_iters,every", [(21, 5), (3, 1), (23, 11)])
def test_step_validate_rows_and_state_bitwise(n_iters, every):
    history_case(n_iters, every, True)


def test_step_validate_without_graphs_in_a_fresh_process():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HPV_NO_GRAPH="1", PYTHONPATH=os.pathsep.join([root] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "21", "5"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "history-case-ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_history_limits():
    from hp_vpinns_amd import _lib
    m = _small_p2()()
    before = m.h.get_state()
    with pytest.raises(_lib.HpvError) as e:
        m.h.step_validate(_lib.HIST_CAP + 1, 1)
    assert e.value.code == -1
    assert np.array_equal(m.h.get_state(), before) and m.h.updates_applied() == 0      # refused before anything ran
    m.h.validation_reset()
    m.h.validate_enqueue()
    m.h.validate_enqueue()
    rows = m.h.validation_read(2)
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], m.h.validate())
    with pytest.raises(_lib.HpvError) as e:
        m.h.validation_read(3)
    assert e.value.code == -3 and "only 2" in str(e.value)
    with pytest.raises(_lib.HpvError) as e:
        m.h.validation_read(_lib.HIST_CAP + 1)
    assert e.value.code == -1


def test_advdiff_train_validated():
    c, kw, _ = EVAL_CASES["adv-[2,20,20,20,1]"]
    a, inp = _model(c, **kw)
    b, _ = _model(c, **kw)
    X = _pts(c, 200, salt=9)
    rng = np.random.default_rng(8300)
    u, du = rng.standard_normal((200, 1)), rng.standard_normal((200, 2))
    for m in (a, b):
        m.set_validation(X, u)
    its, l2, mx = a.train_validated(20, 10)
    assert list(its) == [10, 20] and l2.shape == mx.shape == (2,)
    for k in range(2):
        b._step(10, False)
        v = b.validate()
        assert v["rel_h1"] is None
        assert l2[k] == v["rel_l2"] and mx[k] == v["max_abs"], (k, l2[k], v)
    assert np.array_equal(a.h.get_state(), b.h.get_state())
    b.set_validation(X, u, du)
    v = b.validate()
    assert v["rel_h1"] is not None and np.isfinite(v["rel_h1"]) and v["rel_h1"] > 0
    assert v["rel_l2"] == l2[1]
    its, l2, mx = a.train_validated(7, 10)      # fewer iterations than one sample: trained, not validated
    assert its.size == 0 and a.h.updates_applied() == 27


def test_default_validation_set_is_the_stored_test_grid():
    c, kw, _ = EVAL_CASES["p2-[2,20,20,20,1]"]
    m, inp = _model(c, **kw)          # (gp.p2_tuple hands X_u_train / u_train in as the test grid)
    m.set_validation()
    v = m.validate()
    assert v["raw"][5] == np.shape(m.X_test)[0]
    assert abs(v["rel_l2"] - m.rel_l2_error(m.X_test, m.utest)) < 1e-9


def test_error_paths():
    import ctypes as C
    from hp_vpinns_amd import _lib
    c, kw, _ = EVAL_CASES["p2-[2,20,20,20,1]"]
    m, inp = _model(c, **kw)
    for call in (m.validate, m.h.validate_enqueue, m.h.validation_reset, lambda: m.h.step_validate(2, 1), lambda: m.h.validation_read(0)):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == -3, call
    X = _pts(c, 10)
    u = np.ones((10, 1))
    m.set_validation(X, u)
    assert m.validate()["raw"][5] == 10
    for n_iters, every in ((5, 0), (5, -1), (-1, 1)):
        with pytest.raises(_lib.HpvError) as e:
            m.h.step_validate(n_iters, every)
        assert e.value.code == -1
    out = np.empty(6)
    dp = C.POINTER(C.c_double)
    assert m.h.lib.hpv_step_validate(m.h._h, 2, 1, out.ctypes.data_as(dp), 6) == -1          # two samples need 12
    ch = np.empty(5 * 10 - 1)
    assert m.h.lib.hpv_eval_points(m.h._h, X.ctypes.data_as(dp), 10, ch.ctypes.data_as(dp), ch.size) == -1
    assert m.h.updates_applied() == 0
    m.clear_validation()           # n = 0
    with pytest.raises(_lib.HpvError) as e:
        m.validate()
    assert e.value.code == -3
    with pytest.raises(ValueError):
        m.evaluate(np.zeros((4, 3)))
    with pytest.raises(ValueError):
        m.train_validated(5, 0)


if __name__ == "__main__":      # the fresh child process of test_step_validate_without_graphs_in_a_fresh_process
    history_case(int(sys.argv[1]), int(sys.argv[2]), os.environ.get("HPV_NO_GRAPH") != "1")
    print("history-case-ok")
