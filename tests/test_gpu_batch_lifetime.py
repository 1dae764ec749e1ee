"""Lifetime of a batch and of the MFMA object it owns (Batch::m, csrc/hpv_ctx.h): a point set given again at another size re-creates
the batch while an object, a captured iteration graph or an enqueued pass may still refer to the old one.

One handle per batch kind and backend walks  set(n = 17) -> 3 steps -> set(33) -> 3 steps -> set(16) -> 3 steps  (15, 16, 17, 33: the
sizes around the 16-point tile of the layer kernels; three steps replay a captured graph in the variational scheme).  A fresh handle
is given the final set from the start and the first handle's parameters and optimizer state at that moment (get_state / set_state),
and takes the same three steps: loss, parameters and optimizer state must be EQUAL BIT FOR BIT -- nothing of the earlier sizes may
have survived.  Data and flux terms go on to n = 0 against a handle on which the term was never assembled.

Shape: 2 x 2 elements of 5 x 5 points with 3 x 3 test functions, [2, 20, 20, 1] -- the smallest on which the MFMA layer kernels run
-- and the same with backend="generic".  What tests/test_gpu_flux.py, test_gpu_data_term.py, test_gpu_pinn.py and
test_gpu_validation.py already hold (sweeps of one live handle against the CPU references, pass by pass) is not repeated here."""
import numpy as np
import pytest

import data_term_reference as dr
import generic_point as gp

pytestmark = pytest.mark.gpu

L = [2, 20, 20, 1]
SEED = 9501
SEQUENCE = (17, 33, 16)
W_F = 2.5
_CACHE = {}


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HPV_NO_RULE_PADDING", "1")      # the 5 x 5 rule as it is


def _setup():
    """the warped 2 x 2 grid, generic initial parameters and 33 points of every kind (built once)"""
    if not _CACHE:
        from hp_vpinns_amd.drivers import poisson2d
        s = poisson2d.setup(N_el_x=2, N_el_y=2, N_test_x=3, N_test_y=3, N_quad=5, N_bound=13, with_test_grid=False)
        s = gp.warp_poisson2d(s, SEED)
        th = gp.generic_theta(L, SEED)
        rng = np.random.default_rng(SEED)
        X = dr.points("p2", 33, SEED)
        _CACHE.update(s=s, th=th, X=X, u=dr.targets("p2", L, th, X, SEED), g=rng.uniform(-1, 1, 33), a=rng.uniform(0.5, 1.5, 33),
                      b=rng.uniform(-1, 1, (33, 2)), f=rng.uniform(-2, 2, 33), du=rng.uniform(-1, 1, (33, 2)))
    return _CACHE


def _model(backend, scheme="VPINNs", layers=L, theta=None):
    from hp_vpinns_amd.vpinn import VPINN2D
    c = _setup()
    th = c["th"] if theta is None else theta
    return VPINN2D(*gp.p2_tuple(c["s"], layers), var_form=1, scheme=scheme, lossb_weight=3, init_params=th, backend=backend)


def _set(m, kind, n):
    c = _setup()
    if kind == "data":
        m.h.set_data(c["X"][:n] if n else None, c["u"][:n] if n else None)
    elif kind == "flux":
        if n:
            m.set_flux_data(c["X"][:n], c["g"][:n], a=c["a"][:n], b=c["b"][:n], weight=W_F)
        else:
            m.set_flux_data(None)
    elif kind == "collocation":
        m.h.set_collocation(c["X"][:n], c["f"][:n])
    elif kind == "validation":
        m.h.set_validation(c["X"][:n], c["u"][:n], c["du"][:n])
    else:
        raise AssertionError(kind)


def _three_steps(m, kind):
    """(loss after three steps, parameters, optimizer state, what the kind itself reports)"""
    l3 = np.asarray(m.h.step(3, True))
    own = np.asarray(m.flux_loss()) if kind == "flux" else np.asarray(m.h.validate()) if kind == "validation" else np.zeros(1)
    return l3, m.h.get_params(), m.h.get_state(), own


def _equal(x, y, tag):
    for p, q, what in zip(x, y, ("loss", "parameters", "optimizer state", "the term's own figures")):
        assert np.array_equal(p, q), (tag, what, np.abs(np.asarray(p) - np.asarray(q)).max())


def _expect_backend(m, backend):
    assert m.backend() == ("generic" if backend == "generic" else "mfma"), (backend, m.backend(), m.h.kernel_variant())


@pytest.mark.parametrize("backend", ["auto", "generic"])
@pytest.mark.parametrize("kind,scheme", [("data", "VPINNs"), ("flux", "VPINNs"), ("data", "PINNs"), ("flux", "PINNs"),
                                         ("collocation", "PINNs"), ("validation", "VPINNs")])
def test_a_point_set_given_again_at_other_sizes_leaves_nothing_behind(kind, scheme, backend):
    tag = (kind, scheme, backend)
    m = _model(backend, scheme)
    for n in SEQUENCE[:-1]:
        _set(m, kind, n)
        m.h.step(3, False)
    _set(m, kind, SEQUENCE[-1])
    state = m.h.get_state()
    got = _three_steps(m, kind)
    _expect_backend(m, backend)
    fresh = _model(backend, scheme)
    _set(fresh, kind, SEQUENCE[-1])
    fresh.h.set_state(state)
    _equal(got, _three_steps(fresh, kind), tag)
    if kind in ("data", "flux"):      # ... and on to no term at all
        _set(m, kind, 0)
        state = m.h.get_state()
        got = _three_steps(m, kind)
        never = _model(backend, scheme)
        _set(never, kind, 0)          # (before its first pass: the device batches are assembled lazily, the term never was)
        never.h.set_state(state)
        _equal(got, _three_steps(never, kind), tag + ("n = 0",))


@pytest.mark.parametrize("backend", ["auto", "generic"])
def test_prediction_and_evaluation_points_at_other_sizes_between_steps(backend):
    """hpv_predict, hpv_eval_points and hpv_residual_points keep one forward-only batch each, re-created when n changes"""
    c = _setup()
    m = _model(backend)
    for n in SEQUENCE + (15,):
        m.h.step(3, False)
        X = c["X"][:n]
        got = (m.h.predict(X), m.h.eval_points(X), m.h.residual_points(X, c["f"][:n]))
        fresh = _model(backend)
        fresh.h.set_state(m.h.get_state())
        want = (fresh.h.predict(X), fresh.h.eval_points(X), fresh.h.residual_points(X, c["f"][:n]))
        for p, q, what in zip(got, want, ("predict", "eval_points", "residual_points")):
            assert p.shape[-1] == n and np.array_equal(p, q), (backend, n, what)
        assert np.array_equal(got[0], got[1][0]), (backend, n, "u of predict and of eval_points")
    _expect_backend(m, backend)


def test_required_mfma_backend_on_an_uncovered_shape_of_the_strong_form_scheme():
    """backend='mfma' is a requirement: the first pass returns -4 where the collocation batch has no MFMA instantiation (five hidden
    layers are covered up to width 32 only; narrower and unequal widths would be zero-padded onto a covered one)"""
    from hp_vpinns_amd import _lib
    layers = [2, 40, 40, 40, 40, 40, 1]
    m = _model("mfma", "PINNs", layers, gp.generic_theta(layers, SEED))
    with pytest.raises(_lib.HpvError) as ei:
        m.loss_and_grad()
    assert ei.value.code == -4
    assert str(ei.value).startswith("libhpvpinn error -4: MFMA backend not available: "), str(ei.value)
