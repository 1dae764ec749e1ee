"""The flux term (hpv_set_flux_data: Neumann / Robin conditions, derivative observations) on every launch structure; the measured
errors are in profiles/flux_term.md.

One handle per structure (flux_reference.STRUCTURES, the strong-form scheme on the three problems) at a generic point; on that LIVE
handle the flux set is swept over 1, 15, 16, 17, 33 points and back to 1, with the case's Dirichlet data and without it.  After every
call: loss_and_grad() -- loss triple, gradient per block -- the forward-only loss() and flux_loss() against
oracle + flux_part of tests/flux_reference.py (CPU, fp64; tests/test_flux_host.py proves it), the kernel instantiation and the pass
structure; at the end four Adam steps against the same rule in numpy.  Conditions (a) - (d) of the reference module are asserted on the
reference alone before a device number is looked at.

Bounds: TOL = 1e-9 on the loss triple and the gradient per block, STEP_TOL = 1e-8 on the parameters after four
Adam steps (both imported from tests/test_gpu_generic_point.py), data_term_reference.LOSSB_TOL = 1e-12 on msf against numpy."""
import time

import numpy as np
import pytest

import data_term_reference as dr
import flux_reference as fr
import generic_point as gp
from cases import rel
from test_gpu_data_term import _pinn_model, _rel3
from test_gpu_generic_point import STEP_TOL, TOL, _pair

pytestmark = pytest.mark.gpu

WORST = {}          # (structure, data?, n) -> (loss triple, gradient block, msf, forward-only triple)


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _set(m, f, w=fr.W_F):
    """the class surface: set_flux_data(X, g, a, b, weight); f None clears the term"""
    if f is None:
        m.set_flux_data(None)
    else:
        m.set_flux_data(f["X"], f["g"], a=f["a"], b=f["b"], weight=w)


def _compare(tag, m, prob, L, th, rest, d, f, want, structure, with_data):
    """one flux set on the live handle against rest (lossv, gradient of everything but the flux term) + data figures d + flux_part"""
    ne = dr.n_extra(prob)
    n = f["X"].shape[0]
    fig = fr.conditions(prob, L, th, f, rest["grad"], TOL)                     # the reference alone, first
    fp = fr.flux_part(prob, L, th, f)
    l3o = fr.triple(prob, rest["lossv"], d, fp)
    go = rest["grad"] + fp["grad"]
    _set(m, f)
    l3m, gm = m.loss_and_grad()
    v, ps = m.h.kernel_variant(), m.h.pass_structure()
    fl = m.flux_loss()
    lf = m.loss()
    fl2 = m.flux_loss()
    e3, ef = _rel3(l3m, l3o), _rel3(lf, l3o)
    kb, eb = gp.worst_block(gm, go, L, ne)
    ems = max(abs(fl[1] - fp["msf"]), abs(fl2[1] - fp["msf"])) / fp["msf"]
    print("%s %s n = %d | %s | %s | loss3 %s | worst block %s %.2e (global %.2e) | msf %.1e | forward-only %s | share %.1e, leave-one-out %s, column %.1e"
          % (tag, "with data" if with_data else "no data", n, v, ps, e3, kb, eb, rel(gm, go), ems, ef, fig["share"],
             "%.1e" % fig["loo"] if fig["loo"] is not None else "loss", fig["column"]))
    now = (float(e3.max()), float(eb), float(ems), float(ef.max()))
    key = (tag, with_data, n)
    WORST[key] = tuple(max(x, y) for x, y in zip(now, WORST.get(key, now)))
    for s in want:
        assert s in v, (tag, n, "wanted", s, "ran", v, ps)
    if structure is not None:
        assert ps == structure, (tag, n, v, ps)
    assert e3.max() < TOL, (tag, n, v, "loss triple", l3m, l3o)
    assert eb < TOL, (tag, n, v, "gradient block", kb, eb)
    assert ems < dr.LOSSB_TOL and fl[0] == fr.W_F * fl[1], (tag, n, v, "msf", fl, fl2, fp["msf"])
    assert ef.max() < TOL, (tag, n, v, "forward-only pass", lf, l3o)


def _sweep(tag, o, m, prob, L, th, a, w, want, structure):
    t0 = time.time()
    var = dr.var_part(o, prob, L, th, a[0], a[1], w)
    f33 = fr.sweep_data(prob, L, th)
    zero = dict(wmsq=0.0, msq=0.0, grad=0.0)
    for with_data in (True, False):
        if with_data:
            rest, d = dict(lossv=var["lossv"], grad=var["full"][1]), var["data_full"]
        else:
            m.h.set_data(None, None)
            rest, d = dict(lossv=var["lossv"], grad=var["grad"]), zero
        for n in fr.SWEEP:
            _compare(tag, m, prob, L, th, rest, d, fr.head(f33, n), want, structure, with_data)
    # four Adam steps with the case's Dirichlet data and 17 flux points, from the initial parameters and a fresh optimizer
    m.h.set_data(np.asarray(a[0], dtype=np.float64), np.asarray(a[1], dtype=np.float64).reshape(-1))
    f17 = fr.head(f33, 17)
    _set(m, f17)
    m.set_params(th)
    m._step(4, False)
    pm, po = m.get_params(), fr.adam_trajectory(o, prob, L, f17, 4)
    print("%s | four Adam steps: parameters %.2e | %s | %.1f s" % (tag, rel(pm, po), m.h.kernel_variant(), time.time() - t0))
    WORST[(tag, "adam", 17)] = (float(rel(pm, po)),)
    assert rel(pm, po) < STEP_TOL, (tag, "parameters after four Adam steps", rel(pm, po))
    if dr.n_extra(prob):
        assert abs(pm[-1] - po[-1]) < STEP_TOL * abs(po[-1]), (tag, "epsilon after four Adam steps", pm[-1], po[-1])


@pytest.mark.parametrize("name", list(fr.STRUCTURES))
def test_flux_sweep_on_a_live_handle(name, monkeypatch):
    c = fr.STRUCTURES[name]
    o, m, a, th, _ = _pair(c, monkeypatch)
    _sweep(name, o, m, c["prob"], c["L"], th, a, float(c["lbw"]), c["want"], c["structure"])
    assert m.backend() == ("generic" if c.get("backend") == "generic" else "mfma")


@pytest.mark.parametrize("prob", fr.PINN)
def test_flux_sweep_under_the_strong_form_scheme(prob):
    o, a, L, th = dr.pinn_case(prob, "mfma")
    m = _pinn_model(prob, a, th, "mfma")
    _sweep("pinn-" + prob, o, m, prob, L, th, a, dr.PINN_W[prob], ["k_pinn_residual", "k_fwd_mfma<"], None)
    assert m.backend() == "mfma"


def test_grid_stride_loop_beyond_64_blocks(monkeypatch):
    """16 400 points: more than 64 x 256, every thread of k_flux_loss takes a second trip"""
    c = fr.STRUCTURES["generic"]
    o, m, a, th, _ = _pair(c, monkeypatch)
    var = dr.var_part(o, c["prob"], c["L"], th, a[0], a[1], float(c["lbw"]))
    f = fr.flux_data(c["prob"], c["L"], th, fr.LARGE_N, fr.LARGE_SEED)
    _compare("generic-large", m, c["prob"], c["L"], th, dict(lossv=var["lossv"], grad=var["full"][1]), var["data_full"], f, c["want"],
             c["structure"], True)


def _state(m, steps=4):
    l3, g = m.loss_and_grad()
    m._step(steps, False)
    return np.asarray(l3), np.asarray(g), m.get_params(), m.h.get_state()


@pytest.mark.parametrize("name", ["fused", "tile-1d"])
def test_removing_the_term_restores_the_bytes_of_a_handle_without_it(name, monkeypatch):
    c = fr.STRUCTURES[name]
    _, m0, a, th, _ = _pair(c, monkeypatch)
    _, m1, _, _, _ = _pair(c, monkeypatch)
    _set(m1, fr.head(fr.sweep_data(c["prob"], c["L"], th), 17))
    l3, _ = m1.loss_and_grad()
    assert m1.flux_loss()[1] > 0.0
    _set(m1, None)
    assert m1.flux_loss() == (0.0, 0.0)
    s0, s1 = _state(m0), _state(m1)
    for x, y, what in zip(s0, s1, ("loss triple", "gradient", "parameters after four Adam steps", "optimizer state")):
        assert np.array_equal(x, y), (name, what)
    assert s1[0][0] != l3[0]


def test_a_graph_captured_before_the_flux_data_changed_is_dropped(monkeypatch):
    c = fr.STRUCTURES["fused"]
    o, m, a, th, _ = _pair(c, monkeypatch)
    f33 = fr.sweep_data(c["prob"], c["L"], th)
    _set(m, fr.head(f33, 17))
    m._step(3, False)                       # captures the 3-iteration graph on 17 flux points
    assert m.h.graphs_in_use()
    m.set_params(th)                        # (keeps the graphs)
    _set(m, f33)
    m._step(3, False)
    assert m.h.graphs_in_use()
    pm, po = m.get_params(), fr.adam_trajectory(o, c["prob"], c["L"], f33, 3)
    stale = fr.adam_trajectory(fr.oracle_of(c)[0], c["prob"], c["L"], fr.head(f33, 17), 3)
    print("three steps on 33 flux points: %.2e (against the 17-point trajectory: %.2e)" % (rel(pm, po), rel(pm, stale)))
    assert rel(po, stale) > 100 * STEP_TOL      # the reference alone: the two trajectories are told apart
    assert rel(pm, po) < STEP_TOL


@pytest.mark.parametrize("name", ["fused", "tile-2d", "generic"])
def test_two_passes_at_the_same_parameters_return_the_same_bytes(name, monkeypatch):
    c = fr.STRUCTURES[name]
    _, m, a, th, _ = _pair(c, monkeypatch)
    _set(m, fr.sweep_data(c["prob"], c["L"], th))
    r = []
    for _ in range(2):
        l3, g = m.loss_and_grad()
        r.append((np.asarray(l3), np.asarray(g), np.asarray(m.flux_loss())))
    assert all(np.array_equal(x, y) for x, y in zip(*r)), name


def test_one_rank_communicator_against_the_single_gpu_path(monkeypatch):
    """the multi-GPU code path (in-library RCCL exchange, 1-rank world, as tests/test_gpu_deferred.py sets it up) with flux data: the
    deferred update is applied in front of the pass instead of riding in k_iter_fused's prologue -- eight iterations, bit for bit"""
    from test_gpu_deferred import L3, _model
    res = []
    for mode in ("rccl", "single"):
        m = _model(6, 5, L3, mode)
        th = m.get_params()
        m.set_flux_data(**_kwargs(fr.head(fr.flux_data("p2", L3, th, 33, fr.FLUX_SEED), 17)))
        if mode == "rccl":
            assert m.h.exchange_in_use() == "rccl"
        hist = np.asarray(m.h.step(8, True)).reshape(-1)[:3]
        assert "k_iter_fused" in m.h.kernel_variant()
        res.append((hist, m.h.get_params(), m.h.get_state(), np.asarray(m.flux_loss())))
        assert m.h.updates_applied() == 8 and res[-1][3][1] > 0.0
    for x, y, what in zip(res[0], res[1], ("loss", "parameters", "optimizer state", "flux loss")):
        assert np.array_equal(x, y), (what, rel(x, y))


def _kwargs(f):
    return dict(X=f["X"], g=f["g"], a=f["a"], b=f["b"], weight=fr.W_F)


@pytest.mark.parametrize("prob", ["p1", "p2", "adv"])
def test_python_surface_on_each_class(prob):
    """set_flux_data with a broadcast b and a scalar a, flux_loss, and X=None; a = 1, b = 0, g = u_d, weight = lossb_weight doubles
    the Dirichlet term"""
    o, a, L, th = dr.pinn_case(prob, "mfma")
    m = _pinn_model(prob, a, th, "mfma")
    w = dr.PINN_W[prob]
    l0, g0 = m.loss_and_grad()
    assert m.flux_loss() == (0.0, 0.0)
    Xd, ud = np.asarray(a[0], dtype=np.float64), np.asarray(a[1], dtype=np.float64).reshape(-1)
    m.set_flux_data(Xd, ud, a=1.0, b=None, weight=w)
    l1, g1 = m.loss_and_grad()
    d = dr.data_part(prob, L, th, Xd, ud, w)
    wm, ms = m.flux_loss()
    assert abs(ms - d["msq"]) < dr.LOSSB_TOL * d["msq"] and wm == w * ms
    assert abs(l1[0] - (l0[0] + d["wmsq"])) < TOL * abs(l1[0])
    assert rel(np.asarray(g1) - np.asarray(g0), d["grad"]) < TOL
    # one vector b for all points: a derivative sensor on the last coordinate
    dim = Xd.shape[1]
    e = np.zeros(dim); e[-1] = 1.0
    X = dr.points(prob, 5, 31)
    f = dict(X=X, a=np.zeros(5), b=np.tile(e, (5, 1)), g=np.full(5, 0.25))
    m.set_flux_data(X, f["g"], b=e, weight=2.0)
    m.loss_and_grad()
    fp = fr.flux_part(prob, L, th, f, 2.0)
    assert abs(m.flux_loss()[1] - fp["msf"]) < dr.LOSSB_TOL * fp["msf"]
    m.set_flux_data(None)
    l2, g2 = m.loss_and_grad()
    assert m.flux_loss() == (0.0, 0.0) and np.array_equal(np.asarray(l2), np.asarray(l0)) and np.array_equal(g2, g0)


def test_poisson2d_driver_with_two_neumann_sides():
    from hp_vpinns_amd.drivers import poisson2d
    out = poisson2d.run(Net_layer=[2, 20, 20, 20, 1], N_el_x=2, N_el_y=2, N_bound=20, n_iter=200, verbose=False, neumann_sides="right,top")
    m, his = out["model"], out["loss_his"]
    assert m.X_u_train.shape[0] == 40                              # the points of the two Dirichlet sides
    wm, ms = m.flux_loss()
    print("poisson2d --neumann-sides right,top: loss %.4e -> %.4e, flux loss %.4e, rel L2 %.3e" % (his[0], his[-1], ms, out["rel_l2"]))
    assert np.isfinite(ms) and ms > 0.0 and np.all(np.isfinite(his)) and his[-1] < his[0]


@pytest.fixture(scope="module", autouse=True)
def _report():
    """prints the table of worst errors when the module's last test has run (pytest -rA / -s)"""
    yield
    print("\n| structure | Dirichlet data | n | loss triple | gradient block | msf | forward-only |")
    for (k, wd, n), e in WORST.items():
        if wd == "adam":
            print("| %s | yes | %d | parameters after four Adam steps: %.1e |" % (k, n, e[0]))
        else:
            print("| %s | %s | %d | %.1e | %.1e | %.1e | %.1e |" % ((k, "yes" if wd else "no", n) + e))
