"""Every forward / reverse pair of the per-layer MFMA kernels against a CPU reference, at generic points: one case per row of
tests/shape_matrix.py -- k_fwd_mfma / k_bwd_mfma (H = 20) and k_fwd_wide / k_bwd_wide (H = 24 .. 64) for every channel set a public
configuration reaches, L = 1 .. 6 hidden layers at H <= 32 and 1 .. 4 beyond -- plus zero-padded networks checked in the DEVICE's
parameter layout.  The strong-form scheme is the main probe: its reference needs no quadrature, projection or grid.  Every bias is
non-zero, the collocation set is one full tile and a one-point tail, the variational grids are warped.

Every case asserts, in this order: the exact k_fwd_*<..> / k_bwd_*<..> names and backend() == "mfma"; each entry of the loss triple
within 1e-9; the gradient within 1e-9 PER PARAMETER BLOCK (generic_point.block_errors), d/d epsilon also on its own; the forward-only
loss() within 1e-9; a second loss_and_grad() bit-equal to the first; the parameters after four eager TF1-Adam steps (forward_backward
+ apply_adam: no graph is captured) within 1e-8, epsilon on its own; for the variational cases the residuals within 1e-9 of their
norm.  The figures are DESIGN section 2's, as in test_gpu_generic_point.py.  tests/test_shape_matrix_host.py shows on the CPU that
every case is well posed (two restatements of the reference within 1e-11 per block).

The file's last test checks that the instantiations reached cover every row of the table.  (profiles/shape_matrix.md: the measured errors of every case.)"""
import numpy as np
import pytest

import generic_point as gp
import shape_matrix as sm
from cases import rel

pytestmark = pytest.mark.gpu

TOL = 1e-9
STEP_TOL = 1e-8
REACHED = {}        # (forward name, reverse name) -> the cases that ran the pair
WORST = {}          # case -> (loss, block, step) errors, printed when the module's last test has run

MATRIX, PADDED = sm.matrix_cases(), sm.padded_cases()


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH"):
        monkeypatch.delenv(k, raising=False)


def _pair(c, monkeypatch):
    inp = sm.inputs(c)
    o = sm.reference(c, inp)
    for k, v in c["env"].items():       # (before the handle exists: the library reads the switches at creation)
        monkeypatch.setenv(k, v)
    return o, sm.product(c, inp), inp


def _eps_close(a, b, tol):
    return abs(a - b) < tol * abs(b)


def _check(c, o, m, inp, after_first=None):
    name, layers, n_extra = c["name"], c["layers"], c["n_extra"]
    l3o, go = o.loss_and_grad()
    l3m, gm = m.loss_and_grad()
    v = m.h.kernel_variant()
    assert c["fwd"] in v and c["bwd"] in v, (name, "wanted", c["fwd"], c["bwd"], "ran", v)
    assert m.backend() == "mfma", (name, m.backend())
    REACHED.setdefault((c["fwd"], c["bwd"]), []).append(name)
    rm = m.h.residuals(inp["n_res"]) if c["kind"] == "var" else None
    if after_first is not None:
        after_first()
    l3o, l3m = np.asarray(l3o, dtype=np.float64), np.asarray(l3m, dtype=np.float64)
    e3 = np.abs(l3m - l3o) / np.abs(l3o)
    kb, eb = gp.worst_block(gm, go, layers, n_extra)
    print("%s | %s | loss3 err %s | worst block %s %.2e (global %.2e)" % (name, v, e3, kb, eb, rel(gm, go)))
    assert e3.max() < TOL, (name, v, "loss triple", l3m, l3o)
    assert eb < TOL, (name, v, "gradient block", kb, eb, gp.block_errors(gm, go, layers, n_extra))
    if n_extra:
        assert _eps_close(gm[-1], go[-1], TOL), (name, v, "d/d epsilon", gm[-1], go[-1])
    lf = np.asarray(m.loss(), dtype=np.float64)
    assert (np.abs(lf - l3o) / np.abs(l3o)).max() < TOL, (name, v, "forward-only loss", lf, l3o)
    l3r, gr = m.loss_and_grad()
    assert np.array_equal(np.asarray(l3r), l3m) and np.array_equal(gr, gm), (name, v, "a second loss_and_grad differs from the first")
    for _ in range(4):
        o.adam_step()
        m.h.forward_backward()
        m.h.apply_adam()
    pm, po = m.get_params(), o.get_params()
    ep = rel(pm, po)
    print("%s | four Adam steps: parameters %.2e%s" % (name, ep, " | epsilon %.12f %.12f" % (pm[-1], po[-1]) if n_extra else ""))
    assert ep < STEP_TOL, (name, v, "parameters after four Adam steps", ep)
    if n_extra:
        assert _eps_close(pm[-1], po[-1], STEP_TOL), (name, v, "epsilon after four Adam steps", pm[-1], po[-1])
    er = 0.0
    if rm is not None:
        ro = np.asarray(o.last_first_R, dtype=np.float64).reshape(-1)
        er = rel(rm, ro)
        print("%s | residuals %.2e" % (name, er))
        assert er < TOL, (name, v, "residuals", er)
    WORST[name] = (float(e3.max()), eb, ep, er)


class _KeepsFirstResiduals:
    """the vectorised oracle overwrites .last at every evaluation: the residuals of the FIRST one are what the product's were read
    at"""

    def __init__(self, o):
        self._o, self.last_first_R = o, None

    def loss_and_grad(self):
        out = self._o.loss_and_grad()
        if self.last_first_R is None and getattr(self._o, "last", None):
            self.last_first_R = np.array(self._o.last["R"], dtype=np.float64)
        return out

    def __getattr__(self, k):
        return getattr(self._o, k)


@pytest.mark.parametrize("c", MATRIX, ids=[c["name"] for c in MATRIX])
def test_layer_kernel_pair_at_a_generic_point(c, monkeypatch):
    o, m, inp = _pair(c, monkeypatch)
    _check(c, _KeepsFirstResiduals(o), m, inp)


# ---- zero-padded networks, in the device layout -------------------------------------------------------------------------------------
def _padding_is_zero(m, what, vec, parts=1):
    """every entry of `vec` (parts x num_params, device layout) outside m._pad_idx is exactly 0.0"""
    P = m.h.num_params()
    pad = np.ones(P, dtype=bool)
    pad[m._pad_idx] = False
    assert pad.sum() > 0 and vec.size >= parts * P
    for k in range(parts):
        bad = np.flatnonzero(vec[k * P:(k + 1) * P][pad] != 0.0)
        assert bad.size == 0, (what, "part", k, "non-zero padding entries", bad[:8], vec[k * P:(k + 1) * P][pad][bad[:8]])


@pytest.mark.parametrize("c", PADDED, ids=[c["name"] for c in PADDED])
def test_zero_padded_network_stays_exactly_zero_in_the_device_layout(c, monkeypatch):
    """init.pad_plan promises exactness: a padded neuron outputs act(0) = 0 with zero tangents, every gradient entry that belongs to
    padding is exactly zero and TF1-Adam leaves it there.  Here with every bias non-zero, in the layout the device holds: parameters
    and the m / v parts of the state before the first step, the packed gradient after loss_and_grad, all three after eight steps --
    beside the assertions of every matrix case in the user's layout."""
    o, m, inp = _pair(c, monkeypatch)
    assert m._pad_idx is not None and m.h.num_params() > m.get_params().size
    assert np.array_equal(m.h.get_params()[m._pad_idx], inp["th"])
    _padding_is_zero(m, "parameters before the first step", m.h.get_params())
    _padding_is_zero(m, "m, v before the first step", m.h.get_state()[m.h.num_params():], parts=2)

    def packed_gradient():
        _padding_is_zero(m, "packed gradient", m.h.loss_and_grad(True)[1])
    _check(c, _KeepsFirstResiduals(o), m, inp, after_first=packed_gradient)
    for _ in range(4):                      # (four were taken in _check)
        m.h.forward_backward()
        m.h.apply_adam()
    assert m.h.updates_applied() == 8
    st = m.h.get_state()
    _padding_is_zero(m, "parameters after eight steps", m.h.get_params())
    _padding_is_zero(m, "theta, m, v of the state after eight steps", st, parts=3)
    _padding_is_zero(m, "packed gradient after eight steps", m.h.loss_and_grad(True)[1])
    assert np.all(st[m.h.num_params():2 * m.h.num_params()][m._pad_idx] != 0.0)      # (the moments of the real entries moved)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """prints, when the module's last test has run, the errors of every case (pytest -rA / -s)"""
    yield
    print("\ncase | loss | worst block | four steps | residuals")
    for k, e in WORST.items():
        print("  %-36s %.2e %.2e %.2e %.2e" % ((k,) + e))
    if WORST:
        w = np.array(list(WORST.values()))
        print("worst over %d cases: loss %.2e, block %.2e, step %.2e, residuals %.2e" % ((len(WORST),) + tuple(w.max(axis=0))))


def test_zz_every_row_of_the_table_was_reached():
    """Runs last in the file: the cases above, together, launched every (channel set, H, L) pair of the table (on its own, e.g. under
    -k, it fails: it judges the whole file).  The pairs no public configuration reaches are shape_matrix.DEAD_SETS."""
    assert REACHED, "run the whole file: this test judges what the cases above reached"
    want = {(c["fwd"], c["bwd"]) for c in MATRIX}
    missing = sorted(want - set(REACHED))
    assert not missing, (len(missing), missing[:10])
    cells = {(c["set"], c["H"], c["L"]) for c in MATRIX}
    assert cells == {(s, H, L) for s in sm.INSTANTIATED_SETS if s not in sm.DEAD_SETS for H, L in sm.FULL}
    print("reached %d forward / reverse pairs in %d cases; dead channel sets: %s" % (len(REACHED), len(WORST), sm.DEAD_SETS))
