"""Coefficient identification on the variable-coefficient class (hpv_create_ex, hpv_set_trainable, k_project_id) on the device against
tests/ident_reference.py (CPU, fp64; tests/test_ident_host.py proves it); the measured errors are in profiles/identification.md.

Bounds, exactly those of tests/test_gpu_linear.py / test_gpu_nonlinear.py: TOL = 1e-9 on the loss triple, the
residuals, the network gradient per block and every d c_m; STEP_TOL = 1e-8 on parameters and loss after Adam steps, both imported from
tests/test_gpu_generic_point.py."""
import numpy as np
import pytest

import generic_point as gp
import ident_reference as ir
import nonlinear_reference as nr
from cases import rel
from test_gpu_generic_point import STEP_TOL, TOL

pytestmark = pytest.mark.gpu

WORST = {}
_PROBLEMS = {}


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH", "HPV_NO_DEFERRED_ADAM"):
        monkeypatch.delenv(k, raising=False)


def _problem(name):
    """the case's arrays and its reference (loss triple, gradient, R) at the initial parameters, computed once and left unchanged"""
    if name not in _PROBLEMS:
        p = ir.problem(ir.CASES[name])
        fig = ir.conditions(p)                          # the reference alone, first
        _PROBLEMS[name] = (p, ir.reference(p), fig)
    return _PROBLEMS[name]


class Dev:
    """the C-ABI on problem dict `p`: tests/test_gpu_nonlinear.Dev's sequence on a handle of hpv_create_ex, then hpv_set_trainable.
    n_coef None: the problem's; 0 with planes= / nl=: a handle without coefficients (baked-in planes); create_ex=False: hpv_create
    itself (n_coef 0); trainable=False: stop before hpv_set_trainable; shard=(eb, ee): another slice of the same boxes"""

    def __init__(self, p, n_coef=None, planes=None, nl=None, trainable=True, shard=None, create_ex=True):
        from hp_vpinns_amd import _lib
        from hp_vpinns_amd.init import n_params, pad_plan
        from hp_vpinns_amd.testfcn import tables_1d
        self.p, L = p, p["layers"]
        self.nc = nc = p["dirs"].shape[0] if n_coef is None else n_coef
        plan = pad_plan(L, nc)
        self.dev_layers, self.idx = plan if plan is not None else (L, None)
        self.n_dev = n_params(self.dev_layers, nc)
        args = (_lib.PDE_LINEAR1D if p["dim"] == 1 else _lib.PDE_LINEAR2D, 1, _lib.ACT_SIN if p["act"] == "sin" else _lib.ACT_TANH, self.dev_layers)
        kw = dict(lr=1e-3, lossb_weight=p["lbw"], V=0.6)
        self.h = h = _lib.Handle(*args, n_coef=nc, **kw) if create_ex else _PlainHandle(*args, **kw)
        (xi, wx), yr = p["xr"], p["yr"]
        h.set_quadrature(xi, wx, *(yr if yr is not None else (None, None)))
        h.set_tables(tables_1d(p["ntx"], xi), None if yr is None else tables_1d(p["nty"], yr[0]))
        self.eb, self.ee = (p["eb"], p["ee"]) if shard is None else shard
        self.rank0 = shard is None or shard[0] == p["eb"]
        self.populate(trainable)
        self.set_params(p["full"] if nc else p["theta"])

    def _rows(self, a):
        """the columns of a per-point array of the problem's shard that belong to this handle's slice"""
        p = self.p
        nq = a.shape[-1] // (p["ee"] - p["eb"])
        return np.ascontiguousarray(a[..., (self.eb - p["eb"]) * nq:(self.ee - p["eb"]) * nq])

    def populate(self, trainable=True, planes=None, nl=None):
        p, h = self.p, self.h
        h.set_element_boxes(p["boxes"], self.eb, self.ee)
        h.set_rhs(p["F"].reshape(-1))
        if p["nax"] is not None:
            if p["dim"] == 1:
                h.set_active_tests(p["nax"])
            else:
                h.set_active_tests_2d(p["nax"], p["nay"])
        h.set_operator(self._rows(p["planes"] if planes is None else planes))
        nl = p["nl"] if nl is None else nl
        if np.any(nl != 0.0):                            # (a zero base: the handle never hears of hpv_set_nonlinear)
            h.set_nonlinear(self._rows(nl))
        if self.nc and trainable:
            h.set_trainable(self._rows(p["dirs"]))
        if self.rank0 and p["data"] is not None:
            h.set_data(*p["data"])
        if self.rank0 and p["flux"] is not None:
            import flux_reference as fr
            h.set_flux_data(p["flux"]["X"], fr.coef(p["flux"]), p["flux"]["g"], fr.W_F)

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
            assert np.all(g[pad] == 0.0)                # (a padded neuron's gradient entries are exact zeros)
            g = g[self.idx]
        return np.asarray(l3), g

    def residuals(self):
        p = self.p
        return self.h.residuals((self.ee - self.eb) * p["ntx"] * p["nty"]).reshape(-1, p["nty"], p["ntx"])

    def everything(self):
        l3, g = self.loss_and_grad()
        return l3, g, self.residuals()


def _PlainHandle(*args, **kw):
    """a handle made by hpv_create itself (what every caller before hpv_create_ex got)"""
    import ctypes as C
    from hp_vpinns_amd import _lib
    h = _lib.Handle.__new__(_lib.Handle)
    h.lib = _lib.load()
    tmp = _lib.Handle(*args, **kw)                      # (fills a config the usual way)
    h.cfg, h.layers, h.n_owned, h._keep, h.n_coef = tmp.cfg, tmp.layers, None, [], 0
    tmp.close()
    h._h = C.c_void_p()
    assert h.lib.hpv_create(C.byref(h._h), C.byref(h.cfg)) == 0
    return h


def _rel3(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def _kernel(p, nc=None):
    K, _ = ir.n_planes(p["dim"])
    qx, qy = p["xr"][0].size, 1 if p["yr"] is None else p["yr"][0].size
    touched = np.any(p["dirs"][:, K:] != 0.0, axis=(0, 2)) | np.any(p["nl"] != 0.0, axis=1)
    act = [touched[0], touched[1], touched[2], bool(np.any(touched[3:]))]
    terms = ",".join(t for t, on in zip(nr.TERMS, act) if on)
    return "k_project_id<%dx%d/%dx%d%s;nc=%d>" % (qx, qy, p["ntx"], p["nty"], ";" + terms if terms else "", p["dirs"].shape[0] if nc is None else nc)


def _against_reference(tag, d, ref):
    """loss triple, network gradient per block, every d c_m, the forward-only loss and the residuals against the reference; the
    kernel's name; a second call with the same bytes"""
    p = d.p
    l3o, go, Ro = ref
    l3m, gm, Rm = d.everything()
    v, ps = d.h.kernel_variant(), d.h.pass_structure()
    lf = d.h.loss_and_grad(False)[0]
    nth = p["theta"].size
    e3, ef = _rel3(l3m, l3o), _rel3(lf, l3o)
    kb, eb = gp.worst_block(gm[:nth], go[:nth], p["layers"], 0)
    ec = np.abs(gm[nth:] - go[nth:]) / np.abs(go[nth:])
    eR = float(np.linalg.norm(Rm - Ro) / np.linalg.norm(Ro))
    print("%s | %s | %s | loss3 %s | worst block %s %.2e | d c %s | forward-only %s | residuals %.2e" % (tag, v, ps, e3, kb, eb, ec, ef, eR))
    WORST[tag] = (float(e3.max()), float(eb), float(ec.max()), float(ef.max()), eR)
    assert _kernel(p) in v and ps == "separate", (tag, v, ps, _kernel(p))
    assert d.h.lib.hpv_pass_structure(d.h._h) == 0
    assert gm.size == nth + p["dirs"].shape[0]
    assert e3.max() < TOL, (tag, v, "loss triple", l3m, l3o)
    assert eb < TOL, (tag, v, "gradient block", kb, eb)
    assert ec.max() < TOL, (tag, v, "d c", gm[nth:], go[nth:])
    assert ef.max() < TOL, (tag, v, "forward-only pass", lf, l3o)
    assert eR < TOL, (tag, v, "residuals", eR)
    assert np.all(Rm[Ro == 0.0] == 0.0), (tag, "inactive residual entries are exactly 0")
    again = d.everything()
    assert all(np.array_equal(x, y) for x, y in zip((l3m, gm, Rm), again)), (tag, "a second call returns the same bytes, d c included")


# ---- 1, 3: parity at generic points; reproducibility ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ir.CASES))
def test_cases_against_the_reference(name):
    p, ref, fig = _problem(name)
    d = Dev(p)
    _against_reference(name, d, ref)
    v = d.h.kernel_variant()
    if name in ir.SMALL and p["xr"][0].size < 17:      # the layer kernels around the new projection
        wide = p["layers"][1] == 24
        assert ("k_fwd_wide<" in v and "H=24>" in v) if wide else "k_fwd_mfma<" in v, v
    print(name, fig)


def test_padding_points_add_exact_zeros():
    """the 21 x 21 rule's last point per direction has zero weight: loss and gradients are the 20 x 20 rule's, whatever the planes and
    the directions hold there (the reference has no such point: everything is cut to the 20 x 20 points)"""
    import linear_reference as lr
    p, _, _ = _problem("lds-21x21-padded")
    q = dict(p, xr=lr.rule(20), yr=lr.rule(20))
    ne = p["ee"] - p["eb"]
    for k in ("planes", "nl"):
        q[k] = np.ascontiguousarray(p[k].reshape(5, ne, 21, 21)[:, :, :20, :20]).reshape(5, -1)
    q["dirs"] = np.ascontiguousarray(p["dirs"].reshape(-1, 10, ne, 21, 21)[..., :20, :20]).reshape(p["dirs"].shape[0], 10, -1)
    l3o, go, _ = ir.reference(q)
    l3, g = Dev(p).loss_and_grad()
    nth = p["theta"].size
    assert _rel3(l3, l3o).max() < TOL and gp.block_rel(g[:nth], go[:nth], p["layers"]) < TOL
    assert np.max(np.abs(g[nth:] - go[nth:]) / np.abs(go[nth:])) < TOL


# ---- 2: four Adam steps over network and coefficients, under graphs and without ---------------------------------------------------------
@pytest.mark.parametrize("graphs", [True, False])
def test_four_adam_steps(graphs, monkeypatch):
    if not graphs:
        monkeypatch.setenv("HPV_NO_GRAPH", "1")
    p, _, _ = _problem("2d-h8-counts-flux-shared")
    d = Dev(p)
    l3 = d.h.step(4, True)
    assert bool(d.h.graphs_in_use()) == graphs and _kernel(p) in d.h.kernel_variant()
    th4, _, _ = ir.adam_trajectory(p, 4)
    l3o = ir.reference(p, th4)[0]
    nth = p["theta"].size
    got = d.params()
    ep, ec, el = rel(got[:nth], th4[:nth]), float(np.max(np.abs(got[nth:] - th4[nth:]) / np.abs(th4[nth:]))), _rel3(l3, l3o)
    moved = np.abs(th4[nth:] - p["c0"]) / np.abs(p["c0"])
    print("four Adam steps (graphs %s): parameters %.2e | coefficients %.2e (they moved by %s) | loss %s" % (graphs, ep, ec, moved, el))
    WORST["adam 4, graphs %s" % graphs] = (float(ep), ec, float(el.max()))
    assert moved.min() > 1e3 * STEP_TOL                 # the reference alone: a coefficient that is not updated cannot pass
    assert ep < STEP_TOL and ec < STEP_TOL and el.max() < STEP_TOL
    hist, c_first = d.h.history_read(4)
    assert abs(c_first[0] - p["c0"][0]) == 0.0          # the fourth column: theta[P], the first coefficient, as each forward pass saw it
    assert abs(c_first[1] - ir.adam_trajectory(p, 1)[0][nth]) < STEP_TOL * abs(c_first[1])


# ---- 4: existing paths unchanged ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d-h8", "1d-sin"])
def test_create_ex_with_zero_is_create_byte_for_byte(name):
    p, _, _ = _problem(name)
    a, b = Dev(p, n_coef=0), Dev(p, n_coef=0, create_ex=False)
    assert a.h.num_params() == b.h.num_params() == a.n_dev
    for x, y in zip(a.everything(), b.everything()):
        assert np.array_equal(x, y)
    la, lb = a.h.step(4, True), b.h.step(4, True)
    assert np.array_equal(la, lb) and np.array_equal(a.h.get_params(), b.h.get_params()) and np.array_equal(a.h.get_state(), b.h.get_state())
    assert "k_project_nl<" in a.h.kernel_variant() and a.h.kernel_variant() == b.h.kernel_variant()


# ---- 5: baked-in equivalence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d-h8", "2d-nl-over-zero-base", "1d-sin"])
def test_baked_in_planes_agree(name):
    p, _, _ = _problem(name)
    l3, g = Dev(p).loss_and_grad()
    planes, nl = ir.effective(p, p["c0"])
    q = dict(p, planes=planes, nl=nl)
    b = Dev(q, n_coef=0)
    l3b, gb = b.loss_and_grad()
    assert "k_project_nl<" in b.h.kernel_variant()
    nth = p["theta"].size
    e = (float(_rel3(l3, l3b).max()), float(gp.block_rel(g[:nth], gb, p["layers"])))
    print("baked-in %s: loss %.2e, network gradient block %.2e" % ((name,) + e))
    assert max(e) < TOL and gb.size == nth


# ---- 6: the caller-driven multi-GPU pieces in one process --------------------------------------------------------------------------------
def test_two_shards_summed_on_the_host_match_the_single_handle_step():
    """two handles own the two halves of the shard, each runs hpv_forward_backward; their reduce buffers (torch views of the library's
    own memory, as the multi-GPU path takes them) are summed on the host and written back, hpv_apply_adam runs on each: buffer length
    and slot layout [grad (P) | d c (8) | lossv | w*lossb | msq | pad]"""
    import torch
    from hp_vpinns_amd.dist import Reducer
    p, ref, _ = _problem("2d-h24-nc8")                  # owns boxes 1 .. 3 of four; data and flux live on the first shard
    one = Dev(p)
    one.h.step(1, False)
    want = one.h.get_params()
    shards = [Dev(p, shard=(1, 2)), Dev(p, shard=(2, 4))]
    views = []
    for s in shards:
        s.h.forward_backward()
        s.h.sync()
        ptr, n = s.h.reduce_buffer()
        assert n == s.n_dev + 4
        views.append(Reducer(ptr, n, 0).tensor)
    total = sum(v.cpu().numpy() for v in views)
    nd = shards[0].n_dev
    l3o, go, _ = ref
    assert abs(total[nd] - l3o[2]) < TOL * abs(l3o[2])                                                # lossv sits behind the 8 slots
    assert np.max(np.abs(total[nd - 8:nd] - go[-8:]) / np.abs(go[-8:])) < TOL                         # ... which hold d c, summed over the shards
    for s, v in zip(shards, views):
        v.copy_(torch.from_numpy(total))
        torch.cuda.synchronize()
        s.h.apply_adam()
        s.h.sync()
        got = s.h.get_params()
        e = float(np.max(np.abs(got - want) / np.where(want == 0.0, 1.0, np.abs(want))))
        print("shard %s after hpv_apply_adam against the single-handle step: %.2e" % ((s.eb, s.ee), e))
        assert e < STEP_TOL and np.all(got[-8:] != s.p["c0"])


# ---- 7: state ----------------------------------------------------------------------------------------------------------------------------
def test_state_continues_bit_exactly():
    p, _, _ = _problem("2d-h8")
    a = Dev(p)
    a.h.step(3, False)
    st = a.h.get_state()
    assert st.size == 3 * a.n_dev + 2
    b = Dev(p)
    b.h.set_state(st)
    assert np.array_equal(b.h.get_state(), st)
    a.h.step(3, False)
    b.h.step(3, False)
    sa, sb = a.h.get_state(), b.h.get_state()
    nc = p["dirs"].shape[0]
    moments = sa[a.n_dev:3 * a.n_dev].reshape(2, -1)[:, -nc:]
    assert np.array_equal(sa, sb) and np.all(moments != 0.0)        # the coefficients' moments are carried, and live


# ---- 8: refusals leave the handle usable -------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from hp_vpinns_amd import _lib
    p, ref, _ = _problem("2d-h8")
    d = Dev(p)

    def refused(call, code=-1, message=None):
        with pytest.raises(_lib.HpvError) as e:
            call()
        assert e.value.code == code and (message is None or message in str(e.value)), (e.value.code, str(e.value))

    def usable():
        l3, g = d.loss_and_grad()
        assert _rel3(l3, ref[0]).max() < TOL and np.max(np.abs(g[-2:] - ref[1][-2:]) / np.abs(ref[1][-2:])) < TOL and _kernel(p) in d.h.kernel_variant()
    # n_coef on a Poisson handle, and above 8
    refused(lambda: _lib.Handle(_lib.PDE_POISSON2D, 1, _lib.ACT_TANH, [2, 8, 8, 1], n_coef=1))
    refused(lambda: _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, [2, 8, 8, 1], n_coef=9))
    refused(lambda: _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, [2, 8, 8, 1], n_coef=-1))
    bad = p["dirs"].copy()
    bad[1, 4, 5] = np.nan
    inf = p["dirs"].copy()
    inf[0, 9, 0] = np.inf
    for call in (lambda: d.h.set_trainable(p["dirs"][:, :, :-1]), lambda: d.h.set_trainable(p["dirs"][:1]), lambda: d.h.set_trainable(bad),
                 lambda: d.h.set_trainable(inf), lambda: d.h.set_trainable(None)):
        refused(call)
        usable()
    # a pass before hpv_set_trainable: -3, and the handle works once it is called
    e = Dev(p, trainable=False)
    refused(lambda: e.h.loss_and_grad(True), -3, "hpv_set_trainable has not been called")
    refused(lambda: e.h.step(1, False), -3, "hpv_set_trainable")
    e.h.set_trainable(p["dirs"])
    assert _rel3(e.loss_and_grad()[0], ref[0]).max() < TOL
    # new elements orphan the directions
    d.h.set_element_boxes(p["boxes"], p["eb"], p["ee"])
    d.h.set_operator(p["planes"])
    d.h.set_nonlinear(p["nl"])
    refused(lambda: d.h.loss_and_grad(True), -3, "hpv_set_trainable has not been called")
    refused(lambda: d.h.loss_and_grad(False), -3, "hpv_set_trainable")
    d.h.set_trainable(p["dirs"])
    _against_reference("after new elements", d, ref)
    # before hpv_set_elements: -3
    from hp_vpinns_amd.testfcn import tables_1d
    f = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, d.dev_layers, n_coef=2)
    f.set_quadrature(*p["xr"], *p["yr"])
    f.set_tables(tables_1d(p["ntx"], p["xr"][0]), tables_1d(p["nty"], p["yr"][0]))
    refused(lambda: f.set_trainable(p["dirs"]), -3)
    # hpv_set_trainable on an n_coef = 0 handle
    z = Dev(p, n_coef=0)
    before = z.everything()
    refused(lambda: z.h.set_trainable(p["dirs"]))
    assert all(np.array_equal(x, y) for x, y in zip(before, z.everything()))


# ---- the Python classes ------------------------------------------------------------------------------------------------------------------
def test_python_class_carries_the_coefficients(tmp_path):
    """VPINNNonlinear(trainable=...) on a two-element Burgers setting with an unknown viscosity and an unknown reaction rate: loss and
    gradient (d c included) are the reference's for the model's own fields; get_params, coefficients() and checkpoints carry the
    slots behind the (padded) network; set_operator hands the directions again"""
    from hp_vpinns_amd.vpinn import VPINNNonlinear
    tr = [dict(name="nu", init=0.1, kappa=(-1.0, 0.0)), dict(name="rate", init=-0.4, sigma=lambda P: 1.0 + P[:, 0] ** 2, cubic=0.5)]
    Xb = np.stack([np.linspace(-1.0, 1.0, 9), np.zeros(9)], 1)
    kw = dict(grid_x=np.linspace(-1.0, 1.0, 3), grid_y=np.linspace(0.0, 1.0, 2), n_quad=(6, 5), n_test=(4, 3), kappa=(0.0, 0.0), beta=(0.0, 1.0),
              advection=(1.0, 0.0), f=lambda P: np.sin(P[:, 0]) * P[:, 1], X_u_train=Xb, u_train=np.sin(np.pi * Xb[:, 0]), lossb_weight=3.0,
              trainable=tr)
    m = VPINNNonlinear([2, 8, 8, 1], **kw)
    assert m.coefficients() == {"nu": 0.1, "rate": -0.4} and m.get_params().size == 2 * 8 + 8 + 8 * 8 + 8 + 8 + 1 + 2
    p = ir.from_model(m)
    l3, g = m.loss_and_grad()
    l3o, go, _ = ir.reference(p)
    e = (float(_rel3(l3, l3o).max()), float(gp.block_rel(g[:-2], go[:-2], p["layers"])), float(np.max(np.abs(g[-2:] - go[-2:]) / np.abs(go[-2:]))))
    print("class: loss %.2e, network gradient block %.2e, d c %.2e | %s" % (e + (m.h.kernel_variant(),)))
    assert max(e) < TOL and "k_project_id<6x5/4x3;u3,adv;nc=2>" in m.h.kernel_variant()
    m.train(4)
    full4, _, _ = ir.adam_trajectory(p, 4)
    assert m.h.graphs_in_use() and rel(m.get_params(), full4) < STEP_TOL
    c = m.coefficients()
    assert abs(c["nu"] - full4[-2]) < STEP_TOL * abs(full4[-2]) and c["nu"] != 0.1 and c["rate"] != -0.4
    m.save_checkpoint(tmp_path / "ident")
    m2 = VPINNNonlinear([2, 8, 8, 1], **kw)
    m2.load_checkpoint(tmp_path / "ident")
    assert m2.coefficients() == c and np.array_equal(m2.h.get_state(), m.h.get_state())
    m.set_operator(sigma=0.25)                       # new base planes: the directions are handed again, the pass is not refused
    q = ir.from_model(m)
    assert _rel3(m.loss(), ir.reference(q)[0]).max() < TOL and not np.array_equal(q["planes"], p["planes"])
    m.set_mesh(m._mesh)                              # ... and after new elements
    assert _rel3(m.loss(), ir.reference(q)[0]).max() < TOL
    with pytest.raises(ValueError):
        VPINNNonlinear([2, 8, 8, 1], **dict(kw, trainable=[dict(name="x", init=1.0, kapa=1.0)]))


# ---- 9: the drivers at their smallest settings ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["conductivity", "burgers-nu"])
def test_drivers_recover_the_coefficients(name):
    """drivers/identify.py at SMALLEST for SMALLEST_STEPS Adam steps against the CPU reference's own Adam trajectory on the same
    problem from the same initial parameters.  The step counts were picked from that reference (the driver's comment): its errors are
    asserted below a fifth of the initial ones here.  Bound: each coefficient's error on the device at most twice the reference's
    (the rule of test_gpu_linear.test_python_class_and_boundary_layer_driver_converge)."""
    from hp_vpinns_amd.drivers import identify as drv
    kw = dict(drv.SMALLEST[name])
    s = drv.setup(kw.pop("problem"), **kw)
    n = drv.SMALLEST_STEPS[name]
    out = drv.run(s, n_iter=n, LR=drv.SMALLEST_LR, verbose=False)
    m = out["model"]
    v = m.h.kernel_variant()
    assert "k_project_id<" in v and ";nc=%d>" % len(s["true"]) in v and m.h.graphs_in_use(), v
    p = ir.from_model(m, m._init_params)
    ref, _, _ = ir.adam_trajectory(p, n, lr_=drv.SMALLEST_LR)
    names = list(s["true"])
    true = np.array([s["true"][k] for k in names])
    e0 = np.abs(p["c0"] - true)
    e_ref = np.abs(ref[-true.size:] - true)
    e_dev = np.abs(np.array([out["coefficients"][k] for k in names]) - true)
    print("%s, %d steps at LR %g: coefficient errors %s on the device, %s on the CPU reference's trajectory (initially %s); parameters %.2e"
          % (name, n, drv.SMALLEST_LR, e_dev, e_ref, e0, rel(m.get_params(), ref)))
    WORST["driver " + name] = tuple(float(x) for x in np.concatenate([e_dev, e_ref]))
    assert np.all(e_ref < e0 / 5.0), (e_ref, e0)         # the reference alone: the run is a recovery
    assert np.all(e_dev < 2.0 * e_ref), (e_dev, e_ref)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n| case | loss triple | gradient block | d c | forward-only | residuals |")
    for k, e in WORST.items():
        print("| %s | %s |" % (k, " | ".join("%.1e" % x for x in e)))
