#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by RUNNING the reference's own numpy code.

Run in the build container only (needs /root/reference; the GPU box never sees it):

    python tests/golden/make_golden.py                  (--search-seeds: print the GRAPH_SEEDS block instead of writing graph files)

What is executed from the reference (nothing is copied -- only its *outputs* are stored):
  * `Utilities/GaussJacobiQuadRule_V3.py`  -> Jacobi values, GLL nodes / weights
  * the unbound methods `VPINN.Test_fcn / Test_fcnx / dTest_fcn` of the three drivers
    (imported with `tensorflow` / `pyDOE` stubs; their `__main__` blocks do not run)
  * the `__main__` *set-up* blocks of the three drivers (everything before `model = VPINN(`),
    exec'd TF-free from the source file where it lies, with hyper-parameters pinned to the
    BASELINE.json shapes -> grids, F_ext_total, boundary sets, test data.

  * the three `VPINN` classes themselves (`gen_graph`): constructed from the set-up blocks' arrays with the module globals the
    `__main__` blocks would set, on `tf1_shim.py` installed as `tensorflow` -- a lazy expression graph over torch fp64 that stands
    in for the 24 `tf` symbols the scripts use.  Every line of the class bodies executes: loss, tf.gradients, AdamOptimizer,
    train(), predict().  -> `<problem>_<tag>_graph.npz`: theta0, loss triple, gradient, the loss after each of GRAPH_K updates, the
    parameters after them, a strided prediction (numbers only).  Poisson-2D runs train(K) itself, Poisson-1D train(1, tresh) K times
    (it records at it % 10 == 0 only), AdvDiff its loop body through sess.run (train() cannot return below 11 iterations).

The shim is NOT TensorFlow (no wheel here, no network): what its ops compute stands in for TF1 by documentation, checked by the
shim tests of tests/test_oracle.py.  What is pinned now is the text of the class bodies -- index order of the test-function loops,
Jacobian factors, mean-then-sum, the boundary weight, which variables Adam sees, update-then-read in train() -- which before was a
hand transcription (oracle/vpinn_oracle.py) nobody had executed.  A ragged Poisson-2D case (N_test_x = [4, 2, 3]) is not generated:
the set-up block reshapes F_ext_total to [NE_x, NE_y, N_test_y[0], N_test_x[0]] (P2:414) and raises on unequal blocks.

`pyDOE.lhs` is stubbed with `hp_vpinns_amd.sampling.lhs` (published classic-LHS algorithm);
the sampled points are stored in the fixtures and treated as inputs.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REF, "Utilities"))

from hp_vpinns_amd.sampling import lhs  # noqa: E402

P1 = os.path.join(REF, "main/Poisson-1D/hp-VPINN-Poisson-1D.py")
P2 = os.path.join(REF, "main/Poisson-2D/hp-VPINN-Poisson-2D.py")
P3 = os.path.join(REF, "main/AdvDiff-Identification/hp-VPINN-AdvDiff-Identification.py")


def _install_stubs():
    tf = types.ModuleType("tensorflow")
    tf.set_random_seed = lambda s: None
    sys.modules["tensorflow"] = tf
    pd = types.ModuleType("pyDOE")
    pd.lhs = lhs
    sys.modules["pyDOE"] = pd
    import matplotlib
    matplotlib.use("Agg")


def _import(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Pinned(dict):
    """Namespace whose pinned names ignore re-assignment (hyper-parameter override)."""

    def __init__(self, base, pinned):
        super().__init__(base)
        self._pinned = dict(pinned)
        for k, v in pinned.items():
            dict.__setitem__(self, k, v)

    def __setitem__(self, k, v):
        if k in self._pinned:
            return
        dict.__setitem__(self, k, v)


def _main_setup_source(path, stop_marker="model = VPINN(", start_marker='if __name__ == "__main__":'):
    lines = open(path).read().split("\n")
    i0 = next(i for i, l in enumerate(lines) if l.startswith(start_marker))
    i1 = next(i for i, l in enumerate(lines) if i > i0 and stop_marker in l)
    return lines[i0 + 1:i1]


def _exec_block(lines, ns, fname):
    # the blocks contain column-0 comments, so dedent() cannot be used: keep the indentation
    # and hang the block under an `if True:` instead.
    src = "if True:\n" + "\n".join(lines) + "\n    pass\n"
    exec(compile(src, fname, "exec"), ns)


def gen_quadrature(out):
    import GaussJacobiQuadRule_V3 as Q
    d = {}
    for q in (5, 10, 20, 80):
        x, w = Q.GaussLobattoJacobiWeights(q, 0, 0)
        d[f"gll_x_{q}"] = x
        d[f"gll_w_{q}"] = w
    xs = np.linspace(-1, 1, 41)
    d["jac_x"] = xs
    for (n, a, b) in [(0, 0, 0), (1, 0, 0), (2, 0, 0), (7, 0, 0), (61, 0, 0), (5, 1, 1),
                      (60, 1, 1), (3, 2, 2), (59, 2, 2)]:
        d[f"jac_{n}_{a}_{b}"] = Q.Jacobi(n, a, b, xs)
    d["djac_6_0_0_2"] = Q.DJacobi(6, 0, 0, xs, 2)
    gx, gw = Q.GaussJacobiWeights(7, 0, 0)
    d["gj_x_7"], d["gj_w_7"] = gx, gw
    np.savez_compressed(os.path.join(out, "quadrature.npz"), **d)


def gen_testfcn(out, m1, m2, m3):
    import GaussJacobiQuadRule_V3 as Q
    d = {}
    for (nt, q) in [(60, 80), (5, 10), (10, 20)]:
        x = Q.GaussLobattoJacobiWeights(q, 0, 0)[0][:, None]
        t = m1.VPINN.Test_fcn(None, nt, x)
        d1, d2 = m1.VPINN.dTest_fcn(None, nt, x)
        d[f"phi_{nt}_{q}"], d[f"dphi_{nt}_{q}"], d[f"d2phi_{nt}_{q}"] = t, d1, d2
    # the 2-D / AdvDiff classes carry their own copies: check they agree on one shape
    x = Q.GaussLobattoJacobiWeights(10, 0, 0)[0][:, None]
    d["p2_phix_5_10"] = m2.VPINN.Test_fcnx(None, 5, x)
    d["p2_phiy_5_10"] = m2.VPINN.Test_fcny(None, 5, x)
    d["p2_dphi_5_10"], d["p2_d2phi_5_10"] = m2.VPINN.dTest_fcn(None, 5, x)
    d["p3_phi_5_10"] = m3.VPINN.Test_fcn(None, 5, x)
    d["p3_dphi_5_10"], d["p3_d2phi_5_10"] = m3.VPINN.dTest_fcn(None, 5, x)
    xb = np.array([[-1.0], [1.0]])
    d["dphi_edge_60"], d["d2phi_edge_60"] = m1.VPINN.dTest_fcn(None, 60, xb)
    np.savez_compressed(os.path.join(out, "testfcn.npz"), **d)


def gen_p1(out, tag, pinned):
    np.random.seed(1234)
    base = {"__name__": "p1_setup", "np": np, "lhs": lhs}
    import GaussJacobiQuadRule_V3 as Q
    base.update(Jacobi=Q.Jacobi, DJacobi=Q.DJacobi, GaussLobattoJacobiWeights=Q.GaussLobattoJacobiWeights,
                GaussJacobiWeights=Q.GaussJacobiWeights)
    ns = Pinned(base, pinned)
    _exec_block(_main_setup_source(P1), ns, P1)
    keep = dict(grid=ns["grid"], F_ext_total=ns["F_ext_total"], U_ext_total=ns["U_ext_total"],
                X_quad_train=ns["X_quad_train"], W_quad_train=ns["W_quad_train"],
                X_u_train=ns["X_u_train"], u_train=ns["u_train"],
                X_f_train=ns["X_f_train"], f_train=ns["f_train"],
                X_test=ns["X_test"], u_test=ns["u_test"],
                N_testfcn=np.int64(ns["N_testfcn"]), N_Quad=np.int64(ns["N_Quad"]),
                LR=np.float64(ns["LR"]), var_form=np.int64(ns["var_form"]),
                lossb_weight=np.float64(ns["lossb_weight"]),
                Net_layer=np.asarray(ns["Net_layer"], dtype=np.int64))
    np.savez_compressed(os.path.join(out, f"poisson1d_{tag}.npz"), **keep)
    return ns


def gen_p2(out, tag, pinned, store_test=False):
    np.random.seed(1234)
    import GaussJacobiQuadRule_V3 as Q
    base = {"__name__": "p2_setup", "np": np, "lhs": lhs, "Jacobi": Q.Jacobi, "DJacobi": Q.DJacobi,
            "GaussLobattoJacobiWeights": Q.GaussLobattoJacobiWeights}
    ns = Pinned(base, pinned)
    _exec_block(_main_setup_source(P2), ns, P2)
    keep = dict(grid_x=ns["grid_x"], grid_y=ns["grid_y"], F_ext_total=ns["F_ext_total"],
                XY_quad_train=ns["XY_quad_train"], WXY_quad_train=ns["WXY_quad_train"],
                X_u_train=ns["X_u_train"], u_train=ns["u_train"],
                X_f_train=ns["X_f_train"], f_train=ns["f_train"],
                N_test_x=np.asarray(ns["N_test_x"]), N_test_y=np.asarray(ns["N_test_y"]),
                N_quad=np.int64(ns["N_quad"]), var_form=np.int64(ns["var_form"]),
                Net_layer=np.asarray(ns["Net_layer"], dtype=np.int64),
                X_test_shape=np.asarray(ns["X_test"].shape),
                X_test_head=ns["X_test"][:500], u_test_head=ns["u_test"][:500],
                u_test_sum=np.float64(ns["u_test"].sum()))
    if store_test:
        keep["X_test_sub"] = ns["X_test"][::37]
        keep["u_test_sub"] = ns["u_test"][::37]
    np.savez_compressed(os.path.join(out, f"poisson2d_{tag}.npz"), **keep)
    return ns


def gen_p3(out, tag, pinned, m3):
    np.random.seed(1234)
    import GaussJacobiQuadRule_V3 as Q
    base = {k: getattr(m3, k) for k in ("LR", "Opt_Niter", "Opt_tresh", "var_form", "gamma", "epsilon",
                                        "V", "T", "Net_layer", "N_el_x", "N_el_t", "N_test_x",
                                        "N_test_t", "N_quad", "N_bound")}
    base.update({"__name__": "p3_setup", "np": np, "lhs": lhs, "Jacobi": Q.Jacobi, "DJacobi": Q.DJacobi,
                 "GaussLobattoJacobiWeights": Q.GaussLobattoJacobiWeights})
    ns = Pinned(base, pinned)
    lines = _main_setup_source(P3)
    # P3:451 (np.asarray of the ragged test grid) raises under numpy 2.x because u_ext returns
    # a (1,1) array for t != 0 and a scalar for t == 0 (P3:434-443); run the block in two
    # pieces around it and evaluate the test grid point-wise instead.
    i_a = next(i for i, l in enumerate(lines) if l.strip().startswith("delta_test = 0.01"))
    i_b = next(i for i, l in enumerate(lines) if l.strip().startswith("#### Interior training points"))
    _exec_block(lines[:i_a], ns, P3)
    u_ext = ns["u_ext"]
    xtest = np.linspace(-1, 1, 256)
    ttest = np.arange(0, ns["T"] + 0.01, 0.01)
    xs, ts = xtest[::8], ttest[::5]
    ug = np.array([[float(np.ravel(u_ext(x, t))[0]) for x in xs] for t in ts])
    XT_test = np.stack([np.tile(xtest, len(ttest)), np.repeat(ttest, len(xtest))], axis=1)
    ns["XT_test"] = XT_test  # what P3:454-458 would produce (x fastest)
    _exec_block(lines[i_b:], ns, P3)
    keep = dict(grid_x=ns["grid_x"], grid_t=ns["grid_t"],
                XT_u_train=ns["XT_u_train"], u_train=ns["u_train"], XT_f_train=ns["XT_f_train"],
                T_quad=ns["T_quad"], WT_quad=ns["WT_quad"],
                XT_quad_train=ns["XT_quad_train"][:2000], WXT_quad_train=ns["WXT_quad_train"][:2000],
                N_test_x=np.asarray(ns["N_test_x"]), N_test_t=np.asarray(ns["N_test_t"]),
                N_quad=np.int64(ns["N_quad"]), var_form=np.int64(ns["var_form"]),
                V=np.float64(ns["V"]), epsilon_exact=np.float64(ns["epsilon"]), LR=np.float64(ns["LR"]),
                Net_layer=np.asarray(ns["Net_layer"], dtype=np.int64),
                uext_x=xs, uext_t=ts, uext_grid=ug)
    np.savez_compressed(os.path.join(out, f"advdiff_{tag}.npz"), **keep)
    return ns


# ---- the reference's own VPINN classes, executed on tf1_shim ------------------------------------------------------------------------
GRAPH_K = 6                      # Adam updates per case
GRAPH_PERTURB = 0.3              # N(0,1) scale added to every weight and bias of tests/cases.theta0 (no bias stays zero)
GRAPH_MAX_TRIES = 5              # seeds tried per case: base, base + 1000, ...
TERM_FLOOR = 1e-3                # each loss term's share of the loss
MASK_REL, MASK_CAP = 1e-9, 0.05  # gradient entries below MASK_REL * max|g| are masked after Adam steps; at most MASK_CAP of them

# (problem, tag, key, module globals as the __main__ block would set them, trajectory / prediction stored)
GRAPH_CASES = [
    ("poisson1d", "small", "vf1", {"var_form": 1}, True),
    ("poisson1d", "small", "vf2", {"var_form": 2}, True),
    ("poisson1d", "small", "vf3", {"var_form": 3}, True),
    ("poisson2d", "small", "vf0", {"var_form": 0, "scheme": "VPINNs"}, True),
    ("poisson2d", "small", "vf1", {"var_form": 1, "scheme": "VPINNs"}, True),
    ("poisson2d", "small", "vf2", {"var_form": 2, "scheme": "VPINNs"}, True),
    ("poisson2d", "small", "pinn", {"var_form": 1, "scheme": "PINNs"}, True),
    ("advdiff", "small", "vf0", {"var_form": 0}, True),
    ("advdiff", "small", "vf1", {"var_form": 1}, True),
    ("poisson2d", "e2", "vf2", {"var_form": 2, "scheme": "VPINNs"}, False),     # loss and gradient only
]
# The first seed of base, base + 1000, ... at which the reference alone meets graph_conditions (`--search-seeds` prints this block)
GRAPH_SEEDS = {
    "poisson1d_small_vf1": 8000,
    "poisson1d_small_vf2": 8001,
    "poisson1d_small_vf3": 8002,
    "poisson2d_small_vf0": 8003,
    "poisson2d_small_vf1": 8004,
    "poisson2d_small_vf2": 8005,
    "poisson2d_small_pinn": 8006,
    "advdiff_small_vf0": 8007,
    "advdiff_small_vf1": 8008,
    "poisson2d_e2_vf2": 8009,
}
PRED_STRIDE = {"poisson1d": 25, "poisson2d": 97, "advdiff": 97}


def graph_base_seed(i):
    return 8000 + i


def graph_theta0(layers, seed, extra=()):
    """tests/cases.theta0 (the project's Xavier init) plus a seeded N(0,1) * GRAPH_PERTURB on every weight and bias"""
    from cases import theta0
    th = theta0(layers, seed, extra=extra)
    n = th.size - len(extra)
    th[:n] += GRAPH_PERTURB * np.random.default_rng(seed + 100003).standard_normal(n)
    return th


def graph_conditions(l3, lossb_factor, g, layers, n_extra):
    """(ok, terms, floor, masked): both loss terms >= TERM_FLOOR of the loss, every parameter block >= BLOCK_FLOOR of the gradient
    norm, at most MASK_CAP of the entries under the Adam-step mask"""
    import generic_point as gp
    terms = (lossb_factor * l3[1] / l3[0], l3[2] / l3[0])
    total = np.linalg.norm(g)
    floor = min(np.linalg.norm(g[lo:hi]) for _, lo, hi in gp.blocks(layers, n_extra)) / total
    masked = float(np.mean(np.abs(g) <= MASK_REL * np.abs(g).max()))
    ok = bool(np.all(np.isfinite(g)) and min(terms) >= TERM_FLOOR and floor >= gp.BLOCK_FLOOR and masked <= MASK_CAP)
    return ok, terms, float(floor), masked


def _pack_vars(model):
    """the variables in the project's packing: W0, b0, W1, b1, ..., (epsilon)"""
    vs = []
    for W, b in zip(model.weights, model.biases):
        vs += [W, b]
    if hasattr(model, "epsilon"):
        vs.append(model.epsilon)
    return vs


def _inject(model, theta, layers):
    o = 0
    for l, (W, b) in enumerate(zip(model.weights, model.biases)):
        i, j = layers[l], layers[l + 1]
        W.load(theta[o:o + i * j].reshape(i, j)); o += i * j
        b.load(theta[o:o + j].reshape(1, j)); o += j
    if hasattr(model, "epsilon"):
        model.epsilon.load(theta[o:o + 1]); o += 1
    assert o == theta.size


def _read_theta(model):
    return np.concatenate([np.ravel(model.sess.run(v)) for v in _pack_vars(model)])


def _build_model(problem, mods, ns, glob):
    """The reference's own VPINN(...) of `problem` on the arrays of the set-up block `ns`, its module globals set as the __main__
    block would; returns (model, feed dict of train(), lossb factor in the loss, second loss term, prediction fetch + feed, points)."""
    import tf1_shim as tf
    tf.reset_default_graph()
    mod = mods[problem]
    L = [int(v) for v in ns["Net_layer"]]
    if problem == "poisson1d":
        mod.var_form, mod.LR, mod.lossb_weight = glob["var_form"], ns["LR"], ns["lossb_weight"]
        mod.total_record = []
        m = mod.VPINN(ns["X_u_train"], ns["u_train"], ns["X_quad_train"], ns["W_quad_train"], ns["F_ext_total"], ns["grid"],
                      ns["X_test"], ns["u_test"], L, ns["X_f_train"], ns["f_train"])
        feed = {m.x_tf: m.x, m.u_tf: m.u, m.x_quad: m.xquad, m.x_test: m.xtest, m.xf_tf: m.xf, m.f_tf: m.f}     # P1:203-205
        return m, feed, ns["lossb_weight"], m.lossv, ns["X_test"]
    if problem == "poisson2d":
        mod.var_form, mod.scheme = glob["var_form"], glob["scheme"]
        mod.loss_his = []
        m = mod.VPINN(ns["X_u_train"], ns["u_train"], ns["X_f_train"], ns["f_train"], ns["XY_quad_train"], ns["WXY_quad_train"],
                      ns["U_ext_total"], ns["F_ext_total"], ns["grid_x"], ns["grid_y"], ns["N_testfcn_total"], ns["X_test"],
                      ns["u_test"], L)
        feed = {m.x_tf: m.x, m.y_tf: m.y, m.u_tf: m.utrain, m.x_test: m.xtest, m.y_test: m.ytest,
                m.x_f_tf: m.xf, m.y_f_tf: m.yf}                                                                  # P2:235-238
        return m, feed, 10, (m.lossp if glob["scheme"] == "PINNs" else m.lossv), ns["X_test"]
    mod.var_form, mod.LR, mod.V = glob["var_form"], ns["LR"], ns["V"]
    XT = ns["XT_test"]
    m = mod.VPINN(ns["XT_u_train"], ns["u_train"], ns["XT_f_train"], ns["XT_quad_train"], ns["WXT_quad_train"], ns["T_quad"],
                  ns["WT_quad"], ns["grid_x"], ns["grid_t"], ns["N_testfcn_total"], XT, None, L, XT.min(0), XT.max(0))
    feed = {m.x_tf: m.x, m.t_tf: m.t, m.u_tf: m.u, m.x_f_tf: m.x_f, m.t_f_tf: m.t_f, m.x_quad: m.xquad, m.t_quad: m.tquad,
            m.x_test: m.xtest, m.t_test: m.ttest}                                                                # P3:294-297
    return m, feed, 1, m.lossv, XT


def run_graph_case(problem, key, glob, full, mods, ns, seed):
    """One case at one seed: dict of the arrays stored under `<key>_...`, and graph_conditions' verdict."""
    import contextlib
    import io
    import tf1_shim as tf
    L = [int(v) for v in ns["Net_layer"]]
    n_extra = 1 if problem == "advdiff" else 0
    th0 = graph_theta0(L, seed, extra=[0.9] * n_extra)
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet):
        m, feed, lossb_factor, second, Xt = _build_model(problem, mods, ns, glob)
    vs = _pack_vars(m)
    # Adam sees exactly the packed variables: `a` (P1:117, P2:146, P3:207) is connected to nothing and is skipped
    assert sorted(map(id, m.optimizer_Adam.vars)) == sorted(map(id, vs)), "Adam's variables are not the packed ones"
    _inject(m, th0, L)
    l3 = np.array([m.sess.run(t, feed) for t in (m.loss, m.lossb, second)], dtype=np.float64)
    g = np.concatenate([np.ravel(v) for v in m.sess.run(tf.gradients(m.loss, vs), feed)])
    cond = graph_conditions(l3, lossb_factor, g, L, n_extra)
    d = {"theta0": th0, "seed": np.int64(seed), "loss3": l3, "grad": g, "masked_share": np.float64(cond[3])}
    if not full:
        return d, cond
    with contextlib.redirect_stdout(quiet):
        if problem == "poisson1d":
            # train() records at it % 10 == 0 only (P1:210): K calls of train(1, tresh) run K updates (the optimizer state lives in
            # the session) and record the loss after each
            m_globals = mods[problem]
            for _ in range(GRAPH_K):
                m.train(1, 2e-32)
            his = [r[1] for r in m_globals.total_record]
            assert [r[0] for r in m_globals.total_record] == [0] * GRAPH_K
            pred = m.predict(Xt)                                                                                  # P1:197-199
        elif problem == "poisson2d":
            m.train(GRAPH_K)                                                                                     # P2:233-253
            his = list(mods[problem].loss_his)
            pred = m.predict()                                                                                   # P2:255-257
        else:
            # train(nIter, tresh) cannot return for nIter < 11 (P3:341 reads u_records, assigned only at a recording iteration
            # past 0.9 nIter, P3:327-330): its loop body (P3:309, 315) is run through sess.run in the same order instead
            his = []
            for _ in range(GRAPH_K):
                m.sess.run(m.train_op_Adam, feed)
                his.append(m.sess.run(m.loss, feed))
            pred = m.sess.run(m.u_NN_test, feed)                                                                 # P3:329
    assert len(his) == GRAPH_K
    s = PRED_STRIDE[problem]
    d.update(loss_his=np.array(his, dtype=np.float64), theta_K=_read_theta(m), pred_stride=np.int64(s),
             X_pred=np.ascontiguousarray(Xt[::s]), u_pred=np.ascontiguousarray(pred[::s]))
    return d, cond


def _graph_inputs(kept, m3):
    """set-up namespaces -> the few names _build_model reads (the set-up blocks name them differently per driver)"""
    out = {}
    for (problem, tag), ns in kept.items():
        d = dict(ns)
        if problem == "poisson2d":
            d.setdefault("U_ext_total", None)
        if problem == "advdiff":
            d.setdefault("LR", m3.LR)
        out[(problem, tag)] = d
    return out


def gen_graph(out, mods, kept, search=False):
    """Runs after the numpy generators.  `kept`: {(problem, tag): namespace of the set-up block}.  Writes <problem>_<tag>_graph.npz;
    with `search`, tries the seed list per case and prints the GRAPH_SEEDS block instead of reading it."""
    import time
    import tf1_shim
    import torch
    tf1_shim.install()
    torch.set_num_threads(1)     # (one summation order, whatever the machine: the files regenerate bit for bit)
    inputs = _graph_inputs(kept, mods["advdiff"])
    files, chosen = {}, {}
    t_all = time.time()
    for i, (problem, tag, key, glob, full) in enumerate(GRAPH_CASES):
        if (problem, tag) not in inputs:
            continue
        name = "%s_%s_%s" % (problem, tag, key)
        seeds = [graph_base_seed(i) + 1000 * k for k in range(GRAPH_MAX_TRIES)] if search else [GRAPH_SEEDS[name]]
        t0 = time.time()
        for seed in seeds:
            d, (ok, terms, floor, masked) = run_graph_case(problem, key, glob, full and not search, mods, inputs[(problem, tag)], seed)
            print("%-22s seed %d: terms %.2e %.2e, smallest block %.2e, masked %.3f -> %s"
                  % (name, seed, terms[0], terms[1], floor, masked, "ok" if ok else "rejected"))
            if ok:
                break
        assert ok, "no seed of %s meets the conditions for %s" % (seeds, name)
        chosen[name] = seed
        files.setdefault((problem, tag), {}).update({"%s_%s" % (key, k): v for k, v in d.items()})
        print("%-22s %.1f s" % (name, time.time() - t0))
    if search:
        print("GRAPH_SEEDS = {")
        for k, v in chosen.items():
            print('    "%s": %d,' % (k, v))
        print("}")
        return
    for (problem, tag), d in files.items():
        np.savez_compressed(os.path.join(out, "%s_%s_graph.npz" % (problem, tag)), **d)
    print("gen_graph: %.1f s" % (time.time() - t_all))


def _modules():
    _install_stubs()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, HERE)
    import tf1_shim
    tf1_shim.install()       # the class bodies resolve `tf` when they run; the numpy generators never touch it
    return {"poisson1d": _import(P1, "ref_p1"), "poisson2d": _import(P2, "ref_p2"), "advdiff": _import(P3, "ref_p3")}


SMALL = {
    "poisson1d": {"Net_layer": [1, 8, 8, 1], "N_Element": 4, "N_testfcn": 6, "N_Quad": 12},
    "poisson2d": {"Net_layer": [2, 8, 8, 1], "N_el_x": 3, "N_el_y": 2, "N_test_x": 3 * [4], "N_test_y": 2 * [3], "N_quad": 6,
                  "N_bound": 10, "N_residual": 10},
    "advdiff": {"Net_layer": [2, 8, 8, 1], "N_el_x": 3, "N_el_t": 2, "N_test_x": 3 * [4], "N_test_t": 2 * [3], "N_quad": 6,
                "N_bound": 10},
}
E2 = {"Net_layer": [2, 5, 1], "N_el_x": 2, "N_el_y": 2, "N_test_x": 2 * [5], "N_test_y": 2 * [5], "N_quad": 60,
      "N_bound": 10, "N_residual": 10}


def regenerate_small(out):
    """the small set-up fixtures and every *_graph.npz, into `out` (tests/test_oracle.py compares them with the committed files)"""
    mods = _modules()
    kept = {("poisson1d", "small"): gen_p1(out, "small", SMALL["poisson1d"]),
            ("poisson2d", "small"): gen_p2(out, "small", SMALL["poisson2d"]),
            ("poisson2d", "e2"): gen_p2(out, "e2", E2),
            ("advdiff", "small"): gen_p3(out, "small", SMALL["advdiff"], mods["advdiff"])}
    gen_graph(out, mods, kept)


def main():
    out = HERE
    mods = _modules()
    m1, m2, m3 = mods["poisson1d"], mods["poisson2d"], mods["advdiff"]
    kept = {}
    gen_quadrature(out)
    gen_testfcn(out, m1, m2, m3)
    L1 = [1, 20, 20, 20, 1]
    gen_p1(out, "default", {})                                     # reference defaults (P1:231-240)
    gen_p1(out, "cfg1", {"Net_layer": L1})                          # BASELINE config 1
    gen_p1(out, "ne3", {"Net_layer": L1, "N_Element": 3})           # the published 3-element run
    gen_p1(out, "cfg2", {"Net_layer": L1, "N_Element": 16})         # BASELINE config 2
    kept[("poisson1d", "small")] = gen_p1(out, "small", SMALL["poisson1d"])
    L2 = [2, 20, 20, 20, 1]
    gen_p2(out, "default", {}, store_test=True)                    # reference defaults (P2:279-288)
    gen_p2(out, "cfg3", {"Net_layer": L2, "N_el_x": 8, "N_el_y": 8, "N_test_x": 8 * [5], "N_test_y": 8 * [5]})
    gen_p2(out, "cfg4", {"Net_layer": L2, "N_el_x": 16, "N_el_y": 16, "N_test_x": 16 * [10],
                          "N_test_y": 16 * [10], "N_quad": 20})
    kept[("poisson2d", "small")] = gen_p2(out, "small", SMALL["poisson2d"])
    # anchors of var_form 2 (tests/test_oracle.py): ONE element with Jx = Jy = 1, and a 2 x 2 grid (Jx = Jy = 1/2), fine rule
    gen_p2(out, "e1", {"Net_layer": [2, 5, 1], "N_el_x": 1, "N_el_y": 1, "N_test_x": [5], "N_test_y": [5], "N_quad": 60,
                        "N_bound": 10, "N_residual": 10})
    kept[("poisson2d", "e2")] = gen_p2(out, "e2", E2)
    gen_p3(out, "default", {}, m3)                                 # reference defaults (P3:31-54)
    gen_p3(out, "cfg5", {"Net_layer": L2, "N_el_x": 8, "N_test_x": 8 * [5], "N_quad": 80}, m3)
    kept[("advdiff", "small")] = gen_p3(out, "small", SMALL["advdiff"], m3)
    gen_graph(out, mods, kept, search="--search-seeds" in sys.argv)
    for f in sorted(os.listdir(out)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(out, f)))


if __name__ == "__main__":
    main()
