"""The boundary / data term  lossb_weight * mean((u_d - u_theta(X_d))^2)  on its own, in fp64 on the CPU, and the case table of
tests/test_gpu_data_term.py (a plain helper module like cases.py and generic_point.py; no GPU needed).
tests/test_data_term_host.py proves it: decomposition = oracle, gradient against central differences, and the conditions below for
every case and every point count of the table.

Additive decomposition -- one expensive oracle evaluation serves a whole sweep of point counts:

    loss(theta; data) = var(theta) + w * msq(theta; data)         gradient likewise

  data_part   w * msq, msq and d(w * msq)/d theta by torch autograd through the oracle's own `neural_net`
              (validation_reference.bare_oracle: no second network); the epsilon slot of AdvDiff gets 0.
  var_part    the oracle's lossv and  gradient(full) - data_part(full).gradient  with the data arrays the case starts from.  The
              oracle classes do NOT accept an empty data set (torch.mean over no points is nan), so the subtraction is what is done;
              the loss needs none: the oracle's triple carries lossv itself.  `backend="generic"` references (the 80x80-point
              elements) take the data away on the device instead: hpv_set_data(NULL) and one loss_and_grad().

Inputs.  Data points uniform INSIDE the domain, targets u_d = u_theta(X) + s with |s| uniform in [0.5, 1.5] and a random sign
(seeded): every point carries a residual of the same order, every term of the mean lies in [0.25, 2.25].

Conditions on the reference alone (`conditions`; asserted before anything from the device is looked at):
  (a) every network block (W_l, b_l) of data_part's gradient is at least generic_point.BLOCK_FLOOR of the total gradient's norm
      (epsilon's slot of data_part is identically 0: the data term does not know epsilon; the TOTAL gradient's epsilon block is held
      to BLOCK_FLOOR by generic_point.block_errors in every comparison);
  (b) data_part's gradient norm is at least 1e-2 of the total's;
  (c) n <= 321: leaving out any single point moves at least one block of the reference gradient by more than 100 x the comparison
      bound (relative to that block of the total gradient) -- a kernel that drops a point, a tile's tail or a tile cannot pass.
      Larger n: the same follows for the loss alone -- each term >= 0.25 against a sum <= 2.25 n, so a dropped point moves msq by at
      least 1/(9 n) ~ 7e-6 at n = 16 385, four orders above the bound; `conditions` asserts exactly these two figures.
"""
import numpy as np
import torch

import generic_point as gp
import validation_reference as vr

LOO_MAX = 321                    # leave-one-out on the gradient up to this many points
DATA_SHARE = 1e-2                # (b)
LOO_MARGIN = 100.0               # (c)
DOMAIN = {"p1": (np.array([-1.0]), np.array([1.0])), "p2": (np.array([-1.0, -1.0]), np.array([1.0, 1.0])),
          "adv": (np.array([-1.0, 0.0]), np.array([1.0, 1.0]))}


def n_extra(prob):
    return 1 if prob == "adv" else 0


LOSSB_TOL = 1e-12               # the lossb slots against numpy, relative: non-negative terms, a summation error of a few 2^-53 per partial


def _net(prob, layers, theta):
    return vr.bare_oracle(prob, layers, theta)


def points(prob, n, seed):
    """n points uniform inside the domain"""
    lo, hi = DOMAIN[prob]
    return np.ascontiguousarray(lo + (hi - lo) * np.random.default_rng(seed).uniform(size=(n, lo.size)))


def targets(prob, layers, theta, X, seed):
    """u_theta(X) + s, |s| ~ U(0.5, 1.5), random sign: (n, 1)"""
    rng = np.random.default_rng(seed + 7919)
    with torch.no_grad():
        u = _net(prob, layers, theta).neural_net(torch.tensor(np.asarray(X, dtype=np.float64))).numpy()
    s = rng.uniform(0.5, 1.5, u.shape) * rng.choice([-1.0, 1.0], u.shape)
    return u + s


def data_part(prob, layers, theta, X, u_d, w, per_point=False):
    """dict(wmsq, msq, grad[, sq, J]): the data term, its plain mean and d(w msq)/d theta; per_point: the squares (n,) and their
    gradients J (n, P)"""
    X, u_d = np.asarray(X, dtype=np.float64), np.asarray(u_d, dtype=np.float64).reshape(-1, 1)
    o = _net(prob, layers, theta)
    P = o.theta.numel()
    if X.shape[0] == 0:
        return dict(wmsq=0.0, msq=0.0, grad=np.zeros(P))
    sq = torch.square(torch.tensor(u_d) - o.neural_net(torch.tensor(X))).reshape(-1)
    msq = torch.mean(sq)
    g, = torch.autograd.grad(float(w) * msq, o.theta, retain_graph=per_point)
    sqn = sq.detach().numpy()
    out = dict(wmsq=float(w) * float(np.mean(sqn)), msq=float(np.mean(sqn)), grad=g.numpy().copy())
    assert abs(out["msq"] - float(msq.detach())) <= 1e-14 * out["msq"]
    if per_point:
        J, = torch.autograd.grad(sq, o.theta, grad_outputs=torch.eye(sq.numel(), dtype=torch.float64), is_grads_batched=True)
        out["sq"], out["J"] = sqn, J.numpy()
    return out


def var_part(o, prob, layers, theta, X_full, u_full, w):
    """dict(lossv, grad, full) from an oracle-like `o` (loss_and_grad) holding the data (X_full, u_full): see the module docstring"""
    l3, g = o.loss_and_grad()
    d = data_part(prob, layers, theta, X_full, u_full, w)
    return dict(lossv=float(l3[2]), grad=np.asarray(g, dtype=np.float64) - d["grad"], full=(np.asarray(l3, dtype=np.float64), np.asarray(g, dtype=np.float64)), data_full=d)


def triple(prob, lossv, d):
    """{loss, lossb, lossv} as the classes report it: lossb is the plain mean for the Poisson problems (P1:98, P2:122), the
    weighted one for AdvDiff (P3:184)"""
    return np.array([lossv + d["wmsq"], d["wmsq"] if prob == "adv" else d["msq"], lossv])


def reference(prob, var, d):
    """(loss triple, gradient) of var + data"""
    return triple(prob, var["lossv"], d), var["grad"] + d["grad"]


def conditions(prob, layers, theta, X, u_d, w, g_var, tol):
    """(a) - (c) of the module docstring for this data set against the variational gradient g_var; returns the figures
    dict(block_share, share, loo) for the log.  `tol` is the comparison bound of the gradient blocks."""
    n = np.asarray(X).shape[0]
    d = data_part(prob, layers, theta, X, u_d, w, per_point=n <= LOO_MAX)
    gt = g_var + d["grad"]
    total = np.linalg.norm(gt)
    bl = gp.blocks(layers, 0)
    share = {k: float(np.linalg.norm(d["grad"][lo:hi]) / total) for k, lo, hi in bl}
    worst = min(share, key=share.get)
    assert share[worst] >= gp.BLOCK_FLOOR, ("(a)", n, worst, share)
    s = float(np.linalg.norm(d["grad"]) / total)
    assert s >= DATA_SHARE, ("(b)", n, s)
    if n_extra(prob):
        assert np.all(d["grad"][bl[-1][2]:] == 0.0)
    # (c) the loss: every term in [0.25, 2.25] (up to the rounding of u + s - u)
    sq = d["sq"] if "sq" in d else np.square(_residuals(prob, layers, theta, X, u_d))
    assert sq.min() >= 0.25 * (1 - 1e-12) and sq.max() <= 2.25 * (1 + 1e-12), ("(c) terms", n, sq.min(), sq.max())
    loo = None
    if n <= LOO_MAX:
        # without point i: w / (n - 1) (S - J_i) against w / n S, S = sum_i J_i  ->  w / (n - 1) (S / n - J_i); n = 1: the term is gone
        J, S = float(w) * d["J"], float(w) * d["J"].sum(axis=0)
        D = -d["grad"][None, :] if n == 1 else (S[None, :] / n - J) / (n - 1)
        norms = np.array([np.linalg.norm(gt[lo:hi]) for _, lo, hi in bl])
        rel = np.stack([np.linalg.norm(D[:, lo:hi], axis=1) for _, lo, hi in bl], axis=1) / norms[None, :]
        loo = float(rel.max(axis=1).min())
        assert loo > LOO_MARGIN * tol, ("(c)", n, loo, LOO_MARGIN * tol)
    else:
        assert 0.25 / (2.25 * n) > LOO_MARGIN * tol, ("(c) loss", n)
    return dict(block_share=share[worst], share=s, loo=loo)


def without_data_errors(g, g_ref, layers, n_extra_=0):
    """generic_point.block_errors for the gradient WITHOUT a data term: the weak forms hold derivatives of u only, so the output
    bias has no variational gradient at all.  A block below BLOCK_FLOOR of the reference gradient's norm is compared absolutely,
    against that norm (a stale adjoint of an earlier, larger data set would show exactly there); every other block relatively."""
    g, g_ref = np.asarray(g, dtype=np.float64).ravel(), np.asarray(g_ref, dtype=np.float64).ravel()
    total = np.linalg.norm(g_ref)
    out = {}
    for name, lo, hi in gp.blocks(layers, n_extra_):
        nb = np.linalg.norm(g_ref[lo:hi])
        out[name] = float(np.linalg.norm(g[lo:hi] - g_ref[lo:hi]) / (nb if nb >= gp.BLOCK_FLOOR * total else total))
    return out


def _residuals(prob, layers, theta, X, u_d):
    with torch.no_grad():
        u = _net(prob, layers, theta).neural_net(torch.tensor(np.asarray(X, dtype=np.float64))).numpy().reshape(-1)
    return np.asarray(u_d, dtype=np.float64).reshape(-1) - u


# ---- the case table ------------------------------------------------------------------------------------------------------------
# One handle per launch structure: the smallest grid of its family in CASES of tests/test_gpu_generic_point.py (by name), the data
# seed, lossb_weight (never 1), and the structure's own point-count edges.  Counts written T(k) are "k data tiles": 16 k points.
#   edge    how the structure's limit W is found on the device (tests/test_gpu_data_term.py):
#           "wg"     W = workgroups = elements x split (split read from hpv_kernel_variant); tiles W - 1 (with a tail), W, W + 1
#                    (a 1-point tail) -- computed at run time, `w_static` is what the host test uses for the same counts
#           "list"   the counts given in `own`
COMMON = [1, 15, 16, 17, 31, 33]                # ... then the structure's own edge, then DOWN to 7 and 16, no data, 17 again
DOWN = [7, 16]

STRUCTURES = {
    # name: case of CASES, data seed, lossb_weight, edge kind, own counts or static W
    "fused-unsplit": dict(case="onehot-L2", seed=9101, lbw=3, edge="wg", w_static=15),
    "fused-gen": dict(case="gen-advf0-16x16", seed=9102, lbw=3, edge="wg", w_static=4),
    "fused-split-q14": dict(case="padded-q14-p2vf1", seed=9103, lbw=3, edge="wg", w_static=120),
    # k_iter_small: 64 elements, W = 64 -- 1 025 points are W + 1 tiles AND more than 64 partials on the merged path; 1 041: 66 tiles
    "small": dict(case="small-L2", seed=9104, lbw=3, edge="wg", w_static=64, extra=[1041]),
    # k_iter_tile never declines: an element's free waves (8 - 7 tiles in 2-D, 6 - 5 in 1-D) adopt data tiles, the rest goes to extra
    # workgroups of 8 / 6 tiles: 6 (5) free slots, then the first and the second extra workgroup
    "tile-2d": dict(case="tile-advf0", seed=9105, lbw=3, edge="list", own=[96, 97, 224, 225]),
    "tile-1d": dict(case="tile-1d-vf1", seed=9106, lbw=3, edge="list", own=[79, 81, 175, 177]),
    # k_iter_tall: 8 elements x 32 workgroups; quarter tiles while the data tiles fit the 16 x 8 workgroups without a 13th tile (128),
    # one tile per workgroup at most (256)
    "tall": dict(case="tall-advf0", seed=9107, lbw=3, edge="wg", w_static=256, extra=[2048, 2049]),
    # k_iter_elem, 16x16 points on 8 waves x 2 tiles: no free slot, extra workgroups of 16 tiles -- one full, then a second for one point
    # (var_form 2 with a random F: the variational gradient is 30 x that of the other cases -- lossb_weight 30 keeps condition (b))
    "elem": dict(case="elem-16x16-p2vf2", seed=9108, lbw=30, edge="list", own=[256, 257]),
    "separate": dict(case="separate-project-wg", seed=9109, lbw=3, edge="list", own=[255, 1025, 1041]),
    "reverse-projection": dict(case="projection-in-the-reverse-kernel", seed=9110, lbw=3, edge="list", own=[255, 257]),
    "wide-H32": dict(case="wide-H32", seed=9111, lbw=3, edge="list", own=[255, 257]),
    "generic": dict(case="generic-p2vf1", seed=9112, lbw=3, edge="list", own=[255, 256, 257, 513]),
}


def wg_counts(W):
    """tiles W - 1 (tail of 13 points), W (full), W + 1 (tail of 1 point)"""
    return [16 * (W - 1) - 3, 16 * W, 16 * W + 1]


def sweep_counts(spec, W=None):
    """[(n, kind)] of a structure: kind 'in' (the structure must stay), 'over' (W + 1 and beyond: result only), 'none' (no data)"""
    own = []
    if spec["edge"] == "wg":
        lo, at, over = wg_counts(spec["w_static"] if W is None else W)
        own = [(n, "in") for n in spec.get("extra", []) if n < lo] + [(lo, "in"), (at, "in"), (over, "over")] + \
              [(n, "over") for n in spec.get("extra", []) if n > over]
    else:
        own = [(n, "in") for n in spec["own"]]
    return [(n, "in") for n in COMMON] + own + [(n, "in") for n in DOWN] + [(0, "none"), (17, "in")]


def case_of(name):
    """the case dict of CASES in tests/test_gpu_generic_point.py with lossb_weight set (the builders there read c['lbw'])"""
    import test_gpu_generic_point as T
    spec = STRUCTURES[name]
    c = next(p.values[0] for p in T.CASES if p.values[0]["name"] == spec["case"])
    return dict(c, lbw=spec["lbw"])


def start_data(c, s):
    """(X, u) the case's handle starts from"""
    X = s["XT_u_train" if c["prob"] == "adv" else "X_u_train"]
    return np.asarray(X, dtype=np.float64), np.asarray(s["u_train"], dtype=np.float64).reshape(-1, 1)


def with_data(c, a, X, u):
    """the positional arguments `a` of the case's classes with (X, u) as the training data"""
    a = list(a)
    a[0], a[1] = np.ascontiguousarray(X), np.asarray(u, dtype=np.float64).reshape(-1, 1)
    return a


# ---- scheme='PINNs': the data term has a batch of its own (k_data_loss; on the MFMA backend a small MFMA batch of exactly n points) ----
PINN_LAYERS = {"generic": {"p1": [1, 7, 5, 1], "p2": [2, 7, 9, 1], "adv": [2, 6, 9, 4, 1]},
               "mfma": {"p1": [1, 20, 20, 20, 1], "p2": [2, 20, 20, 20, 1], "adv": [2, 20, 20, 20, 1]}}
PINN_W = {"p1": 30.0, "p2": 30.0, "adv": 3.0}      # (the strong residual of the Poisson fixtures carries f ~ 1e2: 30 keeps condition (b))
PINN_V = 0.6
DATA_LOSS_COUNTS = [1, 255, 256, 257, 513, 16384, 16385, 16641]      # k_data_loss: one block, two, three; the grid-stride loop behind 64 blocks
PINN_MFMA_COUNTS = [1, 15, 17, 257, 3]                                # the last tile of k_fwd_mfma / k_bwd_mfma, then DOWN


def pinn_case(prob, backend):
    """(reference object, positional arguments of the product class, layers, theta) of the strong-form scheme on the small
    fixture of the problem: tests/pinn_reference.py for Poisson-1D and AdvDiff, the oracle's own scheme for Poisson-2D"""
    from cases import gold, p1_args, p2_args, p3_args
    from oracle.vpinn_oracle import OracleVPINN2D
    from pinn_reference import PinnRef1D, PinnRefAdvDiff
    L = PINN_LAYERS[backend][prob]
    th = gp.generic_theta(L, 9300 + len(prob) + len(backend), extra=[0.9] if prob == "adv" else ())
    if prob == "p1":
        a = list(p1_args(gold("poisson1d_small"), L))
        o = PinnRef1D(a[0], a[1], a[9], a[10], L, lossb_weight=PINN_W[prob], init_params=th)
    elif prob == "p2":
        a = list(p2_args(gold("poisson2d_small"), L))
        o = OracleVPINN2D(*a, scheme="PINNs", lossb_weight=PINN_W[prob], init_params=th)
    else:
        a = list(p3_args(gold("advdiff_small"), L))
        o = PinnRefAdvDiff(a[0], a[1], a[2], L, V=PINN_V, lossb_weight=PINN_W[prob], init_params=th)
    return o, a, L, th


def small_generic_case():
    """backend='generic' on a small network: 2 x 2 warped elements of 5 x 5 points, [2, 7, 9, 1]"""
    return dict(name="generic-small", prob="p2", vf=1, q=5, nt=3, nex=2, ney=2, L=[2, 7, 9, 1], seed=9201, lbw=3, backend="generic",
                want=["k_mlp_fwd_generic", "k_mlp_bwd_generic"], structure="separate")
