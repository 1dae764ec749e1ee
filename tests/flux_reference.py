"""The flux term  w_f * mean((a u + b . grad u - g)^2)  (hpv_set_flux_data) on its own, in fp64 on the CPU, and the case table of
tests/test_gpu_flux.py (a plain helper module like data_term_reference.py; no GPU needed).  tests/test_flux_host.py proves it.

The additive decomposition of tests/data_term_reference.py, one term further:

    loss(theta) = [the oracle's loss with the case's Dirichlet data] + w_f * msf(theta; flux data)         gradient likewise

  flux_part   w_f * msf, msf and d(w_f * msf)/d theta by torch autograd through the oracle's own `neural_net`
              (validation_reference.bare_oracle): grad u = torch.autograd.grad(u, X, create_graph=True), then the gradient with
              respect to theta.  The epsilon slot of AdvDiff gets 0: the term does not know epsilon.
  the rest    data_term_reference.var_part / data_part, unchanged.

Inputs.  Flux points uniform INSIDE the domain; a ~ U(0.5, 1.5) with a random sign, every component of b likewise;
g = a u_theta + b . grad u_theta + s with |s| ~ U(0.5, 1.5) and a random sign: every point carries a residual r = -s of order one,
every term of the mean lies in [0.25, 2.25].  w_f = 3.

Conditions on the reference alone (`conditions`), asserted before a device number is looked at:
  (a) every network block of flux_part's gradient is at least generic_point.BLOCK_FLOOR of the total gradient's norm;
  (b) its norm is at least data_term_reference.DATA_SHARE of the total's;
  (c) n <= 33: leaving out any single flux point moves some block of the reference gradient by more than LOO_MARGIN x the comparison
      bound; larger n: the loss's own figure, 0.25 / (2.25 n), against the same margin;
  (d) zeroing `a` alone, or any one column of `b` alone, moves the loss by more than 1e-3 of it: a kernel that reads the wrong channel
      or the wrong coefficient column cannot pass.
"""
import numpy as np
import torch

import data_term_reference as dr
import generic_point as gp
import validation_reference as vr

W_F = 3.0
LOO_MAX = 33
SWEEP = [1, 15, 16, 17, 33, 1]      # up through the 16-point tile's edges and back down: stale GBAR / partials / gradient rows
LARGE_N = 16400                     # more than 64 x 256 points: the grid-stride loop of k_flux_loss
COLUMN_MOVE = 1e-3                  # (d)


def _signed(rng, shape):
    return rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)


def _u_du(o, X):
    """u (n,) and grad u (n, dim) of the oracle's network at X, differentiable with respect to o.theta"""
    Xt = torch.tensor(np.asarray(X, dtype=np.float64), requires_grad=True)
    u = o.neural_net(Xt)
    du, = torch.autograd.grad(u, Xt, grad_outputs=torch.ones_like(u), create_graph=True)
    return u.reshape(-1), du


def flux_data(prob, layers, theta, n, seed):
    """dict(X (n, dim), a (n,), b (n, dim), g (n,)) of the module docstring"""
    X = dr.points(prob, n, seed)
    rng = np.random.default_rng(seed + 104729)
    a, b = _signed(rng, n), _signed(rng, X.shape)
    s = _signed(rng, n)
    u, du = _u_du(vr.bare_oracle(prob, layers, theta), X)
    g = a * u.detach().numpy() + np.sum(b * du.detach().numpy(), axis=1) + s
    return dict(X=X, a=a, b=b, g=g)


def head(f, n):
    """the first n points of a flux data set"""
    return {k: v[:n] for k, v in f.items()}


def coef(f):
    """(n, 1 + dim) rows (a, b_0 ..): the layout of hpv_set_flux_data"""
    return np.ascontiguousarray(np.concatenate([f["a"][:, None], f["b"]], axis=1))


def flux_part(prob, layers, theta, f, w=W_F, per_point=False):
    """dict(wmsf, msf, grad[, sq, J]): the flux term, its plain mean and d(w msf)/d theta; per_point: the squares (n,) and their
    gradients J (n, P)"""
    o = vr.bare_oracle(prob, layers, theta)
    P = o.theta.numel()
    if f is None or f["X"].shape[0] == 0:
        return dict(wmsf=0.0, msf=0.0, grad=np.zeros(P))
    u, du = _u_du(o, f["X"])
    r = torch.tensor(f["a"]) * u + torch.sum(torch.tensor(f["b"]) * du, dim=1) - torch.tensor(f["g"])
    sq = torch.square(r)
    msf = torch.mean(sq)
    g, = torch.autograd.grad(float(w) * msf, o.theta, retain_graph=per_point)
    sqn = sq.detach().numpy()
    out = dict(wmsf=float(w) * float(np.mean(sqn)), msf=float(np.mean(sqn)), grad=g.numpy().copy())
    if per_point:
        J, = torch.autograd.grad(sq, o.theta, grad_outputs=torch.eye(sq.numel(), dtype=torch.float64), is_grads_batched=True)
        out["sq"], out["J"] = sqn, J.numpy()
    return out


def triple(prob, lossv, d, fp):
    """{loss, lossb, lossv} as the classes report it with a flux term: the loss includes it; the second entry is the packed buffer's
    weighted slot for AdvDiff (lossb_weight * msq + w_f * msf, P3:184 folds the weight in) and stays the plain Dirichlet mean for the
    Poisson problems (P1:98, P2:122)"""
    return np.array([lossv + d["wmsq"] + fp["wmsf"], d["wmsq"] + fp["wmsf"] if prob == "adv" else d["msq"], lossv])


def reference(prob, var, d, fp):
    """(loss triple, gradient) of var + data + flux"""
    return triple(prob, var["lossv"], d, fp), var["grad"] + d["grad"] + fp["grad"]


def conditions(prob, layers, theta, f, g_rest, tol, w=W_F):
    """(a) - (d) for the flux data `f` against the gradient of everything else, g_rest; returns the figures for the log"""
    n = f["X"].shape[0]
    fp = flux_part(prob, layers, theta, f, w, per_point=n <= LOO_MAX)
    gt = g_rest + fp["grad"]
    total = np.linalg.norm(gt)
    bl = gp.blocks(layers, 0)
    share = {k: float(np.linalg.norm(fp["grad"][lo:hi]) / total) for k, lo, hi in bl}
    worst = min(share, key=share.get)
    assert share[worst] >= gp.BLOCK_FLOOR, ("(a)", n, worst, share)
    s = float(np.linalg.norm(fp["grad"]) / total)
    assert s >= dr.DATA_SHARE, ("(b)", n, s)
    if dr.n_extra(prob):
        assert np.all(fp["grad"][bl[-1][2]:] == 0.0)
    loo = None
    if n <= LOO_MAX:
        sq = fp["sq"]
        assert sq.min() >= 0.25 * (1 - 1e-9) and sq.max() <= 2.25 * (1 + 1e-9), ("(c) terms", n, sq.min(), sq.max())
        J, S = float(w) * fp["J"], float(w) * fp["J"].sum(axis=0)
        D = -fp["grad"][None, :] if n == 1 else (S[None, :] / n - J) / (n - 1)
        norms = np.array([np.linalg.norm(gt[lo:hi]) for _, lo, hi in bl])
        rel = np.stack([np.linalg.norm(D[:, lo:hi], axis=1) for _, lo, hi in bl], axis=1) / norms[None, :]
        loo = float(rel.max(axis=1).min())
        assert loo > dr.LOO_MARGIN * tol, ("(c)", n, loo, dr.LOO_MARGIN * tol)
    else:
        assert 0.25 / (2.25 * n) > dr.LOO_MARGIN * tol, ("(c) loss", n)
    # (d) one coefficient column at a time
    moves = []
    for col in range(1 + f["X"].shape[1]):
        f0 = dict(f, a=f["a"].copy(), b=f["b"].copy())
        if col == 0:
            f0["a"][:] = 0.0
        else:
            f0["b"][:, col - 1] = 0.0
        moves.append(abs(flux_part(prob, layers, theta, f0, w)["wmsf"] - fp["wmsf"]) / fp["wmsf"])
    assert min(moves) > COLUMN_MOVE, ("(d)", n, moves)
    return dict(block_share=share[worst], share=s, loo=loo, column=min(moves))


def adam_trajectory(o, prob, layers, f, steps, w=W_F):
    """`steps` TF1-Adam updates (the oracle's own rule and constants, adam_step of oracle.vpinn_oracle) of  the oracle's loss +
    flux_part  starting from the oracle's current parameters; the oracle object is advanced in place.  Returns the parameters."""
    m, v = np.zeros(o.theta.numel()), np.zeros(o.theta.numel())
    b1p, b2p = o.beta1, o.beta2
    for _ in range(steps):
        th = o.get_params()
        g = np.asarray(o.loss_and_grad()[1], dtype=np.float64) + flux_part(prob, layers, th, f, w)["grad"]
        lr_t = o.LR * np.sqrt(1.0 - b2p) / (1.0 - b1p)
        m = o.beta1 * m + (1.0 - o.beta1) * g
        v = o.beta2 * v + (1.0 - o.beta2) * g * g
        with torch.no_grad():
            o.theta.copy_(torch.tensor(th - lr_t * m / (np.sqrt(v) + o.eps_adam)))
        b1p, b2p = b1p * o.beta1, b2p * o.beta2
    return o.get_params()


# ---- the case table: one handle per launch structure, the smallest shape that reaches it ----------------------------------------
L2, L3 = [2, 20, 20, 1], [2, 20, 20, 20, 1]
ONE = {"HPV_FUSE": "i"}


def _c(name, prob, vf, q, nt, nex, ney, L, want, structure, seed, **kw):
    return dict(name=name, prob=prob, vf=vf, q=q, nt=nt, nex=nex, ney=ney, L=L, want=want, structure=structure, seed=seed, lbw=3, **kw)


STRUCTURES = {
    "fused": _c("fused", "p2", 1, 12, 6, 2, 2, L2, ["k_iter_fused<L=2,SPLIT=false,", ",12x12/6x6>"], "whole-iteration", 7101, env=ONE, F="random"),
    # (the grid and seed of gen-advf0-16x16 in tests/test_gpu_generic_point.py: d/d epsilon above BLOCK_FLOOR there)
    "fused-gen": _c("fused-gen", "adv", 0, 16, 8, 2, 2, L3, ["k_iter_fused<L=3,SPLIT=false,", ",16x16/8x8,NT2=1,GEN>"], "whole-iteration", 4507, env=ONE),
    # one element of the 1-D 80 / 60 rule: k_iter_tile on a one-workgroup grid finalises in-kernel without flux data
    "tile-1d": _c("tile-1d", "p1", 1, 80, 60, 1, 1, [1, 20, 20, 20, 1], ["k_iter_tile<D=1,", "80x1/60x1"], "whole-iteration-tile", 7103),
    "tile-2d": _c("tile-2d", "p2", 0, 10, 5, 2, 2, L3, ["k_iter_tile<D=2,"], "whole-iteration-tile", 7104),
    "separate": _c("separate", "p2", 1, 12, 6, 2, 2, L3, ["k_fwd_mfma<", "k_bwd_mfma<"], "separate", 7105, env={"HPV_FUSE": "n"}, F="random"),
    "wide-H24": _c("wide-H24", "p2", 1, 10, 5, 2, 2, [2, 24, 24, 24, 1], ["k_fwd_wide<", "k_bwd_wide<", "H=24>"], "separate", 7106),
    "generic": _c("generic", "p2", 1, 5, 3, 2, 2, [2, 7, 9, 1], ["k_mlp_fwd_generic", "k_mlp_bwd_generic"], "separate", 7107, backend="generic"),
}
PINN = ["p1", "p2", "adv"]          # the strong-form scheme: data_term_reference.pinn_case(prob, "mfma")
FLUX_SEED = 8800
LARGE_SEED = 8809                   # (signs average out over 16 400 points: the first seed from 8801 on whose set keeps (a) and (b) with margin)


def sweep_data(prob, layers, theta):
    """the 33 flux points every sweep takes its first n from"""
    return flux_data(prob, layers, theta, max(SWEEP), FLUX_SEED)


def oracle_of(c):
    """(CPU oracle, positional class arguments, initial parameters) of a STRUCTURES case -- what test_gpu_generic_point._pair builds,
    without the device handle"""
    import test_gpu_generic_point as T
    s, th = T._setup(c)
    Oc, _, tup = T._classes(c["prob"])
    a = tup(s, c["L"])
    o = Oc(*a, init_params=th, **T._kw(c))
    o.vectorized = True
    return o, a, th
