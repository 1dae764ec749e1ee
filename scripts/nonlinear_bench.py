"""The iteration of a handle with a nonlinear term (forward -> k_project_nl -> reverse) against the same handle with the term removed
(forward -> k_project_lin -> reverse), in one run, the variants interleaved.

    python scripts/nonlinear_bench.py [--reps 9] [--iters 400]

Per shape (the grids of scripts/linear_bench.py) three handles on the same operator, data and parameters: `lin` (the term removed),
`poly+adv` (a2, a3, gx, gy) and `exp` (ae alone).  Microseconds per training iteration of hpv_step (captured graphs, wall clock around
a synchronising call, median and min..max over the repetitions) and the projection kernel class alone (hipEvents, eager launches).
No gate: profiles/nonlinear_terms.md records the figures."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"lin": (), "poly+adv": (0, 1, 3, 4), "exp": (2,)}


def handle(nex, ney, q, nt, L, rows, seed=3):
    from hp_vpinns_amd import GaussLobattoJacobiWeights, _lib
    from hp_vpinns_amd.init import xavier_init
    from hp_vpinns_amd.testfcn import tables_1d
    x, w = GaussLobattoJacobiWeights(q, 0, 0)
    h = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, L, lr=1e-3, lossb_weight=10.0)
    h.set_quadrature(x, w, x, w)
    t = tables_1d(nt, x)
    h.set_tables(t, t)
    h.set_elements(np.linspace(-1, 1, nex + 1), np.linspace(-1, 1, ney + 1))
    rng = np.random.default_rng(seed)
    h.set_rhs(rng.standard_normal(nex * ney * nt * nt))
    n = nex * ney * q * q
    planes = np.zeros((5, n))
    planes[:2] = 1.0
    h.set_operator(planes)
    nl = np.zeros((5, n))
    nl[list(rows)] = rng.uniform(0.5, 1.5, (len(rows), n))
    h.set_nonlinear(nl)                                  # (all zeros: the term removed)
    Xb = rng.uniform(-1, 1, (80, 2))
    h.set_data(Xb, np.sin(Xb[:, 0]) * Xb[:, 1])
    h.set_params(xavier_init(L, 7))
    return h


def per_iter_us(h, iters):
    t0 = time.perf_counter()
    h.step(iters, False)
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=400)
    a = ap.parse_args()
    L = [2, 20, 20, 20, 1]
    out = []
    for nex, ney, q, nt in ((16, 16, 20, 10), (8, 8, 12, 6)):
        hs = {k: handle(nex, ney, q, nt, L, rows) for k, rows in VARIANTS.items()}
        for h in hs.values():
            h.step(a.iters, False)                       # graphs captured, clocks up
        t = {k: [] for k in hs}
        for _ in range(a.reps):
            for k, h in hs.items():
                t[k].append(per_iter_us(h, a.iters))
        names = {k: h.kernel_variant() for k, h in hs.items()}
        kern = {}
        for k, h in hs.items():
            h.enable_timing(True)
            h.step(200, False)
            kern[k] = h.kernel_time_ms(1)[0] * 1e3
            h.enable_timing(False)
        finite = {k: bool(np.all(np.isfinite(h.loss_and_grad(False)[0]))) for k, h in hs.items()}
        r = dict(shape="%dx%d elements of %dx%d/%dx%d" % (nex, ney, q, q, nt, nt), variants=names, loss_finite=finite,
                 iter_us={k: dict(median=float(np.median(v)), min=min(v), max=max(v)) for k, v in t.items()}, project_us=kern)
        out.append(r)
        print(json.dumps(r))
    return out


if __name__ == "__main__":
    main()
