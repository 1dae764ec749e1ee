"""The linear problems' iteration (forward -> k_project_lin -> reverse) against the existing Poisson-2D var_form 1 handle under
HPV_FUSE=n (forward -> k_project_* -> reverse: the same channels, the same layer kernels) at k = 1, in one run, A and B interleaved.

    python scripts/linear_bench.py [--reps 9] [--iters 400]

Per shape: microseconds per training iteration of hpv_step (captured graphs, wall clock around a synchronising call, median and
min..max over the repetitions), the projection kernel class alone (hipEvents, eager launches), and the gate of profiles/linear_operator.md:
new <= old + spread(old) + the coefficient planes streamed once at the residual kernel's HBM rate."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_RATE = 4.50e12      # bytes / s of the stand-alone residual + adjoint kernel (profiles/r04_notes.md)


def handle(pde, nex, ney, q, nt, L, seed=3):
    from hp_vpinns_amd import GaussLobattoJacobiWeights, _lib
    from hp_vpinns_amd.init import xavier_init
    from hp_vpinns_amd.testfcn import tables_1d
    x, w = GaussLobattoJacobiWeights(q, 0, 0)
    h = _lib.Handle(pde, 1, _lib.ACT_TANH, L, lr=1e-3, lossb_weight=10.0)
    h.set_quadrature(x, w, x, w)
    t = tables_1d(nt, x)
    h.set_tables(t, t)
    h.set_elements(np.linspace(-1, 1, nex + 1), np.linspace(-1, 1, ney + 1))
    rng = np.random.default_rng(seed)
    h.set_rhs(rng.standard_normal(nex * ney * nt * nt))
    if pde == _lib.PDE_LINEAR2D:
        planes = np.zeros((5, nex * ney * q * q))
        planes[:2] = 1.0
        h.set_operator(planes)
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
    os.environ["HPV_FUSE"] = "n"
    from hp_vpinns_amd import _lib
    L = [2, 20, 20, 20, 1]
    out = []
    for nex, ney, q, nt in ((16, 16, 20, 10), (8, 8, 12, 6)):
        old, new = handle(_lib.PDE_POISSON2D, nex, ney, q, nt, L), handle(_lib.PDE_LINEAR2D, nex, ney, q, nt, L)
        l_old, l_new = old.loss_and_grad(True), new.loss_and_grad(True)
        agree = float(np.linalg.norm(l_old[1] - l_new[1]) / np.linalg.norm(l_old[1]))
        for h in (old, new):
            h.step(a.iters, False)                       # graphs captured, clocks up
        t_old, t_new = [], []
        for _ in range(a.reps):
            t_old.append(per_iter_us(old, a.iters))
            t_new.append(per_iter_us(new, a.iters))
        names = (old.kernel_variant(), new.kernel_variant())
        kern = []
        for h in (old, new):
            h.enable_timing(True)
            h.step(200, False)
            kern.append(h.kernel_time_ms(1)[0] * 1e3)
            h.enable_timing(False)
        planes_us = 5 * nex * ney * q * q * 8 / HBM_RATE * 1e6
        spread = max(t_old) - min(t_old)
        r = dict(shape="%dx%d elements of %dx%d/%dx%d" % (nex, ney, q, q, nt, nt), old=names[0], new=names[1],
                 iter_us_old=dict(median=float(np.median(t_old)), min=min(t_old), max=max(t_old)),
                 iter_us_new=dict(median=float(np.median(t_new)), min=min(t_new), max=max(t_new)),
                 project_us_old=kern[0], project_us_new=kern[1], planes_us=planes_us, spread_old_us=spread,
                 gate_pass=bool(np.median(t_new) <= np.median(t_old) + spread + planes_us), gradient_agreement=agree)
        out.append(r)
        print(json.dumps(r))
    return out


if __name__ == "__main__":
    main()
