"""The iteration of a handle with the quasilinear multiplier (forward -> k_project_nl*_q -> reverse) against the same handle with the
multiplier removed (forward -> k_project_nl -> reverse, the code as it was before hpv_set_quasilinear existed), in one run, the
variants interleaved.

    python scripts/quasilinear_bench.py [--reps 9] [--iters 400]

Per shape (the grids of scripts/nonlinear_bench.py, whose handle this builds on, with a cubic term so that every variant runs
k_project_nl) four handles on the same operator, data and parameters: `removed` (hpv_set_quasilinear with planes that leave mu = 1),
`P(u)` (m = (1, 0, 1), r = 0), `B(s)` (delta = 1, r = -1/2) and `both`.  Microseconds per training iteration of hpv_step (captured
graphs, wall clock around a synchronising call, median and min..max over the repetitions) and the projection kernel class alone
(hipEvents, eager launches).  No gate: profiles/quasilinear.md records the figures."""
import argparse
import json

import numpy as np

from nonlinear_bench import handle, per_iter_us

# name: (m2, exponent)
VARIANTS = {"removed": (0.0, 0.0), "P(u)": (1.0, 0.0), "B(s)": (0.0, -0.5), "both": (1.0, -0.5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=400)
    a = ap.parse_args()
    L = [2, 20, 20, 20, 1]
    out = []
    for nex, ney, q, nt in ((16, 16, 20, 10), (8, 8, 12, 6)):
        hs = {}
        for k, (m2, r) in VARIANTS.items():
            hs[k] = h = handle(nex, ney, q, nt, L, (1,))
            planes = np.zeros((4, nex * ney * q * q))
            planes[0], planes[2], planes[3] = 1.0, m2, 1.0
            h.set_quasilinear(planes, r)
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
