"""The iteration of a linear handle with K = 2 integral constraints (forward -> k_project_lin -> k_moment_part -> k_moment_close ->
k_moment_adj -> reverse) against the same handle without terms (forward -> k_project_lin -> reverse: the launches of a handle that never
heard of hpv_set_moments, bit for bit), in one run, the variants interleaved.

    python scripts/moments_bench.py [--reps 9] [--iters 400]

Shapes: 16x16 elements of 8x8 points / 4x4 test functions, and the two grids of scripts/nonlinear_bench.py, whose handle this builds on.
Microseconds per training iteration of hpv_step (captured graphs, wall clock around a synchronising call, median and min..max over the
repetitions).  No gate: profiles/integral_constraints.md records the figures."""
import argparse
import json

import numpy as np

from nonlinear_bench import handle, per_iter_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=400)
    a = ap.parse_args()
    L = [2, 20, 20, 20, 1]
    for nex, ney, q, nt in ((16, 16, 8, 4), (16, 16, 20, 10), (8, 8, 12, 6)):
        hs = {k: handle(nex, ney, q, nt, L, ()) for k in ("none", "K=2", "K=8")}
        n = nex * ney * q * q
        rng = np.random.default_rng(5)
        for k, K in (("K=2", 2), ("K=8", 8)):
            hs[k].set_moments([1 + i % 2 for i in range(K)], rng.uniform(-1.0, 1.0, (K, n)) / n, [0.1] * K, [1.0] * K)
        for h in hs.values():
            h.step(a.iters, False)                       # graphs captured, clocks up
        t = {k: [] for k in hs}
        for _ in range(a.reps):
            for k, h in hs.items():
                t[k].append(per_iter_us(h, a.iters))
        r = dict(shape="%dx%d elements of %dx%d/%dx%d" % (nex, ney, q, q, nt, nt), variants={k: h.kernel_variant() for k, h in hs.items()},
                 loss_finite={k: bool(np.all(np.isfinite(h.loss_and_grad(False)[0]))) for k, h in hs.items()},
                 iter_us={k: dict(median=float(np.median(v)), min=min(v), max=max(v)) for k, v in t.items()})
        print(json.dumps(r))


if __name__ == "__main__":
    main()
