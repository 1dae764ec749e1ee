"""The measurement behind profiles/validation.md: on one MI355X, BASELINE config 4 (16 x 16 elements, 20 x 20 points, [2,20,20,20,1])
with the reference's P2 test grid (201 x 201 points, P2:418-426) as the validation set, microseconds per training iteration of

    step            hpv_step(1000)
    step_validate   hpv_step_validate(1000, 10): 100 validations enqueued between the iterations, one read at the end
    host            100 x (hpv_step(10) + rel_l2_error): the host route (upload, value-only forward, download, numpy norm)

in ONE process, after one untimed call of each (the iteration graphs are captured at first use); five repeats, the three routes
alternating inside every repeat; median, min and max.  A host clock around calls that end in a device synchronise.

    python scripts/validation_bench.py                  the three routes
    python scripts/validation_bench.py --reduce N       50 hpv_validate calls on N points (to be run under rocprofv3 --kernel-trace
                                                        --stats: the reduction kernel alone is the row k_validate_reduce)"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hp_vpinns_amd.drivers import poisson2d  # noqa: E402
from hp_vpinns_amd.init import xavier_init  # noqa: E402

CFG4 = dict(N_el_x=16, N_el_y=16, N_test_x=10, N_test_y=10, N_quad=20, N_bound=80, N_residual=100)
LAYERS = [2, 20, 20, 20, 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reduce", type=int, default=0)
    a = ap.parse_args()
    s = poisson2d.setup(**CFG4, with_test_grid=True)
    theta = xavier_init(LAYERS, 1234)
    m = poisson2d.build_model(s, LAYERS, var_form=1, init_params=theta)
    if a.reduce:
        rng = np.random.default_rng(1)
        X = rng.uniform(-1, 1, (a.reduce, 2))
        m.set_validation(X, poisson2d.u_ext(X[:, 0:1], X[:, 1:2]))
        for _ in range(50):
            m.validate()
        print("50 validations on %d points: %s" % (a.reduce, m.validate()["raw"]))
        return
    m.set_validation()
    X, u = s["X_test"], s["u_test"]
    n, k = a.iters, a.every

    def step():
        m.h.step(n, False)

    def step_validate():
        return m.h.step_validate(n, k)

    def host():
        return [(m.h.step(k, False), m.rel_l2_error(X, u))[1] for _ in range(n // k)]

    routes = [("step", step), ("step_validate", step_validate), ("host", host)]
    for _, f in routes:      # untimed: graph capture, batch creation
        f()
    t = {name: [] for name, _ in routes}
    for _ in range(a.repeats):
        for name, f in routes:
            t0 = time.perf_counter()
            f()
            t[name].append((time.perf_counter() - t0) / n * 1e6)
    print("config 4, %d validation points, %d iterations per call, a sample every %d, %d repeats; graphs in use: %s; %s"
          % (X.shape[0], n, k, a.repeats, m.h.graphs_in_use(), m.h.kernel_variant()))
    for name, _ in routes:
        v = sorted(t[name])
        print("%-14s us per iteration: median %.2f  min %.2f  max %.2f" % (name, v[len(v) // 2], v[0], v[-1]))
    rows = step_validate()
    print("last curve: rel L2 error %.4e -> %.4e" % (np.sqrt(rows[0, 0] / rows[0, 1]), np.sqrt(rows[-1, 0] / rows[-1, 1])))
    ok = sorted(t["step_validate"])[a.repeats // 2] <= sorted(t["host"])[a.repeats // 2]
    print("acceptance (step_validate not slower than the host route): %s" % ("met" if ok else "NOT MET"))


if __name__ == "__main__":
    main()
