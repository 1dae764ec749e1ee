"""Microseconds per iteration of the three scheme='PINNs' runs at the drivers' default collocation counts (Poisson-1D 500,
Poisson-2D 100, AdvDiff 500 points; the drivers' default networks), one GPU: warm-up, then 5 windows of 2 000 iterations each,
bracketed by a device synchronisation on both sides (as bench.py times a window); the median window is reported
(profiles/pinn_schemes.md).

    python scripts/pinn_scheme_speed.py [--steps 2000] [--windows 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hp_vpinns_amd.drivers import advdiff, poisson1d, poisson2d  # noqa: E402
from hp_vpinns_amd.vpinn import VPINN1D  # noqa: E402


def models():
    s = poisson1d.setup()
    L = [1] + [20] * 4 + [1]
    yield "poisson1d", s["X_f_train"].shape[0], L, VPINN1D(
        s["X_u_train"], s["u_train"], s["X_quad_train"], s["W_quad_train"], s["F_ext_total"], s["grid"], s["X_test"], s["u_test"], L,
        s["X_f_train"], s["f_train"], var_form=1, lossb_weight=1, LR=0.001, scheme="PINNs")
    s = poisson2d.setup(with_test_grid=False)
    L = [2] + [5] * 3 + [1]
    yield "poisson2d", s["X_f_train"].shape[0], L, poisson2d.build_model(s, L, scheme="PINNs")
    s = advdiff.setup(with_test_grid=False)
    yield "advdiff", s["XT_f_train"].shape[0], L, advdiff.build_model(s, L, scheme="PINNs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=500)
    a = ap.parse_args()
    for name, n_col, layers, m in models():
        m._step(a.warmup, False)
        m.h.sync()
        wins = []
        for _ in range(a.windows):
            m.h.sync()
            t0 = time.perf_counter()
            m._step(a.steps, False)
            m.h.sync()
            wins.append((time.perf_counter() - t0) / a.steps * 1e6)
        print(json.dumps({"problem": name, "collocation_points": n_col, "layers": layers, "backend": m.backend(), "steps": a.steps,
                          "us_per_iteration_median": round(sorted(wins)[len(wins) // 2], 2),
                          "us_per_iteration_windows": [round(w, 2) for w in wins]}), flush=True)


if __name__ == "__main__":
    main()
