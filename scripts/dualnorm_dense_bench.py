"""The projection kernel of a linear handle under the three residual norms -- l2 (k_project_lin), the table dual norm
(k_project_lin_dual) and the dense dual norm (k_project_lin_dense, hpv_set_residual_gram) -- in one run, the variants interleaved.

    python scripts/dualnorm_dense_bench.py [--reps 7] [--iters 200]

Shapes: 16 x 16 box elements of 10 x 10 points / 5 x 5 functions and of 12 x 12 / 10 x 8, and the same grids as mapped (unit) elements
with a full tensor, where the table norm does not exist.  Microseconds of the projection kernel class per iteration (hipEvents around
the launch, hpv_kernel_time_ms(1), eager launches), median and min..max over the repetitions.  On a build without
hpv_set_residual_gram the dense column is left out, so the same script measures the parent commit.  No gate: profiles/dual_norm_dense.md
records the figures."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def handle(nex, ney, q, nt, L, norm, mapped, seed=3):
    from hp_vpinns_amd import GaussLobattoJacobiWeights, _lib
    from hp_vpinns_amd.init import xavier_init
    from hp_vpinns_amd.quadrature import gram_stacks
    from hp_vpinns_amd.testfcn import tables_1d
    x, w = GaussLobattoJacobiWeights(q, 0, 0)
    h = _lib.Handle(_lib.PDE_LINEAR2D, 1, _lib.ACT_TANH, L, lr=1e-3, lossb_weight=10.0)
    h.set_quadrature(x, w, x, w)
    h.set_tables(tables_1d(nt[0], x), tables_1d(nt[1], x))
    gx, gy = np.linspace(-1, 1, nex + 1), np.linspace(-1, 1, ney + 1)
    ne, n = nex * ney, nex * ney * q * q
    boxes = np.array([[gx[i], gx[i + 1], gy[j], gy[j + 1]] for i in range(nex) for j in range(ney)])
    Jx, Jy = (boxes[:, 1] - boxes[:, 0]) / 2, (boxes[:, 3] - boxes[:, 2]) / 2
    if mapped:                                           # the same boxes as unit elements: the geometry folded into a tensor
        S, T = np.meshgrid(x, x)
        X = np.stack([boxes[:, 0:1] + Jx[:, None] * (S.reshape(-1)[None, :] + 1), boxes[:, 2:3] + Jy[:, None] * (T.reshape(-1)[None, :] + 1)], 1)
        h.set_element_points(X)
        planes = np.zeros((7, n))
        planes[0], planes[3] = np.repeat(Jy / Jx, q * q), np.repeat(Jx / Jy, q * q)
        h.set_operator_tensor(planes)
    else:
        h.set_element_boxes(boxes)
        planes = np.zeros((5, n))
        planes[:2] = 1.0
        h.set_operator(planes)
    rng = np.random.default_rng(seed)
    h.set_rhs(rng.standard_normal(ne * nt[0] * nt[1]))
    if norm == "tables":
        sx, sy = gram_stacks(nt[0]), gram_stacks(nt[1])
        h.set_residual_norm(_lib.NORM_DUAL, 0.0, sx[0], sx[1], sy[0], sy[1])
    elif norm == "dense":
        from hp_vpinns_amd.quadrature import gram_factors, gram_rule
        ng = gram_rule(*nt)[0].size
        A = np.zeros((ne, ng * ng, 2, 2))
        A[:, :, 0, 0], A[:, :, 1, 1] = Jx[:, None], Jy[:, None]
        h.set_residual_gram(gram_factors(2, nt[0], nt[1], nt[0], nt[1], A))
    Xb = rng.uniform(-1, 1, (80, 2))
    h.set_data(Xb, np.sin(Xb[:, 0]) * Xb[:, 1])
    h.set_params(xavier_init(L, 7))
    return h


def main():
    from hp_vpinns_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    L = [2, 20, 20, 20, 1]
    dense = hasattr(_lib.Handle, "set_residual_gram")
    for mapped in (False, True):
        for q, nt in ((10, (5, 5)), (12, (10, 8))):
            norms = ["l2"] + ([] if mapped else ["tables"]) + (["dense"] if dense else [])
            hs = {k: handle(16, 16, q, nt, L, k, mapped) for k in norms}
            t = {k: [] for k in hs}
            for h in hs.values():
                h.step(a.iters, False)                   # clocks up
            for _ in range(a.reps):
                for k, h in hs.items():
                    h.enable_timing(True)
                    h.step(a.iters, False)
                    t[k].append(h.kernel_time_ms(1)[0] * 1e3)
                    h.enable_timing(False)
            print(json.dumps(dict(shape="16x16 %s of %dx%d/%dx%d" % ("mapped elements" if mapped else "boxes", q, q, nt[0], nt[1]),
                                  variants={k: h.kernel_variant() for k, h in hs.items()},
                                  loss_finite={k: bool(np.all(np.isfinite(h.loss_and_grad(False)[0]))) for k, h in hs.items()},
                                  project_us={k: dict(median=float(np.median(v)), min=min(v), max=max(v)) for k, v in t.items()})))


if __name__ == "__main__":
    main()
