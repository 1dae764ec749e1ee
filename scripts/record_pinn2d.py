"""Record the Poisson-2D strong-form (scheme='PINNs') loss, gradient and the loss after three Adam steps, generic and MFMA
backends, on the poisson2d_default fixture -- what tests/test_gpu_pinn.py compares bit for bit (tests/golden/pinn2d_recorded.npz).

    python scripts/record_pinn2d.py OUT.npz [LIBRARY.so]

LIBRARY.so: another build of libhpvpinn.so to record with (the fixture in the repository was recorded with the build of the
commit before k_pinn_residual took the problem as a parameter); default: the library in the tree."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cases import gold, p2_args, theta0  # noqa: E402

from hp_vpinns_amd import _lib  # noqa: E402
from hp_vpinns_amd.vpinn import VPINN2D  # noqa: E402


def record():
    out = {}
    for backend, layers in (("generic", [2, 8, 8, 1]), ("mfma", [2, 20, 20, 20, 1])):
        a = p2_args(gold("poisson2d_default"), layers)
        m = VPINN2D(*a, scheme="PINNs", init_params=theta0(layers, 44), backend=backend)
        l3, g = m.loss_and_grad()
        assert m.backend() == backend
        out["layers_" + backend] = np.asarray(layers)
        out["loss3_" + backend], out["grad_" + backend] = np.asarray(l3), g
        out["loss3_after3_" + backend] = np.asarray(m._step(3, True))
    return out


if __name__ == "__main__":
    if len(sys.argv) > 2:
        with _lib.library(os.path.abspath(sys.argv[2])):
            res = record()
    else:
        res = record()
    np.savez(sys.argv[1], **res)
    print({k: v.shape for k, v in res.items()})
