"""The HIP path against what the reference's OWN class code computed (tests/golden/*_graph.npz: the three VPINN class bodies executed
verbatim on tests/golden/tf1_shim.py by make_golden.py) -- not against the oracle.  Reads nothing but the fixtures.

Every case of reference_graph.CASES, once on the default dispatch and once with backend="generic":
  loss_and_grad()           loss triple within 1e-9, gradient within 1e-8 (the figures of test_gpu_fuzz._against_oracle), per parameter
                            block as well (no block may hide behind a larger one), d/d epsilon on its own for AdvDiff;
  K = 6 Adam updates        the loss read AFTER each update, as the reference's train() records it, within 1e-9 of the recorded list;
                            the parameters after them within STEP_TOL = 1e-8 (test_gpu_generic_point.py) through the Adam mask of
                            test_gpu_fuzz (entries whose gradient is below 1e-9 of the largest; the fixture holds at most 5 % of
                            them, asserted before the mask is used), epsilon on its own;
                            default dispatch: the step path train() runs on (`_step_record`); generic backend: eager forward_backward
                            + apply_adam with loss() after each, as test_gpu_shape_matrix.py steps (no captured graph);
  predict                   at the stored points within 1e-9 of the stored prediction's norm.
kernel_variant() of every case is printed (pytest -s / -rA).  The 2 x 2 x (60 x 60) case holds a loss and a gradient only."""
import numpy as np
import pytest

import generic_point as gp
import reference_graph as rg
from cases import rel

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL, STEP_TOL, PRED_TOL = 1e-9, 1e-8, 1e-8, 1e-9


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for k in ("HPV_FUSE", "HPV_NO_QUARTER_TILE", "HPV_NO_RULE_PADDING", "HPV_FORCE_DIST", "HPV_NO_GRAPH"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("backend", ["auto", "generic"])
@pytest.mark.parametrize("c", rg.CASES, ids=rg.case_id)
def test_device_reproduces_what_the_reference_classes_computed(c, backend):
    d, _ = rg.load(c)
    _, _, layers, n_extra = rg.setup(c)
    name = "%s[%s]" % (rg.case_id(c), backend)
    m = rg.product(c, backend=backend)
    if backend == "generic":
        assert m.backend() == "generic", (name, m.backend())
    l3, g = m.loss_and_grad()
    v = m.h.kernel_variant()
    print("%s | backend %s | %s" % (name, m.backend(), v))
    his = theta = pred = None
    if c[3]:
        big = rg.step_mask(d)                   # (asserts the 5 % cap on the fixture before the mask is used)
        assert big.size == d["theta0"].size
        if backend == "generic":
            his = []
            for _ in range(rg.K):
                m.h.forward_backward()
                m.h.apply_adam()
                his.append(m.loss()[0])
        else:
            his = m._step_record(rg.K)[0][:, 0]
        theta, pred = m.get_params(), m.predict(d["X_pred"])
    e = rg.gaps(d, layers, n_extra, l3, g, his, theta, pred)
    e["grad_global"] = rel(g, d["grad"])
    print("%s | %s" % (name, " ".join("%s %s" % (k, x if isinstance(x, str) else "%.2e" % x) for k, x in e.items())))
    assert e["loss3"] < LOSS_TOL, (name, v, "loss triple", l3, d["loss3"])
    assert e["grad_global"] < GRAD_TOL and e["grad"] < GRAD_TOL, (name, v, "gradient", e["grad_global"], gp.block_errors(g, d["grad"], layers, n_extra))
    if n_extra:
        assert e["d_eps"] < GRAD_TOL, (name, v, "d/d epsilon", g[-1], d["grad"][-1])
    if c[3]:
        assert e["his"] < LOSS_TOL, (name, v, "loss after each update", his, d["loss_his"])
        assert e["theta"] < STEP_TOL, (name, v, "parameters after %d updates" % rg.K, e["theta"])
        if n_extra:
            assert e["eps"] < STEP_TOL, (name, v, "epsilon after %d updates" % rg.K, theta[-1], d["theta_K"][-1])
        assert e["pred"] < PRED_TOL, (name, v, "prediction", e["pred"])
