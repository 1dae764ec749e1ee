"""tests/ident_reference.py on the CPU: every d lossv / d c_m of its autograd against central differences of its own loss, the
conditions (a) - (c), (e), (f) of its docstring for every case of the table (the seeds were chosen here), its agreement with
nonlinear_reference at baked-in coefficients, and the host side of the feature (header, exports, the Python layout of the slots).

Tolerance of the difference quotients: with step h = 1e-5 on coefficients of size 0.3 .. 0.9 the central difference carries a
truncation error of order h^2 |lossv'''| ~ 1e-10 |lossv| and a rounding error of order 1e-16 |lossv| / h = 1e-11 |lossv|; relative to
|d lossv / d c| ~ |lossv| both stay below 1e-9.  Observed over the table: at most 2e-9 of the gradient's norm (printed per case), so
FD_TOL = 2e-8 leaves a factor of ten."""
import os

import numpy as np
import pytest

import ident_reference as ir
import nonlinear_reference as nr

FD_TOL = 2e-8
FD_H = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = {}


def _problem(name):
    if name not in _P:
        _P[name] = ir.problem(ir.CASES[name])
    return _P[name]


@pytest.mark.parametrize("name", list(ir.CASES))
def test_coefficient_gradient_against_central_differences(name):
    p = _problem(name)
    nth = p["theta"].size
    g = ir.var_part(p)["grad"][nth:]
    fd = np.zeros_like(g)
    for m in range(g.size):
        hi, lo = p["full"].copy(), p["full"].copy()
        hi[nth + m] += FD_H
        lo[nth + m] -= FD_H
        fd[m] = (ir.var_part(p, hi, grad=False)["lossv"] - ir.var_part(p, lo, grad=False)["lossv"]) / (2 * FD_H)
    e = float(np.max(np.abs(fd - g)) / np.linalg.norm(g))
    print("%s: d c by autograd %s | central differences: worst entry %.2e of the norm" % (name, g, e))
    assert np.all(g != 0.0) and e < FD_TOL, (name, g, fd)


@pytest.mark.parametrize("name", list(ir.CASES))
def test_conditions_hold_on_the_reference_alone(name):
    fig = ir.conditions(_problem(name))
    print(name, fig)


@pytest.mark.parametrize("name", ["2d-h8", "1d-sin", "2d-nl-over-zero-base"])
def test_baked_in_coefficients_are_the_nonlinear_reference(name):
    """the same loss, residuals and network gradient from nonlinear_reference on planes with c_m D_m added on the host; the data and
    flux terms leave the coefficients' gradient alone"""
    p = _problem(name)
    planes, nl = ir.effective(p, p["c0"])
    l3, g, R = ir.reference(p)
    l3b, gb, Rb = nr.reference(p, planes=planes, nl=nl)
    nth = p["theta"].size
    assert np.allclose(l3, l3b, rtol=1e-13, atol=0) and np.allclose(R, Rb, rtol=1e-12, atol=1e-16)
    assert np.linalg.norm(g[:nth] - gb) < 1e-12 * np.linalg.norm(gb)
    assert np.array_equal(g[nth:], ir.var_part(p)["grad"][nth:])


def test_adam_trajectory_moves_network_and_coefficients():
    p = _problem("2d-h8")
    full, m, v = ir.adam_trajectory(p, 2)
    nth = p["theta"].size
    assert np.all(full[nth:] != p["full"][nth:]) and np.any(full[:nth] != p["full"][:nth]) and np.all(v >= 0.0) and m.shape == full.shape


def test_header_exports_and_python_layout():
    from hp_vpinns_amd import _lib
    from hp_vpinns_amd.init import n_params, pad_plan
    hdr = open(os.path.join(ROOT, "include", "hpvpinn.h")).read()
    assert "int hpv_create_ex(hpv_handle* out, const hpv_config* cfg, int n_coef);" in hdr
    assert "int hpv_set_trainable(hpv_handle h, const double* dirs, size_t n);" in hdr and "#define HPV_MAX_COEF 8" in hdr
    assert {"hpv_create_ex", "hpv_set_trainable"} <= set(_lib.EXPORTS) and hasattr(_lib.Handle, "set_trainable") and _lib.MAX_COEF == 8
    # pad_plan keeps `extra` slots behind the padded network, in order, for extra > 1
    for L in ([2, 8, 8, 1], [1, 8, 8, 1], [2, 5, 5, 5, 1]):
        for extra in (1, 2, 8):
            plan = pad_plan(L, extra)
            if plan is None:
                continue
            dev, idx = plan
            idx = np.asarray(idx)
            assert idx.size == n_params(L, extra) and np.array_equal(idx[-extra:], n_params(dev, 0) + np.arange(extra))
            assert np.all(idx[:-extra] < n_params(dev, 0)) and np.array_equal(idx[:-extra], np.asarray(pad_plan(L, 0)[1]))


@pytest.mark.parametrize("name", ["conductivity", "burgers-nu"])
def test_driver_step_counts_give_a_recovery_on_the_reference(name):
    """drivers/identify.SMALLEST_STEPS were chosen here: after that many TF1-Adam steps of the CPU reference on the driver's smallest
    problem every coefficient's error is below a tenth of its initial one (tests/test_gpu_ident.py bounds the device by twice it)"""
    from hp_vpinns_amd.drivers import identify as drv
    kw = dict(drv.SMALLEST[name])
    s = drv.setup(kw.pop("problem"), **kw)
    p = ir.from_model(ir.host_model(s, LR=drv.SMALLEST_LR))
    full, _, _ = ir.adam_trajectory(p, drv.SMALLEST_STEPS[name], lr_=drv.SMALLEST_LR)
    true = np.array(list(s["true"].values()))
    e0, e = np.abs(p["c0"] - true), np.abs(full[-true.size:] - true)
    print(name, "initial errors", e0, "after", drv.SMALLEST_STEPS[name], "steps", e)
    assert np.all(e < e0 / 10.0)
