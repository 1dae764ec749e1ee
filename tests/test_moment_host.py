"""tests/moment_reference.py, the CPU reference of the integral constraints (hpv_set_moments), proved on the host: its gradient against
central differences, exactness of the integrals it forms, the product's folded measure (vpinn.VPINNLinear._fold_measure) against the
physical one, and -- for the exact inputs of tests/test_gpu_moments.py -- that the constraint part is between 10 % and 90 % of the
total gradient norm at theta0, so that neither part of the gradient can hide an error in the other.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

import linear_reference as lr
import mapped_reference as mr
import moment_reference as mo
from cases import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["1d-7", "5x5-sigma", "8x8-row-hardbc-u3", "6x5-quads-K8"])
def test_gradient_against_central_differences(name):
    p, t = mo.case(name)
    th = mo.full0(p)
    rng = np.random.default_rng(3)
    h = 6e-6                                             # eps^(1/3): truncation and rounding both ~ h^2 = 4e-11 relative
    for _ in range(3):
        d = rng.standard_normal(th.size)
        d /= np.linalg.norm(d)
        for part, key in (("triple", "grad"),):
            fd = (mo.terms(p, th + h * d)[part][0] - mo.terms(p, th - h * d)[part][0]) / (2 * h)
            an = float(t[key] @ d)
            assert abs(fd - an) < 1e-6 * max(1.0, np.linalg.norm(t[key])), (name, fd, an)
    assert np.allclose(t["grad"], t["grad_res"] + t["grad_con"], rtol=0, atol=0)
    assert np.isclose(t["triple"][2], t["loss_e"].sum() + t["pen"].sum(), rtol=1e-14)


def test_the_area_of_the_quarter_annulus():
    """int 1 over r in (1, 2), theta in (0, pi / 2), four polar elements: 3 pi / 4 (the integrand r is linear in r, constant in theta)"""
    rx = ry = lr.rule(6, 0)
    rt = np.array([[1.0, 1.5, 0.0, np.pi / 4], [1.5, 2.0, 0.0, np.pi / 4], [1.0, 1.5, np.pi / 4, np.pi / 2], [1.5, 2.0, np.pi / 4, np.pi / 2]])
    X, A = mr.geom_polar(rt, rx[0], ry[0])
    p = dict(xr=rx, yr=ry, eb=0, ee=4, mom=[dict(rho=np.ones(X.shape[:2]), power=1), dict(rho=np.ones(X.shape[:2]), power=2)])
    I = mo.moments(p, torch.ones(X.shape[:2], dtype=torch.float64), torch.linalg.det(torch.tensor(A))).numpy()
    assert np.allclose(I, 3 * np.pi / 4, rtol=1e-14)


def test_a_polynomial_mean_is_exact_on_a_rule_that_integrates_it():
    """a 5-point Gauss-Lobatto rule integrates degree 7: u = x^3 y^2 + x - 2, u^2 of degree (6, 4), on the boxes of case B"""
    rx = ry = lr.rule(5, 0)
    X, A = mr.geom_boxes(mo.BOXES_B, rx[0], ry[0])
    x, y = X[..., 0], X[..., 1]
    u = torch.tensor(x ** 3 * y ** 2 + x - 2.0)
    p = dict(xr=rx, yr=ry, eb=0, ee=4, mom=[dict(rho=np.ones(x.shape), power=1), dict(rho=np.ones(x.shape), power=2), dict(rho=x * y, power=1)])
    I = mo.moments(p, u, torch.linalg.det(torch.tensor(A))).numpy()
    # over [-1, 1]^2: int u = -8;  int u^2 = int x^6 y^4 + x^2 + 4 + 2 x^4 y^2 = 4/35 + 4/3 + 16 + 8/15;  int x y u = 0
    assert np.allclose(I, [-8.0, 4 / 35 + 4 / 3 + 16 + 8 / 15, 0.0], rtol=1e-13, atol=1e-14)


def _cut(p):
    (xi, wx), (yi, wy) = p["xr"], p["yr"]
    qx, qy, ne = xi.size, yi.size, p["X"].shape[0]
    cut = lambda a: np.ascontiguousarray(a.reshape((ne, qy, qx) + a.shape[2:])[:, :qy - 1, :qx - 1]).reshape((ne, (qy - 1) * (qx - 1)) + a.shape[2:])
    q = dict(p, xr=(xi[:-1], wx[:-1]), yr=(yi[:-1], wy[:-1]), X=cut(p["X"]), A=cut(p["A"]), coefs={k: cut(v) for k, v in p["coefs"].items()})
    q["mom"] = [dict(t, rho=cut(t["rho"])) for t in p["mom"]]
    return q


def test_the_padded_rule_reproduces_the_unpadded_one():
    p, t = mo.case("6x5-padded")
    assert p["xr"][1][-1] == 0.0 and p["yr"][1][-1] == 0.0
    c = mo.terms(_cut(p))
    assert np.allclose(t["I"], c["I"], rtol=1e-14) and np.allclose(t["triple"], c["triple"], rtol=1e-13)
    assert np.allclose(t["grad"], c["grad"], rtol=1e-11, atol=1e-14 * np.abs(c["grad"]).max())


@pytest.mark.parametrize("name", list(mo.CASES))
def test_the_folded_measure_is_the_physical_one(name):
    """boxes: weight x the half widths' product; quadrilaterals: weight x det A of the product's own MappedMesh geometry"""
    from hp_vpinns_amd.adapt import MappedMesh
    from hp_vpinns_amd.vpinn import VPINNLinear
    p, _ = mo.case(name)
    (xi, wx), (yi, wy) = p["xr"], p["yr"]
    w = np.outer(wy, wx).reshape(-1)
    ne, nq = p["X"].shape[:2]
    if p["kind"] == "quads":
        A = MappedMesh.from_quads(mo.QUADS, p["nax"], p["nay"]).geometry(xi, yi, 0, ne)[1]
        jac = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    else:
        b = p["boxes"]
        jac = np.repeat(np.prod([(b[:, 2 * a + 1] - b[:, 2 * a]) / 2 for a in range(p["dim"])], axis=0), nq)
    rho = np.stack([t["rho"].reshape(-1) for t in p["mom"]], 0)
    m = VPINNLinear._fold_measure(rho, w, jac)
    ref = mo.physical_measure(p)
    assert np.allclose(m, ref, rtol=1e-13, atol=0.0)
    pad = np.tile(w, ne) == 0.0
    assert np.all(m[:, pad] == 0.0) and (name != "6x5-padded" or pad.any())


@pytest.mark.parametrize("name", list(mo.CASES))
def test_neither_part_of_the_gradient_hides_the_other(name):
    p, t = mo.case(name)
    share = np.linalg.norm(t["grad_con"]) / np.linalg.norm(t["grad"])
    print("%s: constraint part %.3f of the total gradient norm; I %s targets %s weight %.3e" % (
        name, share, t["I"], [k["target"] for k in p["mom"]], p["mom"][0]["weight"]))
    assert 0.1 <= share <= 0.9, (name, share)
    assert np.all(t["pen"] > 0.0) and all(k["weight"] >= 0.0 for k in p["mom"])
    if len(p["mom"]) > 1:                                # a density that changes sign
        assert any(np.any(k["rho"] > 0) and np.any(k["rho"] < 0) for k in p["mom"])


def test_the_constraint_changes_what_is_computed():
    """the reference alone tells the term from its absence, and a wrong power or a lost sign of the density is of order one"""
    p, t = mo.case("6x5-quads-K8")
    none = mo.terms(p, mom=[])
    assert abs(none["triple"][0] - t["triple"][0]) > 1e-3 * abs(t["triple"][0])
    swapped = mo.terms(p, mom=[dict(k, power=3 - k["power"]) for k in p["mom"]])
    assert rel(swapped["grad"], t["grad"]) > 1e-2


def test_header_and_exports_are_in_step():
    from hp_vpinns_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hpvpinn.h")).read()
    assert "int hpv_set_moments(hpv_handle h, int n_terms, const int* power, const double* measure, size_t n, const double* target, const double* weight);" in hdr
    assert "int hpv_read_moments(hpv_handle h, double* values, double* penalties, int n_terms);" in hdr
    assert "#define HPV_MAX_MOMENTS 8" in hdr and _lib.MAX_MOMENTS == 8
    assert "hpv_set_moments" in _lib.EXPORTS and "hpv_read_moments" in _lib.EXPORTS


def test_class_keyword_is_checked_on_the_host():
    from hp_vpinns_amd.vpinn import VPINNLinear
    chk = VPINNLinear._check_constraints
    c = chk([dict(name="m", kind="mean", target=0.5, weight=3.0), dict(name="n", kind="l2", target=1.0), dict(name="d", kind="moment", density=np.ones(4), power=1)])
    assert [k["power"] for k in c] == [1, 2, 1] and c[0]["density"] is None and c[1]["weight"] == 1.0
    assert chk(None) == [] and chk([]) == []
    for bad, msg in (([dict(name="a", kind="mean", power=2)], "fixes"), ([dict(name="a", kind="moment", power=3)], "power is 1 or 2"),
                     ([dict(name="a", kind="moment")], "needs power"), ([dict(name="a", kind="l2", weight=-1.0)], "not negative"),
                     ([dict(name="a", kind="l2", target=np.nan)], "finite"), ([dict(name="a", kind="l2")] * 2, "names"),
                     ([dict(name=str(i), kind="l2") for i in range(9)], "at most 8"), ([dict(kind="l2")], "constraint is"),
                     ([dict(name="a", kind="max")], "constraint is")):
        with pytest.raises(ValueError, match=msg):
            chk(bad)
