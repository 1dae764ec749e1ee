"""tests/ansatz_reference.py on the CPU (no GPU): its two derivations of the loss under the ansatz u = G + D N agree, the gradient is
the loss's, the identity ansatz is linear_reference's loss, the condition holds exactly where D vanishes -- and the C-ABI carries
hpv_set_ansatz in the header, in _lib.EXPORTS and in the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import ansatz_reference as ar
import ident_reference as ir
import linear_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGREE = 1e-12      # the two derivations: the same fp64 operations in another order, a few hundred roundings on sums of O(1) terms
HOST_CASES = ["1d-21-lin-d17", "1d-21-nl-d1", "2d-180-lin-d17", "2d-180-nl-d17", "2d-180-id-d1", "2d-840-id-d17"]
_P = {}


def _problem(name, kind="generic"):
    if (name, kind) not in _P:
        _P[(name, kind)] = ar.problem(ar.CASES[name], kind)
    return _P[(name, kind)]


@pytest.mark.parametrize("name", HOST_CASES)
def test_the_two_derivations_agree(name):
    p = _problem(name)
    l3a, ga, _ = ar.reference(p)
    l3b, gb = ar.reference_autograd(p)
    e3 = np.abs(l3a - l3b) / np.abs(l3b)
    eg = np.abs(ga - gb) / np.abs(gb)
    print("%s: loss %s, worst gradient entry %.2e, coefficient slots %s" % (name, e3, eg.max(), eg[p["theta"].size:]))
    assert e3.max() < AGREE and eg.max() < AGREE
    assert ga.size == p["full"].size and np.all(ga[p["theta"].size:] != 0.0) and l3a[1] > 0 and l3a[0] > l3a[2]


@pytest.mark.parametrize("name", ["1d-21-nl-d1", "2d-180-id-d17"])
def test_gradient_against_central_differences(name):
    p = _problem(name)
    g = ar.reference(p)[1]
    rng = np.random.default_rng(5)
    nth = p["theta"].size
    idx = list(rng.choice(nth, 4, replace=False)) + list(range(nth, p["full"].size))
    h = 1e-6      # central difference of a smooth loss: h^2 |l'''| / 6 + eps |l| / h ~ 1e-10 |l|; the bound leaves two orders
    for i in idx:
        e = np.zeros_like(p["full"])
        e[i] = h
        fd = (ar.reference(p, p["full"] + e)[0][0] - ar.reference(p, p["full"] - e)[0][0]) / (2 * h)
        assert abs(fd - g[i]) < 1e-8 * max(1.0, np.linalg.norm(g)), (name, i, fd, g[i])


@pytest.mark.parametrize("name", ["1d-21-lin-d17", "2d-180-lin-d17"])
def test_identity_ansatz_is_the_linear_reference_exactly(name):
    p = _problem(name, "identity")
    l3, g, R = ar.reference(p)
    l3o, go, Ro = lr.reference(p)
    assert np.array_equal(l3, l3o) and np.array_equal(R, Ro) and np.array_equal(g, go)


@pytest.mark.parametrize("name", ["1d-21-lin-d1", "2d-180-nl-d1"])
def test_condition_is_exact_where_d_vanishes(name):
    p = _problem(name, "vanishing")
    dim = p["dim"]
    rng = np.random.default_rng(11)
    X = rng.uniform(-1.0, 1.0, (24, dim))
    X[np.arange(24), rng.integers(0, dim, 24)] = rng.choice([-1.0, 1.0], 24)      # every point on a side of [-1, 1]^dim
    A = ar.planes("vanishing", X)
    assert np.all(A[1 + dim] == 0.0)
    for seed in range(3):
        full = p["full"] + np.random.default_rng(seed).standard_normal(p["full"].size)
        assert np.array_equal(ar.predict(p, X, full), A[0])


def test_cabi_carries_hpv_set_ansatz():
    from hp_vpinns_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hpvpinn.h")).read()
    assert re.search(r"\bint\s+hpv_set_ansatz\s*\(\s*hpv_handle\s+h\s*,\s*int\s+which\s*,\s*const\s+double\s*\*\s*planes\s*,\s*size_t\s+n\s*\)\s*;", hdr)
    for k, v in (("QUAD", 0), ("DATA", 1), ("FLUX", 2), ("VALID", 3)):
        assert re.search(r"#define\s+HPV_ANSATZ_%s\s+%d\b" % (k, v), hdr) and getattr(_lib, "ANSATZ_" + k) == v
    assert "hpv_set_ansatz" in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(_lib.LIB_PATH + " is missing: build it first (__graft_entry__.build())")
    assert ctypes.CDLL(_lib.LIB_PATH).hpv_set_ansatz is not None
