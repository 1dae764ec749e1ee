"""tests/dualnorm_reference.py and the host side of the dual-norm residual loss on the CPU (no GPU): the closed-form Gram matrices
against an independent quadrature, the eigen tables, every case of the GPU test's table on the reference alone (table route against
dense solve, two derivations, central differences, the condition of d), the estimator identity, and the keyword of the Python classes.
profiles/dual_norm.md holds the measured figures the bounds take their margins from."""
import numpy as np
import pytest

import dualnorm_reference as dn
import linop_sweep as ls

CASES = dn.cases()


@pytest.mark.parametrize("n", [1, 2, 5, 10, 17, 20])
def test_closed_form_gram_matrices_against_quadrature(n):
    from hp_vpinns_amd.quadrature import gram_1d
    K, M = gram_1d(n)
    Kq, Mq = dn.gram_quadrature(n)
    eK, eM = np.abs(K - Kq).max() / np.abs(Kq).max(), np.abs(M - Mq).max() / np.abs(Mq).max()
    print("n = %d: K %.2e, M %.2e" % (n, eK, eM))
    assert np.count_nonzero(K - np.diag(np.diag(K))) == 0 and np.array_equal(M, M.T)
    assert max(eK, eM) < 1e-11                       # (measured: 2.3e-12 or better)


@pytest.mark.parametrize("n", [1, 2, 5, 17, 20])
def test_eigen_tables(n):
    from hp_vpinns_amd.quadrature import gram_1d, gram_eig, gram_stacks
    K, M = gram_1d(n)
    S, lam = gram_eig(n)
    assert np.all(lam > 0.0) and np.all(np.diff(lam) > 0.0)
    assert np.abs(S.T @ M @ S - np.eye(n)).max() < 1e-12 and np.abs(S.T @ K @ S - np.diag(lam)).max() < 1e-12 * lam.max()
    St, lt = gram_stacks(n)
    assert St.shape == (n, n, n) and lt.shape == (n, n)
    for m in range(1, n + 1):                        # count m in its leading block, zeros behind it
        Sm, lm = gram_eig(m)
        assert np.array_equal(St[m - 1, :m, :m], Sm) and np.array_equal(lt[m - 1, :m], lm)
        assert not St[m - 1, m:].any() and not St[m - 1, :, m:].any() and not lt[m - 1, m:].any()
    if n == 17:
        print("n = 17: lam in [%.4g, %.4g], cond(S) = %.3g" % (lam.min(), lam.max(), np.linalg.cond(S)))
        assert abs(lam.min() - np.pi ** 2 / 4) < 1e-6 and 3.6e3 < lam.max() < 3.8e3 and np.linalg.cond(S) < 14.0


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case_meets_its_conditions_at_its_recorded_seed(c):
    assert c["seed"] == dn.SEEDS[c["name"]]
    r = dn.conditions(c)
    print(c["name"], c["seed"], r["fig"])
    assert r["ok"], (c["name"], c["seed"], r["why"])


def test_the_table_is_the_one_that_was_asked_for():
    by = {c["name"]: c for c in CASES}
    rows = {c["row"] for c in CASES}
    assert rows == {"min", "nty1", "nr272", "tall", "wide", "counts", "padx", "ldsmax", "1d-min", "1d-272", "1d-append", "2d-append"}
    assert all("%s-lin" % r in by for r in rows)
    for r in ("nr272", "counts"):
        assert {"%s-nl" % r, "%s-id" % r} <= set(by)
    assert by["counts-lin-ansatz"]["ansatz"] == "generic"
    for m in (0.0, 3.0):
        assert len({c["row"] for c in CASES if c["mass"] == m}) >= 2
    # counts: 1 and the maxima among the owned counts, unequal half widths, one owned box with aspect ratio >= 20
    c = by["counts-lin"]
    eb, ee = c["shard"]
    for n, top in zip(c["counts"], c["nt"]):
        assert min(n[eb:ee]) == 1 and max(n[eb:ee]) == top
    asp = [(b[1] - b[0]) / (b[3] - b[2]) for b in c["boxes"][eb:ee]]
    assert max(max(asp), 1 / min(asp)) >= 20 and len(set(asp)) == len(asp)
    # the scratch: aliased on every row of the issue, ldsmax included (it runs); appended on the two rows added for that path; a
    # 1-D shape hpv_set_tables admits whose appended scratch is past the limit
    for c in CASES:
        _, qx, qy, ntx, nty = ls.shape(c)
        b, aliased = dn.lds_bytes(qx, qy, ntx, nty)
        assert aliased == (not c["row"].endswith("append")) and b <= ls.LDS_LIMIT, (c["name"], b)
        assert (b == ls.lds_bytes(qx, qy, ntx, nty)) == aliased
    assert ls.lds_bytes(*dn.REFUSED_1D) <= ls.LDS_LIMIT < dn.lds_bytes(*dn.REFUSED_1D)[0] and not dn.lds_bytes(*dn.REFUSED_1D)[1]


ESTIMATOR = {"2d": (2, [[-1.0, -0.2, -1.0, 0.1], [-0.2, 1.0, -1.0, -0.3]], 8, 4, 7301), "1d": (1, [[-0.35, 0.5]], 8, 4, 7302)}


@pytest.mark.parametrize("name", list(ESTIMATOR))
def test_estimator_identity(name):
    """kappa = 1, beta = sigma = 0, mass = 0, channels from a polynomial pt and F from a polynomial u, both integrated exactly by
    the rule: sum_e loss_e = |P_h(pt - u)|^2_{H^1}, the energy of the error's projection onto the bubble spaces"""
    dim, boxes, q, nt, seed = ESTIMATOR[name]
    p, planes, cu, cp, X = dn.estimator_problem(dim, boxes, q, nt, seed)
    loss, energy = dn.estimator_loss(p, planes, cp, X), dn.projected_error_energy(p, cu, cp)
    e = abs(loss - energy) / energy
    print("estimator identity %s: loss %.15e, |P_h(pt - u)|^2 %.15e, relative difference %.2e" % (name, loss, energy, e))
    assert energy > 1e-3
    assert e < dn.ESTIMATOR_TOL                      # (measured 2d 4.6e-15, 1d 2.6e-15: profiles/dual_norm.md)


def test_keyword_of_the_python_classes():
    from hp_vpinns_amd.vpinn import VPINNLinear
    chk = VPINNLinear._check_residual_norm
    assert chk("l2") == ("l2", 0.0) and chk("dual") == ("dual", 0.0) and chk(dict(kind="dual", mass=3)) == ("dual", 3.0)
    for bad in ("h1", None, dict(kind="dual", mass=-1.0), dict(kind="l2", mass=1.0), dict(kind="dual", weight=1.0), dict(mass=1.0),
                dict(kind="dual", mass=float("nan"))):
        with pytest.raises(ValueError):
            chk(bad)


def test_the_patch_of_the_reference_is_undone():
    import ident_reference as ir
    orig = ir._loss
    with dn._dual(0.0):
        assert ir._loss is not orig
    assert ir._loss is orig
