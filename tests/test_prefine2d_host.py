"""Per-element test-function counts of the 2-D drivers (p-refinement, P2:72-73 / P3:112-113): the host side -- what the restated
driver set-ups return for per-column / per-row counts and how the class surface turns the reference's F_ext_total[ex, ey] blocks into
the dense array of the C-ABI.  No GPU."""
import numpy as np
import pytest


def test_poisson2d_setup_returns_the_blocks_of_the_uniform_setup():
    """poisson2d.setup with one count per element column / row: every block is the corner of the uniform 5 x 5 set-up's block, bit for
    bit (the Legendre-difference family is nested: the first n rows of a larger table are the smaller table)."""
    from hp_vpinns_amd.drivers import poisson2d
    nax, nay = [5, 3, 4], [2, 5]
    dense = poisson2d.setup(N_el_x=3, N_el_y=2, N_test_x=5, N_test_y=5, N_quad=12, with_test_grid=False)
    s = poisson2d.setup(N_el_x=3, N_el_y=2, N_test_x=nax, N_test_y=nay, N_quad=12, with_test_grid=False)
    assert dense["F_ext_total"].shape == (3, 2, 5, 5)            # (an integer means what it always meant)
    assert dense["N_testfcn_total"] == [[5, 5, 5], [5, 5]]
    assert s["N_testfcn_total"] == [nax, nay]
    F = s["F_ext_total"]
    assert F.dtype == object and F.shape == (3, 2)
    for ex in range(3):
        for ey in range(2):
            assert F[ex, ey].shape == (nay[ey], nax[ex])
            assert np.array_equal(F[ex, ey], dense["F_ext_total"][ex, ey][:nay[ey], :nax[ex]])
    for k in ("X_u_train", "u_train", "XY_quad_train", "WXY_quad_train", "grid_x", "grid_y"):
        assert np.array_equal(s[k], dense[k])
    with pytest.raises(ValueError):
        poisson2d.setup(N_el_x=3, N_el_y=2, N_test_x=[5, 3], N_test_y=nay, N_quad=12, with_test_grid=False)


def test_advdiff_setup_returns_the_per_column_and_per_row_lists():
    from hp_vpinns_amd.drivers import advdiff
    s = advdiff.setup(N_el_x=3, N_el_t=2, N_test_x=[5, 3, 4], N_test_t=[2, 5], N_quad=12, with_test_grid=False)
    assert s["N_testfcn_total"] == [[5, 3, 4], [2, 5]]
    u = advdiff.setup(N_el_x=3, N_el_t=2, N_test_x=5, N_test_t=4, N_quad=12, with_test_grid=False)
    assert u["N_testfcn_total"] == [[5, 5, 5], [4, 4]]
    with pytest.raises(ValueError):
        advdiff.setup(N_el_x=3, N_el_t=2, N_test_x=[5, 3, 4], N_test_t=[2], N_quad=12, with_test_grid=False)


def test_blocks_are_padded_to_the_dense_right_hand_side():
    """vpinn._dense_rhs_2d / _counts_2d: object array, nested list and dense array give the same (nex, ney, max nty, max ntx) array;
    a block whose shape contradicts the counts is a ValueError; the pairs are flattened e = ex * ney + ey."""
    from hp_vpinns_amd.drivers import poisson2d
    from hp_vpinns_amd.vpinn import _counts_2d, _dense_rhs_2d
    s = poisson2d.setup(N_el_x=3, N_el_y=2, N_test_x=[5, 3, 4], N_test_y=[2, 5], N_quad=12, with_test_grid=False)
    nax, nay, nax_e, nay_e, ragged = _counts_2d(s["N_testfcn_total"])
    assert ragged and list(nax_e) == [5, 5, 3, 3, 4, 4] and list(nay_e) == [2, 5, 2, 5, 2, 5]
    assert not _counts_2d([[4, 4], [3]])[4]
    F = s["F_ext_total"]
    D = _dense_rhs_2d(F, nax, nay)
    assert D.shape == (3, 2, 5, 5)
    for ex in range(3):
        for ey in range(2):
            assert np.array_equal(D[ex, ey, :nay[ey], :nax[ex]], F[ex, ey])
            assert not D[ex, ey, nay[ey]:, :].any() and not D[ex, ey, :, nax[ex]:].any()
    assert np.array_equal(_dense_rhs_2d([[F[ex, ey] for ey in range(2)] for ex in range(3)], nax, nay), D)
    assert _dense_rhs_2d(D, nax, nay) is not None and np.array_equal(_dense_rhs_2d(D, nax, nay), D)
    bad = F.copy()
    bad[1, 0] = np.zeros((3, 3))
    with pytest.raises(ValueError):
        _dense_rhs_2d(bad, nax, nay)
    with pytest.raises(ValueError):
        _dense_rhs_2d(D[:, :, :4], nax, nay)
    with pytest.raises(ValueError):
        _counts_2d([[5, 0], [3]])


def test_the_new_entry_point_is_declared_bound_and_documented():
    import os
    from hp_vpinns_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "hpvpinn.h")).read()
    assert "int hpv_set_active_tests_2d(hpv_handle h, const int* nax, const int* nay, int n);" in hdr
    assert "hpv_set_active_tests_2d" in _lib.EXPORTS and hasattr(_lib.Handle, "set_active_tests_2d")
    assert "hpv_set_active_tests_2d" in open(os.path.join(root, "INTEGRATION.md")).read()
