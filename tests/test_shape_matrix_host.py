"""The reference side of tests/test_gpu_shape_matrix.py, without a GPU: every case of tests/shape_matrix.py is well posed on the
reference alone -- every parameter block (W_l, b_l, epsilon) carries at least generic_point.BLOCK_FLOOR of the gradient norm, both loss
terms at least 1e-3 of the loss, and two CPU restatements agree per block to 1e-11 (variational: the oracle's element loop against its
vectorised path; strong form: tests/pinn_reference.py resp. OracleVPINN2D(scheme="PINNs") -- autograd applied twice -- against the
closed form shape_matrix.pinn_closed_form: forward-mode Taylor channels and a hand-derived reverse pass).  So the 1e-9 of the GPU file
leaves two orders of magnitude over the references' own spread.  And: the table lists exactly the (channel set, H, L) the dispatch
allows."""
import os
import re

import numpy as np
import pytest

import generic_point as gp
import shape_matrix as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hp_vpinns_amd", "csrc")
CASES = sm.matrix_cases() + sm.padded_cases()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case_is_well_posed_on_the_reference_alone(c):
    r = sm.conditions(c)
    print("%s seed %d scale %.2f: smallest block %.1e of the gradient, loss terms %.1e / %.1e, restatements %.1e (blocks) %.1e (loss)"
          % (c["name"], c["seed"], c["scale"], r["floor"], r["terms"][0], r["terms"][1], r["agree"], r["loss_agree"]))
    assert r["floor"] >= gp.BLOCK_FLOOR, (c["name"], r)
    assert min(r["terms"]) >= sm.TERM_FLOOR, (c["name"], r)
    assert r["agree"] <= sm.BLOCK_AGREE and r["loss_agree"] <= sm.BLOCK_AGREE, (c["name"], r)
    assert r["ok"], (c["name"], r["why"])


def test_seeds_follow_the_rule_and_are_literals():
    """every seed is base + 1000 k with k < MAX_TRIES, written down in SEEDS / PADDED_SEEDS; no two cases share one"""
    names = [c["name"] for c in CASES]
    assert set(sm.SEEDS) | set(sm.PADDED_SEEDS) == set(names) and len(set(names)) == len(names)
    for row, spec in sm.ROWS.items():
        for i, (H, L) in enumerate(spec[7]):
            k, rem = divmod(sm.SEEDS["%s-H%d-L%d" % (row, H, L)] - sm.base_seed(row, i), 1000)
            assert rem == 0 and 0 <= k < sm.MAX_TRIES, (row, H, L)
    for i, name in enumerate(sm.PADDED):
        k, rem = divmod(sm.PADDED_SEEDS[name] - (7900 + i), 1000)
        assert rem == 0 and 0 <= k < sm.MAX_TRIES, name
    seeds = [c["seed"] for c in CASES]
    assert len(set(seeds)) == len(seeds)


def _wide_widths_of_build_sh():
    src = open(os.path.join(CSRC, "build.sh")).read()
    m = re.search(r'^WIDE_WIDTHS="([0-9 ]+)"', src, re.M)
    assert m, "csrc/build.sh no longer sets WIDE_WIDTHS"
    return sorted(int(w) for w in m.group(1).split())


def test_table_lists_exactly_what_the_dispatch_allows():
    """Widths: 20 (kernels_mfma.hip) and WIDE_WIDTHS of csrc/build.sh -- a width added there without a row here fails.  Depths: L <= 6
    at H <= 32, L <= 4 beyond (init.pad_plan's rule, asked of pad_plan itself).  Channel sets: the keys of the pick_L / pick_wide_key
    tables, read from the sources; each has a full-grid row or is named in DEAD_SETS."""
    from hp_vpinns_amd import init
    widths = [init.MFMA_WIDTH] + _wide_widths_of_build_sh()
    assert widths == sorted((init.MFMA_WIDTH,) + tuple(init.WIDE_WIDTHS)) == list(sm.WIDTHS)
    allowed = set()
    for H in widths:
        for L in range(1, 9):
            plan = init.pad_plan([2] + [H - 1] * L + [1])          # (one neuron short: padded onto H while that depth is instantiated)
            if plan is not None:
                assert plan[0] == [2] + [H] * L + [1]
                allowed.add((H, L))
    assert allowed == set(sm.FULL) == {(H, L) for H in widths for L in range(1, sm.max_depth(H) + 1)}
    assert len(sm.FULL) == 30
    # channel sets of the two dispatch tables
    for fn in ("kernels_mfma.hip", "kernels_wide.hip"):
        keys = sorted(set(re.findall(r"key == (\d{3})\)", open(os.path.join(CSRC, fn)).read())))
        assert keys == sorted(sm.INSTANTIATED_SETS), (fn, keys)
    by_set = {}
    for c in sm.matrix_cases():
        by_set.setdefault(c["set"], {}).setdefault(c["row"], set()).add((c["H"], c["L"]))
    for key in sm.INSTANTIATED_SETS:
        if key in sm.DEAD_SETS:
            assert key not in by_set
            continue
        assert any(cells == set(sm.FULL) for cells in by_set[key].values()), (key, "has no row over the full (H, L) grid")
    assert by_set["221"]["p2-pinn"] == set(sm.CROSS) == {(H, L) for H, L in sm.FULL if L == 3 or H == 32}
    # the strings follow from (set, H, L) alone
    for c in sm.matrix_cases():
        fam = "mfma" if c["H"] == 20 else "wide"
        assert c["fwd"].startswith("k_fwd_%s<D=%s,NT1=%s,NT2=%s," % ((fam,) + tuple(c["set"])))
        assert c["fwd"].endswith(",L=%d,H=%d>" % (c["L"], c["H"]))
        assert c["bwd"] == c["fwd"].replace("k_fwd_", "k_bwd_")
        assert c["layers"] == [int(c["set"][0])] + [c["H"]] * c["L"] + [1]


def test_padded_cases_are_padded_onto_the_width_they_name():
    from hp_vpinns_amd import init
    for c in sm.padded_cases():
        padded, idx = init.pad_plan(c["layers"], c["n_extra"])
        assert padded == [c["layers"][0]] + [c["H"]] * c["L"] + [1], (c["name"], padded)
        assert idx.size == init.n_params(c["layers"], c["n_extra"]) < init.n_params(padded, c["n_extra"])
    kinds = {(c["layers"][0], c["kind"]) for c in sm.padded_cases()}
    assert kinds == {(1, "pinn"), (1, "var"), (2, "pinn"), (2, "var")}


def test_generic_theta_scale():
    """the default is the 0.3 every earlier caller has; another scale is that multiple of the same draw"""
    L = [2, 24, 24, 1]
    from hp_vpinns_amd.init import xavier_init
    x0 = xavier_init(L, 9, extra=[0.9])
    a, b = gp.generic_theta(L, 9, extra=[0.9]), gp.generic_theta(L, 9, extra=[0.9], scale=0.3)
    c = gp.generic_theta(L, 9, extra=[0.9], scale=0.15)
    assert np.array_equal(a, b) and a[-1] == c[-1] == 0.9
    assert np.allclose((a - x0)[:-1], 2 * (c - x0)[:-1], rtol=1e-12, atol=1e-15)
