"""tests/linop_sweep.py on the CPU (no GPU): every fixed case of the shape sweep meets its conditions at its recorded seed -- the
reference alone, with two derivations of loss and gradient within 1e-11 -- so that a drift in a reference module shows here and not as
a failure of tests/test_gpu_linop_sweep.py; and the restated LDS formula puts the guard's limit where the case table says it is."""
import pytest

import linadapt_reference as la
import linop_sweep as ls

FIXED = ls.fixed_cases()


@pytest.mark.parametrize("c", FIXED, ids=[c["name"] for c in FIXED])
def test_fixed_case_meets_its_conditions_at_its_recorded_seed(c):
    assert c["name"] in ls.SEEDS and c["seed"] == ls.SEEDS[c["name"]]
    r = ls.conditions(c)
    print(c["name"], c["seed"], r["fig"])
    assert r["ok"], (c["name"], c["seed"], r["why"])
    assert max(r["fig"]["agree"]) < ls.AGREE


def test_the_table_is_the_one_the_sweep_was_asked_for():
    names = [c["name"] for c in FIXED]
    assert len(names) == len(set(names)) == len(ls.ROWS) + 2 * len(ls.ALL_VARIANTS) + 2 * len(ls.WITH_ANSATZ) and set(names) == set(ls.SEEDS)
    sh = {c["name"]: ls.shape(c) for c in FIXED}
    nq = {k: v[1] * v[2] for k, v in sh.items()}
    nr_ = {k: v[3] * v[4] for k, v in sh.items()}
    assert nq["nq256-lin"] == 256 and 2 * sh["nq256-lin"][3] * sh["nq256-lin"][1] == 256
    assert nq["nq272-lin"] == 272 and nr_["nr272-lin"] == 272 and nq["1d-272-lin"] == 272 and sh["1d-272-lin"][0] == 1
    assert sh["nty1-lin"][4] == 1 and sh["min-lin"][1:] == (3, 3, 1, 1)
    assert sh["tall-lin"][1:3] == sh["wide-lin"][1:3][::-1] and sh["tall-lin"][3:] == sh["wide-lin"][3:][::-1]
    for v in (0, 1, 17):
        assert sum(r["data"] == v for r in ls.ROWS.values()) >= 2
    for v in (0, 3):
        assert sum(r["flux"] == v for r in ls.ROWS.values()) >= 2
    eb, ee = ls.ROWS["counts"]["shard"]
    for n, top in zip(ls.ROWS["counts"]["counts"], ls.ROWS["counts"]["nt"]):
        own = n[eb:ee]
        assert min(own) == 1 and max(own) == top and len(set(own)) == len(own)
    for c in FIXED:                               # at most 4 elements of at most 1 225 points
        assert len(c["boxes"]) <= 4 and nq[c["name"]] <= 1225


def test_lds_formula_around_the_limit():
    q, nt = ls.LDSMAX_Q, ls.LDSMAX_NT
    at = ls.lds_bytes(q, q, nt, nt)
    around = {s: ls.lds_bytes(s[0], s[1], nt, nt) for s in ls.LDS_NEIGHBOURS}
    print("ldsmax (%d,%d)/(%d,%d): %d B; neighbours %s" % (q, q, nt, nt, at, around))
    assert (q, nt, at) == (35, 17, 65064) and at <= ls.LDS_LIMIT
    assert all(v > ls.LDS_LIMIT for v in around.values())
    assert ls.ROWS["ldsmax"]["q"] == (q, q) and ls.ROWS["ldsmax"]["nt"] == (nt, nt)
    # 1-D at 272 points: 13 functions fit, 14 and 20 do not
    assert ls.NT1D == 13 and ls.lds_bytes(ls.Q1D, 1, ls.NT1D, 1) <= ls.LDS_LIMIT
    assert all(ls.lds_bytes(ls.Q1D, 1, n, 1) > ls.LDS_LIMIT for n in ls.NT1D_REFUSED)
    # the indicator kernel: the largest square rule, and the first one past it
    qi = ls.largest_indicator_rule()
    assert qi == 45 and la.lds_bytes(2, qi, qi) <= ls.LDS_LIMIT < la.lds_bytes(2, qi + 1, qi + 1)
    assert ls.lds_bytes(qi + 1, qi + 1, 1, 1) <= ls.LDS_LIMIT      # (hpv_set_tables admits it: the refusal is hpv_set_strong_form's)


def test_rotating_draws_stay_in_their_ranges():
    for seed in (1, 1792112344, 2 ** 31 - 2):
        for i in range(ls.N_ROTATING):
            c = ls.draw(seed, i)
            dim, qx, qy, ntx, nty = ls.shape(c)
            px, py = c["pad"]
            assert 3 <= qx - px <= 24 and 1 <= ntx <= qx - px - 2 and px in (0, 1, 2)
            if dim == 2:
                assert 3 <= qy - py <= 24 and 1 <= nty <= qy - py - 2 and py in (0, 1, 2)
            eb, ee = c["shard"]
            assert 1 <= ee - eb <= 4 and ee == len(c["boxes"]) <= 4 and c["data"] in (0, 1, 17) and c["flux"] in (0, 3)
            assert ls.lds_bytes(qx, qy, ntx, nty) <= ls.LDS_LIMIT
            assert ls.draw(seed, i) == c and c["name"] == "rotating%d" % i
