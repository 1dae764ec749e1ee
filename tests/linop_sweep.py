"""Shape sweep of the variable-coefficient projection kernels -- k_project_lin, k_project_nl, k_project_id, k_lin_indicators and the
ansatz kernels around them -- the case table of tests/test_gpu_linop_sweep.py (a plain helper module like shape_matrix.py; no GPU
needed).  tests/test_linop_sweep_host.py proves every fixed case on the CPU.

These kernels run one 256-thread workgroup per element over RUN-TIME shapes: every loop is `for (idx = tid; idx < n; idx += 256)` over
a count made of qx, qy, ntx, nty and dim, every LDS row is padded to an odd length, and the host refuses a shape whose LDS exceeds
64 KiB.  The rows below are the smallest shapes at which each of those loops takes another number of trips (NQ = qx qy, NR = ntx nty):

  row      q                 nt        what it reaches                                                              (c) halves asked
  min      (3,3)             (1,1)     smallest Lobatto rule with an interior node, one element, one trip everywhere    q
  nty1     (4,3)             (2,1)     nty == 1 in 2-D                                                                  q
  nq256    (16,16)           (8,8)     NQ == 256 and 2 ntx qx == 256 exactly                                            q, nt
  nq272    (17,16)           (5,4)     second trip of the point loops with 16 live threads                              q, nt
  nr272    (19,18)           (17,16)   NR = 272: second trip of the residual loop, two entries of sq per thread         q, nt
  tall     (4,23)            (2,11)    qx << qy, even qx, odd qy                                                        q, nt
  wide     (23,4)            (11,2)    the transpose of tall                                                            q, nt
  counts   (17,16)           (5,4)     per-element counts with 1 and the maxima in them, on a shard of four boxes       q, nt
  padx     (18,16) pad (2,0) (5,4)     zero-weight points in x only                                                     q, nt
  pady     (16,19) pad (0,3) (5,4)     zero-weight points in y only                                                     q, nt
  ldsmax   (35,35)           (17,17)   the largest square rule hpv_set_tables admits with 17 x 17 functions (65 064 B)  q, nt
  w24      (17,16)           (5,4)     the same projection between the wide layer kernels (H = 24)                      q, nt
  1d-min   3                 1         smallest 1-D shape                                                               (1-D: none)
  1d-272   144 + 128 padded  13        NQ = 272 > 256 with qy = 1                                                       (1-D: none)

Condition (c) of linear_reference exchanges two extents in the reference's own indexing; where one of the two is 1 the exchange is
the same indexing and moves nothing, so that half is not asked for (last column).

1d-272: quadrature.GaussLobattoJacobiWeights overflows math.gamma somewhere above 170 points, hence 144 real nodes and 128 zero-weight
ones.  The kernel keeps both x tables of all functions in LDS, 2 ntx (qx | 1) doubles: at qx = 272 the 64 KiB guard admits ntx <= 13
(LDS_1D: 63 800 B) and refuses 14 and above, so the row runs with 13 functions and the GPU test asserts the refusal of 14 and 20.

Every row runs as `lin` without an ansatz; nq272, nr272, ldsmax and 1d-272 also as `nl` (all four terms) and `id` (two trainable
coefficients); nq272 and nr272 as `nl` and `id` under the `generic` ansatz as well.  Data sets of 0, 1 and 17 points and flux sets of
0 and 3 are spread over the rows, each value on at least two.

Conditions on the reference alone (`conditions`), before a device is touched: linear_reference.conditions (a) - (c) with
flux_reference.COLUMN_MOVE and generic_point.BLOCK_FLOOR as they are; nonlinear_reference.conditions for `nl`;
ident_reference.conditions for `id`; ansatz_reference.reference and .reference_autograd within AGREE = 1e-11 per block and per loss
entry (a case without an ansatz states the second derivation with the identity fields G = 0, D = 1).  A case's seed is the first of
base, base + 1, .. (at most MAX_TRIES) that keeps them: scripts/linop_sweep_seeds.py searches and prints SEEDS.

The ROTATING part: N_ROTATING further cases drawn from test_gpu_fuzz.FUZZ_SEED (`rotating_case`), a failing draw redrawn with
seed + 1000 k, k <= ROTATING_REDRAWS."""
import numpy as np

import ansatz_reference as ar
import generic_point as gp
import ident_reference as ir
import linear_reference as lr
import nonlinear_reference as nr

AGREE = 1e-11
MAX_TRIES = 40
N_ROTATING = 6
ROTATING_REDRAWS = 5
LDS_LIMIT = 64 * 1024
L1 = [1, 8, 8, 1]
KERNEL = {"lin": "k_project_lin<", "nl": "k_project_nl<", "id": "k_project_id<"}


# ---- the LDS formulas of the kernels, restated -------------------------------------------------------------------------------------------
def lds_bytes(qx, qy, ntx, nty):
    """hpv_linop_lds_bytes (csrc/kernels_linop.hip; k_project_nl and k_project_id use the same layout):
    G [3][qy][qx|1]  T [3][qy][ntx|1]  U [nty][ntx]  X [2][ntx][qx|1]  Y [2][nty][qy|1]  red [4]"""
    gs, ts, ys = qx | 1, ntx | 1, qy | 1
    return 8 * (3 * qy * gs + 3 * qy * ts + ntx * nty + 2 * ntx * gs + 2 * nty * ys + 4)


def largest_square_rule(nt):
    q = nt + 2
    while lds_bytes(q + 1, q + 1, nt, nt) <= LDS_LIMIT:
        q += 1
    return q


LDSMAX_NT = 17
LDSMAX_Q = largest_square_rule(LDSMAX_NT)                                   # 35
LDS_NEIGHBOURS = [(LDSMAX_Q + 1, LDSMAX_Q), (LDSMAX_Q, LDSMAX_Q + 1), (LDSMAX_Q + 1, LDSMAX_Q + 1)]
Q1D, PAD1D = 272, 128
NT1D = max(n for n in range(1, 21) if lds_bytes(Q1D, 1, n, 1) <= LDS_LIMIT)    # 13
NT1D_REFUSED = (NT1D + 1, 20)


def largest_indicator_rule():
    """the largest square rule hpv_set_strong_form admits (linadapt_reference.lds_bytes restates hpv_linadapt_lds_bytes)"""
    import linadapt_reference as la
    q = 3
    while la.lds_bytes(2, q + 1, q + 1) <= LDS_LIMIT:
        q += 1
    return q


# ---- the fixed rows ------------------------------------------------------------------------------------------------------------------------
B2, B1 = lr.BOXES2, lr.BOXES1
ROWS = {
    "min": dict(L=lr.S8, boxes=B2[3:], q=(3, 3), nt=(1, 1), data=0, flux=0),
    "nty1": dict(L=lr.S8, boxes=B2[:3], q=(4, 3), nt=(2, 1), data=1, flux=3),
    "nq256": dict(L=lr.S8, boxes=B2[:2], q=(16, 16), nt=(8, 8), data=17, flux=0),
    "nq272": dict(L=lr.S8, boxes=B2[:3], q=(17, 16), nt=(5, 4), data=17, flux=3),
    "nr272": dict(L=lr.S8, boxes=B2[:2], q=(19, 18), nt=(17, 16), data=1, flux=0),
    "tall": dict(L=lr.S8, boxes=B2[:3], q=(4, 23), nt=(2, 11), data=0, flux=3),
    "wide": dict(L=lr.S8, boxes=B2[:3], q=(23, 4), nt=(11, 2), data=17, flux=0),
    "counts": dict(L=lr.S8, boxes=B2, q=(17, 16), nt=(5, 4), data=1, flux=3, shard=(1, 4), counts=([5, 1, 3, 5], [4, 4, 1, 2])),
    "padx": dict(L=lr.S8, boxes=B2[:2], q=(18, 16), nt=(5, 4), data=0, flux=0, pad=(2, 0)),
    "pady": dict(L=lr.S8, boxes=B2[2:], q=(16, 19), nt=(5, 4), data=17, flux=3, pad=(0, 3)),
    "ldsmax": dict(L=lr.S8, boxes=B2[3:], q=(LDSMAX_Q, LDSMAX_Q), nt=(LDSMAX_NT, LDSMAX_NT), data=17, flux=3),
    "w24": dict(L=lr.W24, boxes=B2[:3], q=(17, 16), nt=(5, 4), data=1, flux=0),
    "1d-min": dict(L=L1, boxes=B1, q=3, nt=1, data=1, flux=0),
    "1d-272": dict(L=L1, boxes=B1[:2], q=Q1D, nt=NT1D, data=17, flux=3, pad=(PAD1D, 0)),
}
ALL_VARIANTS = ("nq272", "nr272", "ldsmax", "1d-272")      # rows that also run as nl and id, and take eight Adam steps
WITH_ANSATZ = ("nq272", "nr272")                           # ... and as nl and id under the generic ansatz

# the first seed from each case's base that keeps `conditions` (scripts/linop_sweep_seeds.py prints this block)
SEEDS = {
    "min-lin": 9901, "nty1-lin": 9951, "nq256-lin": 10001, "nq272-lin": 10051,
    "nr272-lin": 10104, "tall-lin": 10151, "wide-lin": 10201, "counts-lin": 10252,
    "padx-lin": 10301, "pady-lin": 10351, "ldsmax-lin": 10401, "w24-lin": 10451,
    "1d-min-lin": 10501, "1d-272-lin": 10551, "nq272-nl": 10603, "nq272-id": 10651,
    "nr272-nl": 10702, "nr272-id": 10751, "ldsmax-nl": 10801, "ldsmax-id": 10862,
    "1d-272-nl": 10903, "1d-272-id": 10952, "nq272-nl-ansatz": 11001, "nq272-id-ansatz": 11051,
    "nr272-nl-ansatz": 11104, "nr272-id-ansatz": 11152,
}


def _case(name, row, variant, ansatz, seed):
    kw = {k: v for k, v in row.items() if k not in ("L", "boxes", "q", "nt")}
    return lr._c(name, row["L"], row["boxes"], row["q"], row["nt"], seed, variant=variant, ansatz=ansatz, **kw)


def fixed_cases(seeds=None):
    """the fixed cases in table order; seeds: name -> seed (default SEEDS; a name it lacks starts at its base, 9901 + 50 * position)"""
    seeds = SEEDS if seeds is None else seeds
    todo = [(r, "lin", None) for r in ROWS]
    todo += [(r, v, None) for r in ALL_VARIANTS for v in ("nl", "id")]
    todo += [(r, v, "generic") for r in WITH_ANSATZ for v in ("nl", "id")]
    out = []
    for i, (r, v, a) in enumerate(todo):
        name = "%s-%s%s" % (r, v, "-ansatz" if a else "")
        out.append(_case(name, ROWS[r], v, a, seeds.get(name, 9901 + 50 * i)))
        out[-1]["row"] = r
    return out


# ---- problems, conditions --------------------------------------------------------------------------------------------------------------
def shape(c):
    """(dim, qx, qy, ntx, nty) of case dict c"""
    dim = c["L"][0]
    return (dim,) + ((c["q"] + c["nt"]) if dim == 2 else (c["q"], 1, c["nt"], 1))


def problem(c):
    return ar.problem(c, c["ansatz"])


def swaps(c):
    _, qx, qy, ntx, nty = shape(c)
    return tuple(w for w, ok in (("q", qx > 1 and qy > 1), ("nt", ntx > 1 and nty > 1)) if ok)


def _rel0(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def agreement(p):
    """(worst loss entry, worst gradient block) between ansatz_reference.reference and .reference_autograd"""
    l3a, ga, _ = ar.reference(p)
    l3b, gb = ar.reference_autograd(p if p["kind"] is not None else dict(p, kind="identity"))
    return float(_rel0(l3a, l3b).max()), float(gp.block_rel(ga, gb, p["layers"], p["c0"].size))


def conditions(c, p=None):
    """dict(ok, why, fig) of case c: the module docstring's conditions on the reference alone"""
    p = problem(c) if p is None else p
    fig = {}
    try:
        fig["lin"] = lr.conditions(p, swaps=swaps(c))
        if c["variant"] == "nl":
            fig["nl"] = nr.conditions(p, swaps=swaps(c))
        if c["variant"] == "id":
            fig["id"] = ir.conditions(p)
        fig["agree"] = agreement(p)
        assert max(fig["agree"]) < AGREE, ("the two derivations", fig["agree"])
    except AssertionError as e:
        return dict(ok=False, why=str(e)[:300], fig=fig)
    return dict(ok=True, why="", fig=fig)


# ---- the rotating part -----------------------------------------------------------------------------------------------------------------
def draw(seed, i):
    """rotating case i of `seed`: qx, qy in [3, 24], ntx in [1, qx - 2], nty in [1, qy - 2], 1 .. 4 boxes with an optional shard offset,
    variant, ansatz, counts, 0 .. 2 zero-weight points per direction, data in {0, 1, 17}, flux in {0, 3}, S8 or W24; one in three 1-D"""
    rng = np.random.RandomState((seed + 7919 * i) % (2 ** 31 - 1))
    one_d = rng.randint(3) == 0
    qx, qy = int(rng.randint(3, 25)), int(rng.randint(3, 25))
    ntx, nty = int(rng.randint(1, qx - 1)), int(rng.randint(1, qy - 1))
    px, py = int(rng.randint(3)), int(rng.randint(3))
    pool = B1 if one_d else B2
    nb = int(rng.randint(1, len(pool) + 1))
    off = int(rng.randint(0, len(pool) - nb + 1))
    boxes, shard = pool[:off + nb], (off, off + nb)
    variant = ("lin", "nl", "id")[rng.randint(3)]
    ansatz = "generic" if rng.randint(2) else None
    counts = None
    if rng.randint(2):
        counts = ([int(v) for v in rng.randint(1, ntx + 1, len(boxes))], None if one_d else [int(v) for v in rng.randint(1, nty + 1, len(boxes))])
    data, flux = int(rng.choice([0, 1, 17])), int(rng.choice([0, 3]))
    wide = bool(rng.randint(2)) and not one_d
    kw = dict(variant=variant, ansatz=ansatz, data=data, flux=flux, shard=shard)
    if counts is not None:
        kw["counts"] = counts
    if one_d:
        kw["pad"] = (px, 0)
        return lr._c("rotating%d" % i, L1, boxes, qx + px, ntx, seed % 100000 + 10 * i, **kw)
    kw["pad"] = (px, py)
    return lr._c("rotating%d" % i, lr.W24 if wide else lr.S8, boxes, (qx + px, qy + py), (ntx, nty), seed % 100000 + 10 * i, **kw)


def rotating_case(seed, i):
    """(case, problem, tries): the first of the draws seed, seed + 1000, .. + 1000 ROTATING_REDRAWS that keeps `conditions`, or
    (None, why, tries)"""
    why = []
    for k in range(ROTATING_REDRAWS + 1):
        c = draw(seed + 1000 * k, i)
        p = problem(c)
        r = conditions(c, p)
        if r["ok"]:
            return c, p, k + 1
        why.append(r["why"])
    return None, why, ROTATING_REDRAWS + 1
