"""Writes rule_advice_parent.npz: which quadrature rule / test-function count the three problem classes handed to the device BEFORE
hpv_rule_advice learned the variational form and the network (the commit in front of "one rule advice").

Until then the decision was spread over hpv_rule_advice(device, dim, q, ntx, nty, n_elem_shard, exact_counts, n_hidden, ..) and the
classes of hp_vpinns_amd/vpinn.py, which gated the call on width / depth / form and rejected some of its answers.  This script
restates that Python half line by line and evaluates it with a library built FROM THAT COMMIT (old signature):

    python tests/golden/make_rule_advice_table.py /path/to/parent/hp_vpinns_amd/libhpvpinn.so

device = -1 everywhere: no device is queried, the library assumes 256 compute units (and so did vpinn._n_cus without a device).
tests/test_host_numerics.py asserts that today's single call answers every row of the table alike."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

POISSON1D, POISSON2D, ADVDIFF = 0, 1, 2
N_CUS = 256

Q2D = range(4, 23)
COUNTS_2D = lambda q: sorted({(max(q // 2, 1),) * 2, (5, 5), (4, 5), (9, 3), (11, 3), (10, 10)})
SHARDS_2D = (1, 64, 255, 256, 257, 289, 400, 480, 512, 552, 768, 1023, 1024, 1025, 1280, 1281, 1296, 1536, 1537, 1600, 2048, 4096, 10000)
SHARDS_2D_THIN = (64, 256, 1024, 1280, 1281, 10000)          # networks the classes never asked the library about: these shards,
COUNTS_2D_THIN = lambda q: sorted({(max(q // 2, 1),) * 2, (5, 5), (9, 3)})      # these count pairs
FORMS_2D = ((POISSON2D, 0), (POISSON2D, 1), (POISSON2D, 2), (ADVDIFF, 0), (ADVDIFF, 1))
Q1D = (10, 40, 55, 56, 60, 79, 80, 81, 90)
COUNTS_1D = (5, 20, 30, 60, 61)
SHARDS_1D = (4, 16, 256, 257, 512, 513, 10000)


def parent_advice(lib):
    lib.hpv_rule_advice.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def advice(dim, q, ntx, nty, ne, exact_counts=False, n_hidden=0):
        qd, nd = C.c_int(0), C.c_int(0)
        rc = lib.hpv_rule_advice(-1, dim, q, ntx, nty, ne, 1 if exact_counts else 0, n_hidden, C.byref(qd), C.byref(nd))
        assert rc == 0, (rc, dim, q, ntx, nty, ne)
        return qd.value, nd.value
    return advice


def parent_decision(advice, pde, var_form, n_hidden, width, q, ntx, nty, ne):
    """(q_dev, nt_dev) as VPINN1D / VPINN2D / VPINNAdvDiff (backend "auto", no HPV_*_RULE_PADDING switch) chose them."""
    def device_rule_2d(exact_counts=False, only=None, n_hidden=0, reject=()):        # vpinn._device_rule_2d
        q_dev, _ = advice(2, q, ntx, nty, ne, exact_counts, n_hidden)
        return q_dev if (q_dev > q and (only is None or q_dev == only) and q_dev not in reject) else q

    if pde == POISSON1D:
        tile_ok = var_form in (1, 2) and width <= 20 and 2 <= n_hidden <= 4 and q <= 80 and ntx <= 60
        if not tile_ok:
            return q, ntx
        q_dev, nt_dev = advice(1, q, ntx, 1, ne)
        pad_rule = q_dev > q
        return (80 if pad_rule else q), (nt_dev if (pad_rule or q == 80) else ntx)
    if pde == POISSON2D:
        if var_form in (0, 1) and width <= 20 and 2 <= n_hidden <= 3:
            rej = () if var_form == 1 else ((10, 20) if (n_hidden == 3 and ne > 5 * N_CUS) else (10,))
            return device_rule_2d(n_hidden=n_hidden, reject=rej), ntx
        return q, ntx
    if width <= 20 and 2 <= n_hidden <= 3 and q < 10:
        return device_rule_2d(exact_counts=True, only=10), ntx
    if width <= 20 and 2 <= n_hidden <= 3 and 10 < q < 20:
        rej = (10,) if (var_form == 1 or n_hidden == 2 or ne <= 5 * N_CUS) else (10, 20)
        return device_rule_2d(n_hidden=n_hidden, reject=rej), ntx
    return q, ntx


def sweep():
    """Rows (pde, var_form, n_hidden, width, q, ntx, nty, n_elem_shard): the full cross product for the networks the classes consult
    the library about (20-wide, two / three hidden layers; 1-D: one to five), a thinner one for the others."""
    for (pde, vf), nh, width in itertools.product(FORMS_2D, range(1, 6), (5, 20, 24)):
        shards, counts = (SHARDS_2D, COUNTS_2D) if (width == 20 and nh in (2, 3)) else (SHARDS_2D_THIN, COUNTS_2D_THIN)
        for q in Q2D:
            for (ntx, nty), ne in itertools.product(counts(q), shards):
                yield pde, vf, nh, width, q, ntx, nty, ne
    for vf, nh, width in itertools.product((1, 2, 3), range(1, 6), (5, 20, 24)):
        if width != 20 and nh not in (2, 5):
            continue
        for q, nt, ne in itertools.product(Q1D, COUNTS_1D, SHARDS_1D):
            yield POISSON1D, vf, nh, width, q, nt, 1, ne


def main():
    advice = parent_advice(C.CDLL(sys.argv[1]))
    rows = np.array(list(sweep()), dtype=np.int32)
    out = np.array([parent_decision(advice, *(int(v) for v in r)) for r in rows], dtype=np.int32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rule_advice_parent.npz")
    np.savez_compressed(path, rows=rows, q_dev=out[:, 0], nt_dev=out[:, 1])
    print("%s: %d rows, %d padded, %d bytes" % (path, rows.shape[0], int(np.sum(out[:, 0] != rows[:, 4])), os.path.getsize(path)))


if __name__ == "__main__":
    main()
