#!/usr/bin/env python3
"""Seed search behind tests/shape_matrix.py (CPU only): per case the first of base, base + 1000, .. -- at most MAX_TRIES -- at which the
reference alone meets shape_matrix.conditions (block floor, loss-term floor, two restatements within 1e-11 per block).  Prints the
SEEDS / PADDED_SEEDS block to paste into tests/shape_matrix.py and, on stderr, the cases that needed more than one try.

    python scripts/shape_matrix_seeds.py > block.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import shape_matrix as sm  # noqa: E402


def search(cases):
    chosen, failed = {}, []
    for c in cases:
        base = c["seed"]
        for k in range(sm.MAX_TRIES):
            c["seed"] = base + 1000 * k
            r = sm.conditions(c)
            if r["ok"]:
                break
            print("%s: seed %d refused: %s" % (c["name"], c["seed"], r["why"]), file=sys.stderr)
        else:
            failed.append(c["name"])
        chosen[c["name"]] = c["seed"]
    return chosen, failed


def emit(name, d):
    items = ['"%s": %d' % kv for kv in d.items()]
    print("%s = {" % name)
    for i in range(0, len(items), 4):
        print("    " + ", ".join(items[i:i + 4]) + ",")
    print("}")


if __name__ == "__main__":
    a, fa = search(sm.matrix_cases(seeds={}))
    b, fb = search(sm.padded_cases(seeds={}))
    emit("SEEDS", a)
    emit("PADDED_SEEDS", b)
    if fa or fb:
        print("NO SEED within %d tries: %s" % (sm.MAX_TRIES, fa + fb), file=sys.stderr)
        sys.exit(1)
