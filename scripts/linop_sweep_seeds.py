#!/usr/bin/env python3
"""Seed search behind tests/linop_sweep.py (CPU only): per fixed case the first of base, base + 1, .. -- at most MAX_TRIES -- at which
the reference alone meets linop_sweep.conditions (linear_reference's (a) - (c), the nonlinear and identification conditions of the
variant, two derivations within 1e-11).  Prints the SEEDS block to paste into tests/linop_sweep.py and, on stderr, every refused seed.

    python scripts/linop_sweep_seeds.py > block.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import linop_sweep as ls  # noqa: E402


def search(cases):
    chosen, failed = {}, []
    for c in cases:
        base = c["seed"]
        for k in range(ls.MAX_TRIES):
            c["seed"] = base + k
            r = ls.conditions(c)
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
    a, fa = search(ls.fixed_cases(seeds={}))
    emit("SEEDS", a)
    if fa:
        print("NO SEED within %d tries: %s" % (ls.MAX_TRIES, fa), file=sys.stderr)
        sys.exit(1)
