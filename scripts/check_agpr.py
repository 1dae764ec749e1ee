#!/usr/bin/env python3
"""Build guard of the hand-managed AGPR stash (kernels_fused.hip, kernels_fused_gen.hip, kernels_tall.hip): those kernels park
live values in the top accumulation registers by hand, and the compiler does not know it.  The guard reads both sides from the
device assembly.  Hand-managed operands are inline-asm immediates and print in hexadecimal (`a[0x6a]`, `a[0xbe:0xbf]`): the
lowest one of a function is where ITS hand-managed range starts (none: 256, nothing to guard).  Compiler-allocated operands
print in decimal (`a91`, `a[16:23]`) and must stay below it.  A new instantiation, or a stash that moves, needs no edit here.

usage: check_agpr.py --plan kernels_fused|kernels_fused_gen|kernels_tall file.s       (csrc/build.sh, once per guarded file)
         every function of the file's kernel is checked; one report line each on stderr; stdout = the -D flags that compile the
         overlapping instantiations out (POLICY below; nothing when all are clear)
         exit codes: 0 = the flags are valid, 2 = build.sh FAILS: the check could not run (no assembly file, no function of that
                     kernel after a rename / mangling change, no function end marker), or a guarded kernel spills registers to
                     scratch memory -- either way a silently slower library would be the alternative
       check_agpr.py file.s kernel-substring base [--spills-ok]                        (one kernel against a given base)
         exit codes: 0 = clear, 1 = register overlap, 3 = no overlap, but scratch accesses (--spills-ok: report only), 2 = as above"""
import re
import sys
from collections import namedtuple

Fn = namedtuple("Fn", "name stem targs hi base spills")   # hi: highest compiler-allocated AGPR (-1: none), base: lowest hand-managed one (256: none)


class CannotRun(Exception):
    pass


def scan(src, select):
    """One pass over the assembly file `src`: an Fn for every function whose (mangled name, stem) `select` accepts, each read up to
    its .Lfunc_end -- a kernel may hold several s_endpgm (early returns)."""
    try:
        lines = open(src).read().split("\n")
    except OSError as e:
        raise CannotRun(f"cannot read {src}: {e}")
    fns, name = [], None
    for l in lines:
        if name is None:
            m = re.match(r"^(_Z(\d*)(\w+)):", l)
            if m:
                n = int(m.group(2) or 0)
                stem, rest = m.group(3)[:n], m.group(3)[n:]       # _Z<length><stem>I<template arguments>E<parameter types>
                if select(m.group(1), stem):
                    t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
                    name, targs = m.group(1), tuple(int(v) for v in re.findall(r"L[ib](\d+)E", t.group(1))) if t else ()
                    hi, base, spills = -1, 256, 0
        elif l.startswith(".Lfunc_end"):
            fns.append(Fn(name, stem, targs, hi, base, spills))
            name = None
        else:
            code = l.split(";")[0]
            if re.search(r"\bscratch_(load|store)_", code):       # scratch accesses = register spills: a hand-scheduled kernel that spills runs at a
                spills += 1                                       # fraction of its speed (420 - 540 of them once: 148 instead of 58 us per iteration)
            for m in re.finditer(r"\ba(\d+)\b|\ba\[\d+:(\d+)\]", code):
                hi = max(hi, int(m.group(1) or m.group(2)))
            for m in re.finditer(r"\ba\[0x([0-9a-f]+)(:0x[0-9a-f]+)?\]", code):
                base = min(base, int(m.group(1), 16))
    if name is not None:
        raise CannotRun(f"no function end marker behind {name} in {src}")
    return fns


def report(key, hi, base, spills):
    return (f"check_agpr: {key}: highest compiler-allocated AGPR a{hi}, hand-managed range starts at a{base}"
            + (f", {spills} SCRATCH ACCESSES (spills)" if spills else ""))


# ---- what a trip compiles out ----------------------------------------------------------------------------------------------
# Per guarded file: the kernel, its template parameters, and rows (flag, when, alone, what the build says) evaluated in order
# over the functions that tripped.  `when(a, flags)` sees one tripped function's template arguments and the flags set so far; a
# row whose flag is already set is passed over; after an `alone` row nothing else is evaluated (the kernel is gone).
FUSED = namedtuple("FUSED", "L SPLIT QT QX QY NTX NTY MULTI NT2 GEN")
TALL = namedtuple("TALL", "NT1 NT2 L QX QY NTX NTY QT")


def big(a):         # the headline shape: 20x20 points
    return (a.QX, a.QY) == (20, 20)


def tight(a):       # the tight plan (FzPlan): four channels, three hidden layers, 20x20 points
    return a.NT2 == 1 and a.L == 3 and big(a)


NO_NT2 = "-DHPV_FZ_GEN_NO_NT2"
POLICY = {
    "kernels_fused": ("k_iter_fused", FUSED, [
        ("-DHPV_AGPR_GUARD_TRIPPED", lambda a, fl: big(a) and not a.QT and not a.MULTI, True,
         "AGPR guard tripped in kernels_fused.hip: building without k_iter_fused (fallback = HPV_FUSE=b structure)"),
        ("-DHPV_AGPR_GUARD_TRIPPED_QT", lambda a, fl: big(a) and a.QT and not a.MULTI, False,
         "AGPR guard tripped in the quarter-tile instantiation of k_iter_fused: building with 7 / 6 / 6 / 6 whole tiles per wave"),
        ("-DHPV_FZ_NO_EXTRA_SHAPES", lambda a, fl: not big(a) and not a.MULTI, False,
         "AGPR guard tripped in an extra element shape of k_iter_fused: those shapes run on the other structures"),
        ("-DHPV_FZ_NO_MULTI", lambda a, fl: a.MULTI, False,
         "AGPR guard tripped in an element-loop instantiation of k_iter_fused: grids larger than the chip keep one workgroup per element"),
    ]),
    # the general variational forms: a trip compiles out, in this order of preference, the quarter-tile instantiations, the
    # four-channel ones (the tight plan is one of them, with a flag of its own), everything
    "kernels_fused_gen": ("k_iter_fused", FUSED, [
        ("-DHPV_FZ_GEN_TRIPPED", lambda a, fl: a.NT2 == 0 and not a.QT, True,
         "AGPR guard tripped in the general forms of k_iter_fused: those forms run on the separate launches"),
        (NO_NT2, lambda a, fl: a.NT2 == 1 and not a.QT and not tight(a), False,
         "AGPR guard tripped in a four-channel instantiation of k_iter_fused: those forms run on the separate launches"),
        ("-DHPV_FZ_GEN_NO_QT", lambda a, fl: a.QT and not (a.NT2 == 1 and NO_NT2 in fl), False,
         "AGPR guard tripped in a quarter-tile instantiation of the general forms: whole tiles only"),
        ("-DHPV_FZ_GEN_NO_TIGHT", lambda a, fl: NO_NT2 in fl, False,
         "without the four-channel instantiations of k_iter_fused the tight plan goes too"),
        ("-DHPV_FZ_GEN_NO_TIGHT", lambda a, fl: tight(a), False,
         "AGPR guard tripped in the tight-plan instantiation of k_iter_fused: four channels on 20x20 points with three hidden layers run on the separate launches"),
    ]),
    "kernels_tall": ("k_iter_tall", TALL, [
        ("-DHPV_AGPR_GUARD_TRIPPED", lambda a, fl: not a.QT, True,
         "AGPR guard tripped in kernels_tall.hip: building without k_iter_tall (fallback = the separate launches)"),
        ("-DHPV_AGPR_GUARD_TRIPPED_QT", lambda a, fl: a.QT, False,
         "AGPR guard tripped in the quarter-tile instantiations of k_iter_tall: building with whole tiles only"),
    ]),
}


def plan(unit, src):
    """The -D flags `unit` must be compiled with, given its assembly `src`; report and warnings on stderr."""
    kernel, params, rows = POLICY[unit]
    fns = scan(src, lambda name, stem: stem == kernel)
    if not fns:
        raise CannotRun(f"no {kernel} function in {src} (renamed?)")
    tripped = []
    for f in fns:
        print(report(f.name, f.hi, f.base, f.spills), file=sys.stderr)
        if len(f.targs) != len(params._fields):
            raise CannotRun(f"{f.name} does not carry the template arguments <{', '.join(params._fields)}> (template arguments changed?)")
        if f.spills:
            raise CannotRun(f"{f.name} spills registers to scratch memory ({f.spills} accesses): a hand-scheduled kernel must not")
        if f.hi >= f.base:
            print(f"check_agpr: FAILED -- the compiler uses a{f.hi}, which overlaps the hand-managed AGPR stash of {f.name}", file=sys.stderr)
            tripped.append(params(*f.targs))
    flags = []
    for flag, when, alone, text in rows:
        if flag not in flags and any(when(a, flags) for a in tripped):
            print(f"build.sh: WARNING -- {text}", file=sys.stderr)
            flags.append(flag)
            if alone:
                break
    return flags


def main(argv):
    try:
        if argv[1] == "--plan":
            print(" ".join(plan(argv[2], argv[3])))
            return 0
        src, key, base = argv[1], argv[2], int(argv[3])
        fns = scan(src, lambda name, stem: key in name)
        if not fns:
            raise CannotRun(f"kernel {key} not found in {src} (renamed? template arguments changed?)")
    except CannotRun as e:
        print(f"check_agpr: ERROR -- {e}", file=sys.stderr)
        return 2
    hi, spills = max(f.hi for f in fns), sum(f.spills for f in fns)
    print(report(key, hi, base, spills))
    if spills:
        print(f"check_agpr: WARNING -- {key} spills registers to scratch memory ({spills} accesses): expect a large slow-down", file=sys.stderr)
        if "--spills-ok" not in argv:
            return 3
    if hi >= base:
        print(f"check_agpr: FAILED -- the compiler uses a{hi}, which overlaps the hand-managed AGPR stash of {key}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
