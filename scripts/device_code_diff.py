#!/usr/bin/env python3
"""Is the device code of two builds of the product library the same?  (The check behind a refactor that must not touch a kernel.)

    device_code_diff.py emit <tree> <out dir> [jobs]     every product object of <tree>/hp_vpinns_amd/csrc/build.sh compiled with
                                                          -save-temps=obj in a directory of its own; its gfx950 assembly -> <out dir>/<unit>.s
    device_code_diff.py compare <dir A> <dir B>          function by function: instruction stream and kernel descriptor

Normalised before comparing: comments, basic-block label numbers, and mangled names (demangled; a function of A matches the
function of B with the same template arguments, or with ONE argument position removed -- a retired template parameter).  Two
functions that differ only in the offset immediates of scalar loads (a kernel-argument struct that lost a field) are reported as
such, not as identical.  Exit status 1 when anything else differs or a function has no partner.
"""
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

CXXFILT = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"


def units(csrc):
    """(unit name, source, extra flags) of every product object, read from build.sh itself"""
    sh = open(os.path.join(csrc, "build.sh")).read()
    var = lambda n: re.search(rf'^{n}="([^"]*)"', sh, re.M).group(1)
    flags = var("FLAGS").replace("$HPV_EXTRA_FLAGS", "").split()
    out = [(f, f + ".hip", []) for f in var("SRCS").split()]
    for w in var("WIDE_WIDTHS").split():
        for d in (1, 2):
            out.append((f"kernels_wide_{w}_d{d}", "kernels_wide.hip", [f"-DHPV_WIDE_H={w}", f"-DHPV_WIDE_D={d}"]))
    for shp in var("ELEM_SHAPES").split():
        qx, qy, ntx, nty = shp.split(",")
        out.append((f"kernels_elem_{qx}_{qy}_{ntx}_{nty}", "kernels_elem.hip",
                    [f"-DHPV_ELEM_QX={qx}", f"-DHPV_ELEM_QY={qy}", f"-DHPV_ELEM_NTX={ntx}", f"-DHPV_ELEM_NTY={nty}"]))
    return flags, out


def emit(tree, out, jobs):
    csrc = os.path.join(tree, "hp_vpinns_amd", "csrc")
    flags, us = units(csrc)
    os.makedirs(out, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def one(u):
        name, src, extra = u
        tmp = os.path.join(out, ".tmp_" + name)
        os.makedirs(tmp, exist_ok=True)
        subprocess.run([hipcc] + flags + extra + ["-save-temps=obj", "-c", src, "-o", os.path.join(tmp, name + ".o")],
                       cwd=csrc, check=True, stderr=subprocess.DEVNULL)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        shutil.copy(os.path.join(tmp, asm[0]), os.path.join(out, name + ".s"))
        shutil.rmtree(tmp)
        return name

    with ThreadPoolExecutor(jobs) as ex:
        for name in ex.map(one, us):
            print("emitted", name, flush=True)


def demangle(names):
    p = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, p.stdout.split("\n")))


def split_args(dem):
    """'k<a, b<c, d>, e>(T)' -> ('k', ['a', 'b<c, d>', 'e'])"""
    i = dem.find("<")
    par = dem.find("(")
    if i < 0 or (0 <= par < i):
        return dem.split("(")[0], []
    depth, args, cur = 0, [], ""
    for ch in dem[i:]:
        if ch == "<":
            depth += 1
            if depth == 1:
                continue
        elif ch == ">":
            depth -= 1
            if depth == 0:
                args.append(cur.strip())
                break
        elif ch == "," and depth == 1:
            args.append(cur.strip())
            cur = ""
            continue
        cur += ch
    base = dem[:i]
    return base.split()[-1], args       # ('void k' -> 'k')


def functions(path):
    """name -> (instruction lines, descriptor lines) of every function of a device assembly file"""
    fns, desc = {}, {}
    name, body, kd = None, [], None
    for raw in open(path, errors="replace"):
        line = raw.split(";")[0].rstrip()
        if not line.strip():
            continue
        s = line.strip()
        m = re.match(r"\.type\s+(\S+),@function", s)
        if m:
            name, body = m.group(1), []
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            kd = m.group(1)
            desc[kd] = []
            continue
        if s == ".end_amdhsa_kernel":
            kd = None
            continue
        if kd is not None:
            desc[kd].append(" ".join(s.split()))
            continue
        if name is not None:
            if s.startswith(".Lfunc_end"):
                fns[name] = body
                name = None
            elif not s.startswith((".p2align", ".globl", ".protected", ".weak", ".hidden", ".section", ".text")) and s != name + ":":
                body.append(" ".join(s.split()))
    return {n: (b, desc.get(n, [])) for n, b in fns.items()}


def normalise(lines, dem):
    out = []
    for s in lines:
        s = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s)
        s = re.sub(r"\.L(tmp|func_begin|func_end)\d+", r".L\1", s)
        s = re.sub(r"_Z\w+", lambda m: "<" + split_args(dem.get(m.group(0), m.group(0)))[0] + ">", s)
        out.append(s)
    return out


SLOAD = re.compile(r"^(s_load_dword\w*\s+\S+,\s*\S+,\s*)(0x[0-9a-f]+|\d+)(.*)$")


def only_load_offsets(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x == y:
            continue
        mx, my = SLOAD.match(x), SLOAD.match(y)
        if not (mx and my and mx.group(1) == my.group(1) and mx.group(3) == my.group(3)):
            return False
    return True


def compare(da, db):
    fa, fb = {}, {}
    for d, f in ((da, fa), (db, fb)):
        for fn in sorted(os.listdir(d)):
            if fn.endswith(".s"):
                for n, v in functions(os.path.join(d, fn)).items():
                    f[(fn, n)] = v
    dem = demangle(sorted({n for _, n in list(fa) + list(fb)}))
    keyed_b = {}
    for (fn, n) in fb:
        base, args = split_args(dem[n])
        keyed_b.setdefault((fn, base), []).append((args, n))
    # a retired template parameter sits at ONE position for all instantiations of a kernel in a file: the position whose removal maps
    # the argument lists of A one to one onto those of B
    drop = {}
    for key in {(fn, split_args(dem[n])[0]) for fn, n in fa}:
        la = [split_args(dem[n])[1] for fn, n in fa if (fn, split_args(dem[n])[0]) == key]
        lb = sorted(a for a, _ in keyed_b.get(key, []))
        if la and lb and len(la[0]) == len(lb[0]) + 1:
            pos = [i for i in range(len(la[0])) if sorted(a[:i] + a[i + 1:] for a in la) == lb]
            if pos:
                drop[key] = pos[0]
    used, same, offs, diff, lone = set(), 0, [], [], []
    n_kernels = 0
    for (fn, n), (body, desc) in sorted(fa.items()):
        base, args = split_args(dem[n])
        if (fn, base) in drop:
            args = args[:drop[(fn, base)]] + args[drop[(fn, base)] + 1:]
        hit = [m for a, m in keyed_b.get((fn, base), []) if a == args and (fn, m) not in used]
        if len(hit) != 1:
            lone.append(f"{fn}: {dem[n]}  (A only, {len(hit)} candidates)")
            continue
        used.add((fn, hit[0]))
        n_kernels += bool(desc)
        body_b, desc_b = fb[(fn, hit[0])]
        na, nb = normalise(body, dem), normalise(body_b, dem)
        if na == nb and desc == desc_b:
            same += 1
        elif desc == desc_b and only_load_offsets(na, nb):
            offs.append(f"{fn}: {dem[n]}  ({sum(x != y for x, y in zip(na, nb))} scalar-load offsets)")
        else:
            what = []
            if desc != desc_b:
                what.append("descriptor: " + "; ".join(f"{x} -> {y}" for x, y in zip(desc, desc_b) if x != y))
            if na != nb:
                what.append(f"instructions: {len(na)} -> {len(nb)} lines")
            diff.append(f"{fn}: {dem[n]}  ({', '.join(what)})")
    for (fn, n) in sorted(fb):
        if (fn, n) not in used:
            lone.append(f"{fn}: {dem[n]}  (B only)")
    print(f"functions compared: {len(used)} (of them kernels: {n_kernels})")
    print(f"identical: {same}")
    print(f"differing only in scalar-load offsets: {len(offs)}")
    for s in offs:
        print("   ", s)
    print(f"differing otherwise: {len(diff)}")
    for s in diff:
        print("   ", s)
    print(f"without a partner: {len(lone)}")
    for s in lone:
        print("   ", s)
    return 1 if diff or lone else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "emit":
        emit(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 8)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
