#!/usr/bin/env python3
"""Per-kernel diff of the gfx950 code two source trees compile to, without a
GPU -- the proof that a refactor left the device code alone:

    tools/isa_diff.py OLD_TREE NEW_TREE [--allow REGEX ...] [-j JOBS]

Compiles every device unit of both trees to assembly with the flags of the
tree's own Makefile (l7m_kernels.hip, l7m_kafka.hip, and l7m_http_feat.hip
once per feature set F = 0..3 with L7M_FEAT_DENSE = F + 4), splits it per
function symbol (compile and parsing: tools/isa_stats.py) and compares the
functions of the same demangled name, the parameter list left out.  Ignored:
comments, the numbers of compiler-local labels (.LBB<n>_, .Lfunc_end<n>,
.Ltmp<n>, .Lpost_getpc<n>: counted per translation unit, so they move with
the order the kernels are emitted in) and the __hip_cuid_* symbol.  A function's text runs from its label
through its .amdhsa_kernel descriptor.

Prints `same` or the differing lines for every function, and the functions
only one tree has.  Exit status 1 on any difference, except differing line
pairs of which both lines match one --allow expression.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_stats import compile_asm, split_functions  # noqa: E402

CSRC = "cilium_amd/csrc"
UNITS = [("l7m_kernels", "l7m_kernels.hip", []), ("l7m_kafka", "l7m_kafka.hip", [])] + [
    (f"l7m_http_f{f}", "l7m_http_feat.hip", [f"-DL7M_FEAT={f}", f"-DL7M_FEAT_DENSE={f + 4}"]) for f in range(4)]


def makefile_flags(tree):
    """HIPFLAGS of the tree's Makefile, its variables expanded."""
    var = dict(re.findall(r"^(\w+) \??= (.*)$", open(os.path.join(tree, CSRC, "Makefile")).read(), re.M))
    flags = var["HIPFLAGS"]
    while "$(" in flags:
        flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], flags)
    return flags.split()


def normalise(line):
    line = line.split(";", 1)[0].rstrip()
    line = re.sub(r"\.(LBB|Lfunc_end|Ltmp|Lpost_getpc)\d+", r".\1", line)
    return re.sub(r"__hip_cuid_\w+", "__hip_cuid", line)


def functions(asm):
    """{demangled name without parameters: normalised lines} of one assembly file."""
    raw = split_functions(open(asm).read())
    names = subprocess.run([shutil.which("llvm-cxxfilt") or "c++filt"], input="\n".join(raw), text=True,
                           capture_output=True, check=True).stdout.splitlines()
    out = {}
    for sym, name in zip(raw, names):
        depth, cut = 0, len(name)
        for i in range(len(name) - 1, -1, -1):  # the parameter list: the last balanced (...)
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                cut = i if name[i] == "(" else len(name)
                break
        key = name[:cut]
        while key in out:  # overloads
            key += "'"
        out[key] = [l for l in map(normalise, raw[sym]) if l.strip()]
    return out


def report(unit, old, new, allow):
    """Prints the comparison of one unit's functions; the number that differ beyond `allow`."""
    bad = 0
    print(f"== {unit}: {len(old)} functions old, {len(new)} new")
    for name in old:
        if name not in new:
            bad += 1
            print(f"missing  {name}")
            continue
        if old[name] == new[name]:
            print(f"same     {name}")
            continue
        lines, ok = [], True
        sm = difflib.SequenceMatcher(None, old[name], new[name], autojunk=False)
        for tag, i1, i2, j1, j2 in sm.get_opcodes():
            if tag == "equal":
                continue
            o, n = old[name][i1:i2], new[name][j1:j2]
            paired = len(o) == len(n)
            for k in range(max(len(o), len(n))):
                lo, ln = o[k] if k < len(o) else None, n[k] if k < len(n) else None
                fine = paired and any(r.search(lo) and r.search(ln) for r in allow)
                ok &= fine
                mark = " " if fine else "!"
                if lo is not None:
                    lines.append(f"  {mark}- {lo.strip()}")
                if ln is not None:
                    lines.append(f"  {mark}+ {ln.strip()}")
        bad += not ok
        print(f"{'allowed ' if ok else 'DIFFERS '} {name}")
        print("\n".join(lines))
    for name in new:
        if name not in old:
            bad += 1
            print(f"added    {name}")
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--allow", action="append", default=[], metavar="REGEX",
                    help="a differing line pair is accepted when both lines match REGEX")
    ap.add_argument("-j", "--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    allow = [re.compile(r) for r in a.allow]
    trees = {"old": os.path.abspath(a.old_tree), "new": os.path.abspath(a.new_tree)}

    with tempfile.TemporaryDirectory() as td:
        with concurrent.futures.ThreadPoolExecutor(min(a.jobs, 16)) as pool:
            jobs = [pool.submit(compile_asm, src, os.path.join(td, f"{side}_{unit}.s"), makefile_flags(tree) + defs,
                                os.path.join(tree, CSRC))
                    for side, tree in trees.items() for unit, src, defs in UNITS]
            for j in jobs:
                j.result()
        bad = 0
        for unit, _, _ in UNITS:
            bad += report(unit, *(functions(os.path.join(td, f"{side}_{unit}.s")) for side in trees), allow)
    print(f"{bad} functions differ beyond what --allow accepts" if bad else "no difference beyond what --allow accepts")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
