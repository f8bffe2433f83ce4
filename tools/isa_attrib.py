#!/usr/bin/env python3
"""Static attribution of one kernel's instructions to source ranges (gfx950),
without a GPU: where the VALU / SALU / LDS / VMEM / branch / wait instructions
of a kernel come from in the source.

    tools/isa_attrib.py [--asm FILE] [-k SUBSTR] [--weights FILE] [--lines]

Without --asm it compiles cilium_amd/csrc/l7m_http_feat.hip, feature set 0,
with the Makefile's flags plus -gline-tables-only -S --offload-device-only
(line tables do not change the code: the totals equal tools/isa_stats.py's).
-k picks the kernel by a substring of its symbol (default: the lean
http_eval_kernel<1, 4, 0, 8>).  Every instruction is booked on the source line
of its innermost inlined frame (the assembly's .loc directives), and lines are
grouped by the RANGES table below; instructions the compiler made without a
line (.loc line 0: mask and copy traffic, spills) get a bucket of their own.

--weights FILE: JSON {range name: executions per tile}; prints the weighted
sums next to the static ones (an estimate: a range counts as straight-line
code executed that many times).  --lines lists the per-line counts too.
"""
import argparse
import collections
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_diff import CSRC, makefile_flags  # noqa: E402
from isa_stats import compile_asm, split_functions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_KERNEL = "http_eval_kernelILi1ELi4ELi0ELi8EE"

# Source ranges of l7m_http_impl.h: (name, text that the range's first line
# contains).  A range runs to the line before the next one's start (in file
# order); the anchors are looked up in the file, so the table survives edits.
# Lines of other files are booked under the file's name.
RANGES = [
    ("loads and end_code", "__device__ __forceinline__ uint32_t gld(const uint32_t* p)"),
    ("walk_hbm / dense (generic)", "#define L7M_WALK_BYTES(STEP, DEAD)"),
    ("LdsChain step and init", "typedef __attribute__((address_space(3))) const uint32_t* lds_cptr;"),
    ("LdsChain::run", "__device__ __forceinline__ void run(const Src& src, uint32_t pos, uint32_t len, uint32_t k)"),
    ("LdsChain end code", "__device__ __forceinline__ uint32_t code_in_entry("),
    ("set_has and Codes", "__device__ __forceinline__ bool set_has("),
    ("search / alit walks (generic)", "struct Ctx {"),
    ("name_field_of", "__device__ __forceinline__ uint32_t name_field_of("),
    ("code_has", "// Does end code `code` of DFA d contain pattern p?"),
    ("ent_lookup, dcap, WalkOut", "// (policy, direction, port) -> entry | kEntHaveHttp"),
    ("lean: per-wave constants (LeanHeader, jobs 0-2)", "// What one walk of the lean kernel needs of its automaton"),
    ("lean: one walk (chain start, end code, set, candidate)", "// One walk of the lean kernel:"),
    ("tile_header, field_at", "// The header the tile loop reads: the program's, or the lean kernel's copy."),
    ("walk: validation and directory scan", "__device__ __forceinline__ int32_t eval_walk("),
    ("walk: job set-up and selection", "  HPROF(1);"),
    ("walk: lean jobs 0-2", "    // Jobs 0-2 outside the loop:"),
    ("walk: job selection (cursor, header names)", "  for (uint32_t job = kLean ? 3 : 0;; ++job) {"),
    ("walk: lean job body (descriptors, set, touch)", "    HPROF(2);  // job selection, header-name lookup"),
    ("walk: generic job body", "    } else if (f != kNone) {"),
    ("walk: hand-over", "  HPROF(5);"),
    ("verification", "// Verification phase: the first rule (smallest index) among the keyed"),
    ("tile: set-up, plan, issue", "// Per-rule hit counters: none, per-workgroup LDS counters"),
    ("tile: loop top and walk call", "  while (t.cur < end) {"),
    ("tile: plan and issue of the next tile", "    const Tile t2 = plan(t.cur + t.take, o2, n2);"),
    ("tile: verify call and verdict store", "    qtn(3);"),
    ("tile: counters", "    if (kHits != kNoHits) {"),
    ("tile: loop end, flush, signal", "    wave_sync();  // the stage is overwritten by the next tile"),
    ("slow pass and launchers", "// Second pass over the requests the first pass deferred"),
]
IMPL = "l7m_http_impl.h"
CLASSES = ("valu", "salu", "lds", "vmem", "br", "wait")


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_cbranch") or op.startswith("s_branch"):
        return "br"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    return None


def resolve_ranges(path):
    """[(first line, name)] sorted by line, from the anchors of RANGES."""
    lines = open(path).read().splitlines()
    out = []
    for name, anchor in RANGES:
        at = [i + 1 for i, l in enumerate(lines) if l.rstrip() == anchor.rstrip()] or \
             [i + 1 for i, l in enumerate(lines) if anchor in l]  # a whole line, else a part of one
        if not at:  # (an older tree: the range does not exist there)
            print(f"isa_attrib: no range '{name}' in {path}", file=sys.stderr)
            continue
        out.append((at[0], name))
    if sorted(out) != out:
        raise SystemExit("isa_attrib: RANGES is not in file order")
    return out


def file_table(text):
    """{file number: base name} of the assembly's .file directives."""
    files = {}
    for m in re.finditer(r'^\t\.file\t(\d+) (?:"([^"]*)" )?"([^"]*)"', text, re.M):
        files[int(m.group(1))] = os.path.basename(m.group(3))
    return files


def attribute(lines, files, ranges):
    """{bucket: Counter(class)}, {(file, line): Counter(class)} of one function's lines."""
    starts = [s for s, _ in ranges]
    buckets = collections.OrderedDict()
    per_line = collections.defaultdict(collections.Counter)
    cur = ("?", 0)
    for l in lines:
        m = re.match(r"^\t\.loc\t(\d+) (\d+)", l)
        if m:
            cur = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        if not l.startswith("\t") or l.startswith("\t."):
            continue
        op = l.split()[0]
        cls = classify(op)
        if cls is None:
            continue
        fname, line = cur
        if line == 0:
            b = "(no line: compiler-made)"
        elif fname == IMPL:
            k = -1
            for i, s in enumerate(starts):
                if s <= line:
                    k = i
            b = ranges[k][1] if k >= 0 else f"{IMPL} (head)"
        else:
            b = f"other: {fname}"
        buckets.setdefault(b, collections.Counter())[cls] += 1
        per_line[(fname, line)][cls] += 1
    return buckets, per_line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="assembly already compiled with -gline-tables-only -S --offload-device-only")
    ap.add_argument("--tree", default=ROOT, help="source tree (default: this one)")
    ap.add_argument("-k", "--kernel", default=DEFAULT_KERNEL, help="substring of the kernel symbol")
    ap.add_argument("--weights", help="JSON {range name: executions per tile}")
    ap.add_argument("--lines", action="store_true", help="also list the counts per source line")
    a = ap.parse_args()

    csrc = os.path.join(os.path.abspath(a.tree), CSRC)
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            asm = os.path.join(td, "k.s")
            flags = [f for f in makefile_flags(os.path.abspath(a.tree)) if f not in ("-fPIC", "-pthread")]
            compile_asm("l7m_http_feat.hip", asm, flags + ["-gline-tables-only", "-DL7M_FEAT=0", "-DL7M_FEAT_DENSE=4"],
                        csrc)
            text = open(asm).read()
    ranges = resolve_ranges(os.path.join(csrc, IMPL))
    files = file_table(text)
    weights = json.load(open(a.weights)) if a.weights else None

    found = False
    for name, lines in split_functions(text).items():
        if a.kernel not in name:
            continue
        found = True
        buckets, per_line = attribute(lines, files, ranges)
        order = [n for _, n in ranges if n in buckets] + [b for b in buckets if b not in dict((n, 0) for _, n in ranges)]
        print(name[:100])
        hdr = f"{'range':<56}" + "".join(f"{c:>7}" for c in CLASSES)
        if weights:
            hdr += f"{'x/tile':>8}{'w.valu':>8}{'w.salu':>8}{'w.lds':>7}"
        print(hdr)
        tot, wtot = collections.Counter(), collections.Counter()
        for b in order:
            c = buckets[b]
            tot.update(c)
            row = f"{b:<56}" + "".join(f"{c[k]:>7}" for k in CLASSES)
            if weights:
                w = float(weights.get(b, 0))
                for k in ("valu", "salu", "lds"):
                    wtot[k] += w * c[k]
                row += f"{w:>8.2f}{w * c['valu']:>8.0f}{w * c['salu']:>8.0f}{w * c['lds']:>7.0f}"
            print(row)
        row = f"{'total':<56}" + "".join(f"{tot[k]:>7}" for k in CLASSES)
        if weights:
            row += f"{'':>8}{wtot['valu']:>8.0f}{wtot['salu']:>8.0f}{wtot['lds']:>7.0f}"
        print(row)
        if a.lines:
            print("per line (file:line valu salu lds vmem br wait)")
            for (f, ln), c in sorted(per_line.items()):
                print(f"  {f}:{ln} " + " ".join(str(c[k]) for k in CLASSES))
    if not found:
        raise SystemExit(f"isa_attrib: no kernel matching {a.kernel!r}")


if __name__ == "__main__":
    main()
