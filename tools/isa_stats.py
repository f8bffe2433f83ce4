#!/usr/bin/env python3
"""Static ISA summary of the kernels in one .hip file (gfx950), for A/B work
on code generation without a GPU:

    tools/isa_stats.py cilium_amd/csrc/l7m_kafka.hip [-DFLAG ...] [-k substr]

Prints per kernel: VGPR / SGPR / LDS / scratch from the code object metadata
and instruction counts by class (VALU, SALU, DS, global, branches, waitcnt),
the code bytes, the scalar loads (all, and those in basic blocks the compiler
marks as part of a loop), and the SGPR spill traffic to VGPR lanes
(v_writelane / v_readlane).
The compile and the assembly parsing are shared with tools/isa_diff.py.
"""
import argparse
import os
import re
import subprocess
import tempfile

HIPCC = "/opt/rocm/bin/hipcc"
BASE_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics"]


def compile_asm(src, out, flags=BASE_FLAGS, cwd=None):
    """Device-side assembly of one .hip file."""
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True, cwd=cwd)


def split_functions(text):
    """{symbol: the lines from its label to the end of its body}, in file order."""
    funcs, cur = {}, None
    is_func = set(re.findall(r"^\t\.type\t(\S+),@function", text, re.M))  # (not the data symbols)
    for line in text.splitlines():
        m = re.match(r"^(_Z\S+):\s*(;.*)?$", line)
        if m and m.group(1) in is_func:
            cur = funcs[m.group(1)] = []
            continue
        if cur is not None and (line.startswith(".Lfunc_end") or line.startswith("\t.end_amdhsa_kernel")):
            cur = None
        if cur is not None:
            cur.append(line)
    return funcs


def kernel_descriptors(text):
    """{kernel symbol: the lines of its .amdhsa_kernel block}."""
    return {m.group(1): m.group(2).strip("\n").splitlines()
            for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}


def code_bytes(text):
    """{symbol: codeLenInByte of the compiler's per-function summary}."""
    return {m.group(1): int(m.group(2))
            for m in re.finditer(r"^\t\.size\t(\S+), \.Lfunc_end\d+-\S+\n(?:.*\n)*?; codeLenInByte = (\d+)", text, re.M)}


def loop_counts(lines):
    """(scalar loads, scalar loads in loop blocks, v_writelane, v_readlane) of one function."""
    in_loop, at_label, n = False, False, dict(sload=0, sload_loop=0, wlane=0, rlane=0)
    for l in lines:
        if re.match(r"^\.LBB\d+_\d+:", l):
            in_loop, at_label = "in Loop" in l or "Loop Header" in l, True
            continue
        if at_label and l.lstrip().startswith(";"):  # a named block carries the loop note on the comment lines below its label
            in_loop |= "in Loop" in l or "Loop Header" in l
            continue
        at_label = False
        op = l.split()[0] if l.startswith("\t") and l.split() else ""
        if op.startswith("s_load_") or op.startswith("s_buffer_load_"):
            n["sload"] += 1
            n["sload_loop"] += in_loop
        elif op.startswith("v_writelane"):
            n["wlane"] += 1
        elif op.startswith("v_readlane"):
            n["rlane"] += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("-k", "--kernel", default="", help="substring of the kernel symbol")
    ap.add_argument("--asm", action="store_true", help="src is assembly already compiled (compile_asm's output)")
    ap.add_argument("flags", nargs="*")
    a, extra = ap.parse_known_args()

    if a.asm:
        text = open(a.src).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            asm = os.path.join(td, "k.s")
            compile_asm(a.src, asm, BASE_FLAGS + a.flags + extra)
            text = open(asm).read()

    size = code_bytes(text)
    meta = {}
    for name, lines in kernel_descriptors(text).items():
        body = "\n".join(lines)
        g = lambda k: (re.search(r"\.%s (\d+)" % k, body) or [None, "?"])[1]
        meta[name] = (g("amdhsa_next_free_vgpr"), g("amdhsa_next_free_sgpr"),
                      g("amdhsa_group_segment_fixed_size"), g("amdhsa_private_segment_fixed_size"))

    for name, lines in split_functions(text).items():
        if a.kernel not in name or name not in meta:
            continue
        ins = [l.strip() for l in lines if l.startswith("\t") and not l.startswith("\t.")]
        c = dict(valu=0, salu=0, ds=0, glob=0, br=0, wait=0)
        for i in ins:
            op = i.split()[0] if i else ""
            if op.startswith("v_"):
                c["valu"] += 1
            elif op.startswith("s_waitcnt"):
                c["wait"] += 1
            elif op.startswith("s_cbranch") or op.startswith("s_branch"):
                c["br"] += 1
            elif op.startswith("s_"):
                c["salu"] += 1
            elif op.startswith("ds_"):
                c["ds"] += 1
            elif op.startswith(("global_", "buffer_", "flat_")):
                c["glob"] += 1
        v, s, l, p = meta[name]
        c.update(loop_counts(lines))
        print(f"{name[:90]}\n   vgpr {v} sgpr {s} lds {l} scratch {p} code_bytes {size.get(name, '?')} | lines {len(ins)} " +
              " ".join(f"{k} {n}" for k, n in c.items()))


if __name__ == "__main__":
    main()
