#!/usr/bin/env python3
"""Digest of the HTTP programs the compiler emits for a fixed corpus, without
a GPU -- the host-side counterpart of tools/isa_diff.py: the proof that a
change to the compiler left every program alone.

    tools/program_digest.py [-j JOBS] [--only SUBSTRING] > digest.txt
    L7M_LIB=/other/tree/cilium_amd/libl7match.so tools/program_digest.py > other.txt

One line per corpus entry: its name, the sha256 of RuleSet.program(), the word
count, info.n_dfas, info.total_dfa_states and info.n_dense_dfas -- or, for a
compile that fails, the status and the whole error text.  Every entry is
compiled twice; differing digests (uninitialised padding, an address-ordered
container) are reported on the entry's line and make the exit status 1.
Two libraries compute the same programs when their outputs are identical.
"""
import argparse
import hashlib
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from cilium_amd import l7match as L  # noqa: E402
from cilium_amd import workloads as W  # noqa: E402
import lean_job_cases  # noqa: E402
import lean_tail_cases  # noqa: E402
import lean_verify_cases  # noqa: E402
import policy_cases  # noqa: E402
import regex_ext_cases  # noqa: E402
import tile_geometry  # noqa: E402

R = L.PortRuleHTTP
RE2 = L.DIALECT_RE2_SEARCH


def corpus():
    """[(name, rules or policies thunk, compile keywords, through compile_http_policies)]"""
    out = []

    def add(name, thunk, kw=None, policies=False):
        out.append((name, thunk, kw or {}, policies))

    def sweep(name, thunk, budgets, denses, re2_budgets=()):
        for b in budgets:
            for d in denses:
                add(f"{name}/lds{b}/dense{d}", thunk, {"lds_budget_bytes": b, "dense_dfa": d})
        for b in re2_budgets:
            add(f"{name}/re2/lds{b}", thunk, {"lds_budget_bytes": b, "dialect": RE2})

    for cfg, n in ((1, None), (2, 1000), (2, 5000), (5, 20000)):
        sweep(f"config{cfg}-{n or 1}", lambda cfg=cfg, n=n: W.rules(cfg, n_rules=n), (0, 1, 16384, 65536), (0, 1, 2),
              (0, 1, 4096, 16384))
    sweep("extended+config2", lambda: list(W.EXTENDED_RULES) + W.rules(2), (0, 1), (0, 1, 2))
    for seed in range(4):
        add(f"random_policies/{seed}", lambda seed=seed: policy_cases.random_policies(seed), policies=True)
    add("golden_npds", lambda: [policy_cases.npds(policy_cases.golden_npds()["policy"])], policies=True)
    for mod in (lean_verify_cases, lean_job_cases, lean_tail_cases):
        for fam, thunk in mod.FAMILY_RULES.items():
            add(f"{mod.__name__}/{fam}", thunk)
    for kind in tile_geometry.HTTP_KINDS:
        add(f"tile_geometry/{kind}", lambda kind=kind: tile_geometry.http_rules(kind)[0],
            tile_geometry.http_rules(kind)[1])
    for seed in (1, 2):
        for backrefs in (False, True):
            add(f"regex_ext/random/seed{seed}/backrefs{int(backrefs)}",
                lambda seed=seed, backrefs=backrefs: regex_ext_cases.random_rules(np.random.default_rng(seed), 60,
                                                                                  backrefs=backrefs))
        add(f"regex_ext/dcap/seed{seed}", lambda seed=seed: regex_ext_cases.dcap_rules(np.random.default_rng(seed), 40))
        add(f"regex_ext/dcap/seed{seed}/dense2/lds1",
            lambda seed=seed: regex_ext_cases.dcap_rules(np.random.default_rng(seed), 40),
            {"dense_dfa": 2, "lds_budget_bytes": 1})

    # compiles that fail: one per message the HTTP compiler can produce from rules
    add("error/fields65", lambda: [R(Headers=[f"h{j}" for j in range(62)])])
    add("error/matchers256", lambda: [R(Headers=[f"h: v{j}" for j in range(256)])])
    add("error/regex-ecma", lambda: [R(Path="/ok"), R(Path="/a(")])
    add("error/regex-re2", lambda: [R(Path="/a(")], {"dialect": RE2})
    add("error/re2-unsupported-class", lambda: [R(Path="/\\pL+")], {"dialect": RE2})
    add("error/re2-unsupported-boundary", lambda: [R(Method="\\bGET\\b")], {"dialect": RE2})
    add("error/ecma-repeat-count", lambda: [R(Path="/a{100001}")])
    add("error/ecma-nfa-too-large", lambda: [R(Path="/(a{1000}){1000}{10}")])
    add("error/fixed-lds", lambda: [R(Headers=[f"h{j}: v{j}" for j in range(60)])])
    add("error/duplicate-matcher", lambda: [R(Headers=["a: b", "a: b"])])
    add("error/empty-header-name", lambda: [R(Headers=[": v"])])
    add("error/dfa-table-limit", lambda: [R(Path="/abc.*def")], {"max_table_bytes": 16})
    add("error/search-dfa-limit", lambda: [R(Path="(a|b)*a(a|b){20}$")], {"dialect": RE2})
    add("error/unknown-dialect", lambda: [R(Path="/a")], {"dialect": 7})
    add("error/policy-duplicate-name", lambda: policy_cases.random_policies(0)[:1] * 2, policies=True)
    return out


CORPUS = corpus()


def compile_once(i):
    _, thunk, kw, policies = CORPUS[i]
    try:
        rs = (L.RuleSet.compile_http_policies if policies else L.RuleSet.compile_http)(thunk(), **kw)
    except L.L7Error as e:
        return f"status={e.code} {str(e)!r}"
    p = rs.program()
    return (f"sha256={hashlib.sha256(p.tobytes()).hexdigest()} words={p.size} n_dfas={rs.info.n_dfas} "
            f"states={rs.info.total_dfa_states} n_dense={rs.info.n_dense_dfas}")


def digest(i):
    a, b = compile_once(i), compile_once(i)
    return CORPUS[i][0], a, a == b


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-j", "--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--only", default="", help="entries whose name contains this")
    ap.add_argument("--skip", action="append", default=[], metavar="SUBSTRING",
                    help="leave out the entries whose name contains this (config5-20000/re2 takes CPU-hours)")
    a = ap.parse_args()
    todo = [i for i, e in enumerate(CORPUS) if a.only in e[0] and not any(s in e[0] for s in a.skip)]
    bad = 0
    with multiprocessing.get_context("fork").Pool(max(1, a.jobs)) as pool:
        for name, line, same in pool.imap(digest, todo):
            bad += not same
            print(f"{name} {line}{'' if same else ' NONDETERMINISTIC'}", flush=True)
    print(f"{len(todo)} entries, {bad} nondeterministic")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
