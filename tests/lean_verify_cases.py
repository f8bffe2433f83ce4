"""Records and rule sets for three parts of the lean HTTP kernel
(l7m_http_impl.h): the verdict stores held over the tile loop's edge, the
header jobs of the job loop (a lean program has one header field with an
automaton at the most), and the inline matchers decided from the candidate
entry's pad words (program.h CandEntry::pad, kHttpInlineMasks); needs no GPU.
tests/test_http_lean_verify_gpu.py evaluates them on the device,
tests/test_lean_verify_cases.py checks the conditions below on the CPU.

Every family has its own rule set; one shared, shuffled batch holds the records
of all of them and every rule set is evaluated on the whole batch.

  nohdr      no header automaton at all (three value automata), presence headers
  among      the header automaton's field among presence-only header fields, in
             front of and behind them in the record; the owning header repeated
             (first occurrence wins) and absent
  vlen       header values of 0-9 bytes at the four start alignments
  sets1/31/32/33  rules keyed on the path with an inline matcher on the method
             automaton, which has that many sets (33: the flag is off, the lean
             kernel takes its mask-table rounds)
  codes      a set code against a latched code against code 0 on one inline
             matcher; two rules that differ in one mask bit only (the same
             path key class, method sets {a.*} and {a.*, ab.*})
  inline     entries with 1-4 inline matchers and with 5 (scanned: no pad), a
             list of two rules on one path key, a matcher on an absent field

A header value is matched exactly, so the library compiles no header automaton
that is dead from its start; the nearest case is in `among`: values whose
first byte already leaves the automaton.

Conditions (asserted by expectations()): every family is of the lean class, in
every family some request is allowed and some denied.
"""
import numpy as np

from cilium_amd import l7match as L
from lean_job_cases import record
from lean_tail_cases import CUTS, cut  # noqa: F401  (the batch shapes: one tile, 64 records and one more)
from oracle import HttpOracle

R = L.PortRuleHTTP
ALPHA = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOP"


# ---- the header jobs ----------------------------------------------------------------
def nohdr_rules():
    return [R(Method="GET", Path="/a", Host="h"), R(Headers=["x-flag"]), R(Path="/b", Headers=["x-tenant"])]


def nohdr_records():
    flag, ten, other = (b"x-flag", b""), (b"x-tenant", b"t1"), (b"x-other", b"o")
    return [record(m, p, b"h", hdrs) for m in (b"GET", b"PUT") for p in (b"/a", b"/b", b"/c")
            for hdrs in ([], [flag], [ten], [other], [other, ten, flag], [ten, ten])]


def among_rules():
    # x-val owns the automaton; x-aa, x-bbbb and x-cccccc are presence-only fields
    return [R(Headers=["x-val: 0123"]), R(Headers=["x-aa", "x-val: 77"]), R(Path="/b", Headers=["x-bbbb"]),
            R(Headers=["x-cccccc", "x-bbbb"]), R(Method="QQ", Host="never")]


def among_records():
    good, v77, bad, far = (b"x-val", b"0123"), (b"x-val", b"77"), (b"x-val", b"0124"), (b"x-val", b"zzzz")
    aa, bb, cc, plain = (b"x-aa", b"1"), (b"x-bbbb", b""), (b"x-cccccc", b"c"), (b"ua", b"curl")
    out = []
    for host in (b"z", b"zz", b"zzz", b"zzzz"):
        for path in (b"/a", b"/b"):
            def rec(hdrs):
                return record(b"ZZ", path, host, hdrs)
            out += [
                rec([good, aa, bb, cc]), rec([aa, bb, cc, good]), rec([aa, good, bb]), rec([aa, bb, cc]),   # in front, behind, absent
                rec([aa, v77]), rec([v77, aa]), rec([aa, plain, v77, cc]), rec([aa, bad]), rec([aa, far]),
                rec([good, bad]), rec([bad, good]), rec([far, good]), rec([aa, bad, bb, good]), rec([v77, good, aa]),  # repeated
                rec([bb]), rec([cc]), rec([cc, bb]), rec([cc, plain, bb, far]), rec([]), rec([plain]),
            ]
    return out


def vlen_rules():
    return [R(Headers=["x-val: " + "0123456789"[:k]]) for k in range(1, 10)] + [R(Path="/e", Headers=["x-val"]),
                                                                               R(Method="QQ", Host="never")]


def vlen_records():
    out = []
    for host in (b"z", b"zz", b"zzz", b"zzzz"):          # the value's first byte at every alignment
        for k in range(10):
            for v in (b"0123456789"[:k], b"0123456788"[:k]):
                out += [record(b"GET", b"/e" if k % 2 else b"/f", host, [(b"x-val", v)]),
                        record(b"GET", b"/f", host, [(b"ua", b"c"), (b"x-val", v)])]
    return out


# ---- inline matchers -------------------------------------------------------------------
def sets_rules(n):
    """n nested method patterns a[a-zA-Z]*, ab[a-zA-Z]*, ...: the method automaton has n + 1 sets (n >= 2), one for n = 1."""
    return [R(Path="/p%d" % i, Method=ALPHA[:i + 1] + "[a-zA-Z]*") for i in range(n)] + [R(Path="/hh", Host="h")]


def sets_records():
    out = []
    for i in (0, 1, 2, 15, 29, 30, 31, 32):
        for j in (0, 1, 2, 15, 29, 30, 31, 32, 33):
            out.append(record(ALPHA[:j + 1].encode(), b"/p%d" % i, b"g"))
    out += [record(b"", b"/p0", b"g"), record(b"b", b"/p1", b"g"), record(None, b"/p0", b"g"), record(b"a", b"/hh", b"h")]
    return out


def codes_rules():
    # method codes: "lit" is latched (one pattern), "a", "ab..." end in sets, "zz" in code 0;
    # rules 2 and 3 share the path key class and differ in the method pattern only
    return [R(Path="/l", Method="lit"), R(Path="/s", Method="a.*"), R(Path="/t/.*", Method="ab.*"),
            R(Path="/t/x", Method="a.*"), R(Path="/u", Method="a.*", Host="h")]


def codes_records():
    return [record(m, p, a) for m in (b"lit", b"a", b"ab", b"abc", b"zz", b"", None)
            for p in (b"/l", b"/s", b"/t/x", b"/t/y", b"/u") for a in (b"h", b"g")]


def inline_rules():
    # (a record's matchers include the one on its key field, the path)
    return [
        R(Path="/m0"),                                                                     # 1 matcher
        R(Path="/m1", Method="G.*"),                                                       # 2
        R(Path="/m2", Method="G.*", Host="h"),                                             # 3
        R(Path="/m3", Method="G.*", Host="h", Headers=["x-val: v"]),                       # 4
        R(Path="/m4", Method="G.*", Host="h", Headers=["x-val: v", "x-flag"]),             # 5: scanned
        R(Path="/m5", Method="G.*", Host="h", Headers=["x-val: v", "x-flag", "x-more"]),   # 6: scanned
        R(Path="/two", Method="G.*", Headers=["x-flag"]), R(Path="/two", Method="G.*", Host="h"),  # a list of two
        R(Path="/abs", Headers=["x-val: v"]),                                              # a matcher on an absent field
    ]


def inline_records():
    v, w, f, more = (b"x-val", b"v"), (b"x-val", b"w"), (b"x-flag", b""), (b"x-more", b"1")
    out = []
    for p in (b"/m0", b"/m1", b"/m2", b"/m3", b"/m4", b"/m5", b"/two", b"/abs"):
        for m in (b"G", b"GET", b"PUT", None):
            for a in (b"h", b"g"):
                for hdrs in ([], [v], [v, f], [v, f, more], [w, f, more], [f, more]):
                    out.append(record(m, p, a, hdrs))
    return out


FAMILY_RULES = {
    "nohdr": nohdr_rules, "among": among_rules, "vlen": vlen_rules,
    "sets1": lambda: sets_rules(1), "sets31": lambda: sets_rules(30), "sets32": lambda: sets_rules(31),
    "sets33": lambda: sets_rules(32), "codes": codes_rules, "inline": inline_rules,
}
FAMILY_RECORDS = {
    "nohdr": nohdr_records, "among": among_records, "vlen": vlen_records, "sets": sets_records,
    "codes": codes_records, "inline": inline_records,
}
RECORDS_OF = {"sets1": "sets", "sets31": "sets", "sets32": "sets", "sets33": "sets"}
# the method automaton's set count per family that fixes one, and whether the program says kHttpInlineMasks
METHOD_SETS = {"sets1": 1, "sets31": 31, "sets32": 32, "sets33": 33}
INLINE_MASKS = {fam: fam != "sets33" for fam in FAMILY_RULES}
N_DFAS = {"nohdr": 3, "among": 4, "vlen": 4, "inline": 4}


def batch():
    """(arena, offsets, {record family: indices}): every family's records in a seeded shuffled order."""
    recs = [(fam, r) for fam in FAMILY_RECORDS for r in FAMILY_RECORDS[fam]()]
    recs *= -(-16 * 128 // len(recs))  # at least 16 x 128 records: two full tiles for each of a workgroup's waves
    order = np.random.default_rng(18).permutation(len(recs))
    where = {fam: [] for fam in FAMILY_RECORDS}
    out = []
    for i in order:
        where[recs[i][0]].append(len(out))
        out.append(recs[i][1])
    assert 16 * 128 <= len(out) <= 4096
    arena, offs = L.pack_records(out)
    return arena, offs, {fam: np.array(ix) for fam, ix in where.items()}


def expectations():
    """(batch, {family: oracle verdicts of the whole batch}); the conditions are asserted on the way."""
    arena, offs, where = batch()
    exp = {}
    for fam, mk in FAMILY_RULES.items():
        assert L.RuleSet.compile_http(mk()).http_lean, fam
        exp[fam] = HttpOracle(mk()).eval(arena, offs, threads=8)
        own = exp[fam][where[RECORDS_OF.get(fam, fam)]]
        assert (own >= 0).any() and (own == L.VERDICT_DENY).any(), fam
    return (arena, offs, where), exp


def error_batch(n):
    """n records that are all parse errors (a length word that disagrees with the parts)."""
    return L.pack_records([record(b"GET", b"/p%d" % (i % 7), b"h", rec_len=4 + (i % 3)) for i in range(n)])
