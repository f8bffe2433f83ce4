"""Records and rule sets for the lean HTTP kernel's walk jobs and verification
phase (l7m_http_impl.h: jobs 0-2 from the wave's scalars outside the job loop,
the header jobs behind them, the verification that follows); needs no GPU.
tests/test_http_lean_jobs_gpu.py evaluates them on the device,
tests/test_lean_job_cases.py checks the conditions below with the oracle.

Every family has its own rule set; one shared, shuffled batch holds the records
of all of them and every rule set is evaluated on the whole batch.

  flags      records lacking each of the method / path / authority flags
  dead_m/p/a an automaton that is dead from the start, for each of the three
  directory  0-4 headers of a referenced name length; the real one first,
             second, third, last, repeated, behind an unused name of the same
             length, among 255, behind 70,000 bytes; two referenced headers
  cands      candidate lists of length 1 with 0-4 matchers, of length 2 and
             more, latched and set end codes
  remote     rules with remote sets (hit, miss, empty set) and a zero-list rule
  presence   presence-only rules before and behind the path candidate
  f32 / f33  32 and 33 fields (the mask of present fields past one word): the
             same verdicts

Conditions (asserted by expectations()): every family is of the lean class;
in every family some request is allowed and some denied;
the verdict classes named in CLASSES occur where the family claims them.
"""
import struct

import numpy as np

from cilium_amd import l7match as L
from lean_tail_cases import CUTS, cut  # noqa: F401  (the batch shapes: one tile, 64 records and one more)
from oracle import HttpOracle

R = L.PortRuleHTTP


def record(method=b"GET", path=b"/", host=b"h", hdrs=(), remote=0, rec_len=None):
    """One raw record (include/l7match.h); None = the field is absent."""
    flags = (1 if method is not None else 0) | (2 if path is not None else 0) | (4 if host is not None else 0) | 8
    method, path, host = method or b"", path or b"", host or b""
    ents = [len(n) | len(v) << 16 for n, v in hdrs]
    body = b"".join(struct.pack("<I", e) for e in ents) + method + path + host + b"".join(n + v for n, v in hdrs)
    size = 20 + len(body)
    rec = struct.pack("<5I", size if rec_len is None else rec_len, remote, 80 | flags << 16 | len(hdrs) << 24,
                      len(method) | len(path) << 16, len(host)) + body
    return rec + b"\0" * (-len(rec) % 4)


# ---- flags -----------------------------------------------------------------------
def flags_rules():
    return [R(Method="GET", Path="/a", Host="h"), R(Method="PUT"), R(Path="/b"), R(Host="only")]


def flags_records():
    out = []
    for m in (b"GET", b"PUT", None):
        for p in (b"/a", b"/b", None):
            for a in (b"h", b"only", None):
                out.append(record(m, p, a))
    return out


# ---- automata dead from the start --------------------------------------------------
NEVER = "[^\\s\\S]"  # matches no string: the automaton's start state is dead


def dead_rules(field):
    live = {"Method": "GET", "Path": "/a", "Host": "h"}
    return [R(**{field: NEVER}), R(**{k: v for k, v in live.items() if k != field})]


def dead_records():
    return [record(m, p, a) for m in (b"GET", b"PUT", b"") for p in (b"/a", b"/b") for a in (b"h", b"x")]


# ---- the header directory ------------------------------------------------------------
def directory_rules():
    # x-val (5 bytes) has the one value automaton; x-tenant (8) and x-flag (6) are presence matchers
    return [R(Headers=["x-val: 0123"]), R(Path="/flag", Headers=["x-flag"]),
            R(Headers=["x-val: 01234567", "x-tenant"]), R(Method="QQ", Host="never\\.host")]


def directory_records():
    good, bad = (b"x-val", b"0123"), (b"x-val", b"0124")
    long_ = (b"x-val", b"01234567")
    look = (b"y-val", b"0123")     # a referenced length, a name no rule uses
    look8 = (b"y-tenant", b"t")
    plain = (b"ua", b"curl/8")
    ten, flag = (b"x-tenant", b"t12"), (b"x-flag", b"")
    out = []
    for host in (b"z", b"zz", b"zzz", b"zzzz"):  # the directory's names at every alignment
        def rec(hdrs, path=b"/zzz"):
            return record(b"ZZZZ", path, host, hdrs)
        out += [
            rec([]), rec([plain]),                                                  # 0 referenced lengths
            rec([good]), rec([bad]), rec([look]),                                   # 1
            rec([good, look]), rec([look, good]), rec([look, bad]), rec([plain, look, plain, good]),  # 2
            rec([good, look, look]), rec([look, good, look]), rec([look, look, good]), rec([look, look, bad]),  # 3
            rec([good, look, look8, look]), rec([look, good, look8, look]), rec([look, look8, good, look]),  # 4
            rec([look, look8, look, good]), rec([look, look8, look, bad]), rec([look, plain, look8, plain, look, good]),
            rec([good, bad]), rec([bad, good]), rec([look, good, bad]), rec([look, look, bad, good]),  # repeated
            rec([long_, ten]), rec([ten, long_]), rec([look, ten, look8, long_]), rec([long_]), rec([ten]),  # both must hold
            rec([long_, (b"x-tenanu", b"t")]), rec([look, look8, ten, plain, long_]), rec([bad, ten]),
            rec([flag], b"/flag"), rec([flag]), rec([look, look8, flag], b"/flag"), rec([look, look, look8, flag], b"/flag"),
            rec([good], b"/zzz") if host != b"zz" else record(b"ZZZZ", b"/zzz", host, [good], rec_len=4),  # a bad record
        ]
    fill = [(b"h%d" % k, b"v") for k in range(254)]      # names of 2-4 bytes: no rule references these lengths
    fill5 = [(b"q%04d" % k, b"v") for k in range(254)]   # 5 bytes: every one is a candidate
    for hit in (good, bad):
        out += [record(b"ZZZZ", b"/zzz", b"zz", [hit] + fill), record(b"ZZZZ", b"/zzz", b"zz", fill + [hit]),
                record(b"ZZZZ", b"/zzz", b"zz", fill5[:1] + fill[:100] + [hit] + fill[100:253]),
                record(b"ZZZZ", b"/zzz", b"zz", fill5[:40] + [hit] + fill[:214])]
        for name in (b"bulk", b"y-val"):  # behind 70,000 bytes of values (two values of 35,000: a length has 16 bits)
            out.append(record(b"ZZZZ", b"/zzz", b"zz", [(name, b"b" * 35000), (name, b"b" * 35000), hit]))
    return out


# ---- candidate lists -------------------------------------------------------------------
def cands_rules():
    return [
        R(Path="/m0"),                                                              # list of 1, no other matcher
        R(Path="/m1", Method="GET"),                                                # 1 inline matcher
        R(Path="/m2", Method="GET", Host="h"),                                      # 2
        R(Path="/m3", Method="GET", Host="h", Headers=["x-val: v"]),                # 3
        R(Path="/m4", Method="GET", Host="h", Headers=["x-val: v", "x-flag"]),      # 4
        R(Path="/m5", Method="GET", Host="h", Headers=["x-val: v", "x-flag", "x-more"]),  # 5: not inline
        R(Path="/two", Method="PUT"), R(Path="/two", Method="GET"),                 # a list of 2
        R(Path="/many", Method="A"), R(Path="/many", Method="B"), R(Path="/many", Host="c"), R(Path="/many", Host="d"),
        R(Path="/s/ab", Method="PUT"), R(Path="/s/a.*", Method="GET"), R(Path="/s/.*"),  # set end codes
    ]


def cands_records():
    out = []
    v, f, more = (b"x-val", b"v"), (b"x-flag", b""), (b"x-more", b"1")
    for p in (b"/m0", b"/m1", b"/m2", b"/m3", b"/m4", b"/m5", b"/m6"):
        for m in (b"GET", b"PUT"):
            for a in (b"h", b"g"):
                for hdrs in ([], [v], [v, f], [v, f, more], [(b"x-val", b"w"), f, more], [f, more]):
                    out.append(record(m, p, a, hdrs))
    for m in (b"GET", b"PUT", b"A", b"B", b"C"):
        for a in (b"c", b"d", b"e"):
            out += [record(m, b"/two", a), record(m, b"/many", a)]
    for p in (b"/s/", b"/s/a", b"/s/ab", b"/s/abc", b"/s", b"/t/ab"):
        for m in (b"GET", b"PUT", b"A"):
            out.append(record(m, p, b"h"))
    return out


# ---- remote sets ------------------------------------------------------------------------
def remote_rules():
    return [R(Path="/r", RemoteIDs=[5, 9, 700]), R(Path="/any", RemoteIDs=[]), R(Path="/r2", Method="GET", RemoteIDs=[9]),
            R(Method="ZL", Host="zl", RemoteIDs=[1]), R(RemoteIDs=[42, 43])]  # the last: the zero list


def remote_records():
    return [record(m, p, b"h", remote=r) for p in (b"/r", b"/any", b"/r2", b"/no") for m in (b"GET", b"PUT")
            for r in (0, 5, 7, 9, 42, 43, 700, 701)]


# ---- presence lists -------------------------------------------------------------------
def presence_rules():
    return [R(Headers=["x-first"]), R(Path="/p", Method="GET"), R(Headers=["x-later"]), R(Path="/q"),
            R(Host="hh", Headers=["x-later", "x-first"])]


def presence_records():
    first, later, other = (b"x-first", b"1"), (b"x-later", b""), (b"x-other", b"1")
    out = []
    for p in (b"/p", b"/q", b"/n"):
        for m in (b"GET", b"PUT"):
            for hdrs in ([], [first], [later], [other], [first, later], [other, later], [later, other, first]):
                out.append(record(m, p, b"h", hdrs))
    return out


# ---- the field-count edge ----------------------------------------------------------------
def fields_rules(n_fields):
    """A rule set with n_fields fields: method, path, authority and presence headers."""
    return [R(Method="GET", Path="/a", Host="h")] + [R(Headers=["x-h%02d" % k]) for k in range(n_fields - 3)]


def fields_records():
    out = [record(b"GET", b"/a", b"h"), record(b"PUT", b"/a", b"h")]
    for k in (0, 1, 15, 27, 28, 29, 30):
        out += [record(b"PUT", b"/b", b"h", [(b"x-h%02d" % k, b"")]),
                record(b"PUT", b"/b", b"h", [(b"ua", b"x"), (b"x-h%02d" % k, b"1"), (b"x-h00", b"")])]
    return out


FAMILY_RULES = {
    "flags": flags_rules, "dead_m": lambda: dead_rules("Method"), "dead_p": lambda: dead_rules("Path"),
    "dead_a": lambda: dead_rules("Host"), "directory": directory_rules, "cands": cands_rules, "remote": remote_rules,
    "presence": presence_rules, "f32": lambda: fields_rules(32), "f33": lambda: fields_rules(33),
}
FAMILY_RECORDS = {
    "flags": flags_records, "dead": dead_records, "directory": directory_records, "cands": cands_records,
    "remote": remote_records, "presence": presence_records, "fields": fields_records,
}
RECORDS_OF = {"dead_m": "dead", "dead_p": "dead", "dead_a": "dead", "f32": "fields", "f33": "fields"}
GENERIC = ()  # families outside the lean class: none
# Verdict classes a family must show on its own records: "cand" = allowed by a rule found through a
# candidate entry, "pres" = allowed by a presence-list or zero-list rule (the rule indices named), "deny", "error".
CLASSES = {
    "flags": {"cand": (0, 1, 2, 3), "deny": True},
    "dead_m": {"cand": (1,), "deny": True}, "dead_p": {"cand": (1,), "deny": True}, "dead_a": {"cand": (1,), "deny": True},
    "directory": {"cand": (0, 1, 2), "deny": True, "error": True},
    "cands": {"cand": tuple(range(15)), "deny": True},
    "remote": {"cand": (0, 1, 2), "pres": (4,), "deny": True},
    "presence": {"cand": (1, 3), "pres": (0, 2), "deny": True},
    "f32": {"cand": (0,), "pres": (1, 16, 28, 29), "deny": True},
    "f33": {"cand": (0,), "pres": (1, 16, 28, 29, 30), "deny": True},
}


def batch():
    """(arena, offsets, {record family: indices}): every family's records in a seeded shuffled order."""
    recs = [(fam, r) for fam in FAMILY_RECORDS for r in FAMILY_RECORDS[fam]()]
    recs *= -(-16 * 65 // len(recs))  # at least 16 x 65 records: every case again at another place of the batch
    order = np.random.default_rng(16).permutation(len(recs))
    where = {fam: [] for fam in FAMILY_RECORDS}
    out = []
    for i in order:
        where[recs[i][0]].append(len(out))
        out.append(recs[i][1])
    assert 16 * 65 <= len(out) <= 4096
    arena, offs = L.pack_records(out)
    return arena, offs, {fam: np.array(ix) for fam, ix in where.items()}


def expectations():
    """(batch, {family: oracle verdicts of the whole batch}); the conditions are asserted on the way."""
    arena, offs, where = batch()
    exp = {}
    for fam, mk in FAMILY_RULES.items():
        assert L.RuleSet.compile_http(mk()).http_lean == (fam not in GENERIC), fam
        exp[fam] = HttpOracle(mk()).eval(arena, offs, threads=8)
        own = exp[fam][where[RECORDS_OF.get(fam, fam)]]
        want = CLASSES[fam]
        for rid in want.get("cand", ()) + want.get("pres", ()):
            assert (own == rid).any(), (fam, "no request allowed by rule", rid)
        assert (own == L.VERDICT_DENY).any(), fam
        if want.get("error"):
            assert (own == L.VERDICT_PARSE_ERROR).any(), fam
    assert np.array_equal(exp["f32"], np.where(exp["f33"] == 30, L.VERDICT_DENY, exp["f33"]))  # (rule 30: the 33rd field's)
    return (arena, offs, where), exp
