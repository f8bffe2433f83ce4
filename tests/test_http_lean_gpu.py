"""GPU parity tests of the lean HTTP first pass (l7m_http_impl.h kFeatLean,
l7m_dispatch.h http_program_lean): every rule set of the lean class is
evaluated twice -- by the lean kernel and, compiled under L7M_HTTP_GENERIC=1,
by the generic one -- and both must equal the CPU oracle bit for bit, verdicts
and per-rule hit counters; one rule set per clause of the predicate reports
"not lean" and still equals the oracle.  The records stress the field tails
(lengths around the walk's 4- and 8-byte blocks, the deciding byte first and
last), the header directory (no header, repeated and look-alike names, 255
headers) and the tile's edges (bad records between good ones, a record larger
than the stage, batches of 1, 63, 64 and 65).  All batches are <= 4096
records."""
import re
import struct

import numpy as np
import pytest

from cilium_amd import l7match as L
from cilium_amd import workloads as W
from oracle import HttpOracle, PolicyOracle
from program_interp import KNONE, HttpProgram

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)
UPPER, LOWER, HOSTC, DIGITS = b"ABCDEFGHIJKLMNOPQRS", b"/abcdefghijklmnopqr", b"hijklmnopqrstuvwxyz", b"0123456789"
LIT = "lit-0123456789"


# ---- records -------------------------------------------------------------------
def record(method=b"GET", path=b"/", host=b"h", hdrs=(), policy=0, rec_len=None, dir_add=0, ingress=True, port=80):
    """One raw record (include/l7match.h); None = the field is absent (flag bit
    clear).  rec_len: the length word written (default: the true one);
    dir_add: added to the first directory entry's value length."""
    flags = (1 if method is not None else 0) | (2 if path is not None else 0) | (4 if host is not None else 0) | \
        (8 if ingress else 0)
    method, path, host = method or b"", path or b"", host or b""
    ents = [len(n) | len(v) << 16 for n, v in hdrs]
    if dir_add:
        ents[0] += dir_add << 16
    body = b"".join(struct.pack("<I", e) for e in ents) + method + path + host + b"".join(n + v for n, v in hdrs)
    size = 20 + len(body)
    rec = struct.pack("<5I", size if rec_len is None else rec_len, 0, port | flags << 16 | len(hdrs) << 24,
                      len(method) | len(path) << 16, len(host) | policy << 16) + body
    return rec + b"\0" * (-len(rec) % 4)


def flip(b, at):
    return b[:at] + b"~" + b[at + 1:]


def matching(rule, tenant=None):
    """(method, path, host, headers) of a request that config-2-shaped `rule` allows."""
    m = rule.Method.split("|")[0] if rule.Method and "[" not in rule.Method else "GET"
    p = rule.Path.replace("v[0-9]+", "v12").replace("(users|orders|items)", "orders").replace("[0-9]+", "7") \
        .replace(".*", "q")
    h = rule.Host.replace("\\.", ".") if rule.Host else "other.host"
    hdrs = []
    for s in rule.Headers:
        name, _, val = s.partition(": ")
        hdrs.append((name.encode(), (tenant if tenant is not None and name == "x-tenant" else val or "1").encode()))
    return m.encode(), p.encode(), h.encode(), hdrs


def length_records():
    """Method, path and authority of every length of LENGTHS, exact and with the
    first or the last byte changed; header values of length 0-9 (and 10, 14)."""
    out = []
    for f, base in enumerate((UPPER, LOWER, HOSTC)):
        for n in LENGTHS:
            for v in {base[:n], flip(base[:n], 0) if n else b"", flip(base[:n], n - 1) if n else b""}:
                vals = [b"ZZ", b"/zz", b"zz"]
                vals[f] = v
                out.append(record(*vals))
    for name in (b"x-val", b"x-tenant"):
        for n in list(range(10)) + [10, 14]:
            for v in {DIGITS[:n], (b"t" + DIGITS)[:n], LIT.encode()[:n], flip(LIT.encode()[:n], n - 1) if n else b""}:
                out.append(record(b"POST", b"/api/sjqvjzik/x", b"zz", [(name, v)]))
    return out


def header_records(rules):
    """The header jobs: for every rule with a header matcher, its matching
    request with the directory shapes that move the lane's header cursor."""
    out = []
    named = [r for r in rules if r.Headers]
    for r in named[:12]:
        m, p, h, hdrs = matching(r)
        name, val = hdrs[0]
        other = b"y" + name[1:]  # the referenced length, another name
        out += [
            record(m, p, h, []),                                            # n_hdr = 0
            record(m, p, h, hdrs),                                          # the referenced header(s) alone
            record(m, p, h, [(other, val)] + hdrs),                         # a look-alike in front of the real one
            record(m, p, h, [(other, val)]),
            record(m, p, h, [(name, val + b"~"), (name, val)]),             # first occurrence wins: no match
            record(m, p, h, [(name, val), (name, val + b"~")]),
            record(m, p, h, [(b"x-debug", b"1"), (b"x-tenant", val), (b"x-flag", b"")]),  # different referenced headers
            record(m, p, h, [(b"x-tenant", val), (b"x-val", val), (b"x-debug", b"")]),
            record(m, p, h, [(b"h%d" % k, b"v") for k in range(254)] + [(name, val)]),  # 255 headers, the last one referenced
            record(m, p, h, [(b"accept", b"*/*"), (b"user-agent", b"curl/8"), (name.upper(), val)] + hdrs),
        ]
    return out


def odd_records(rules):
    """Absent fields, bad records between good ones, policy != 0, a record
    larger than any record stage between staged ones."""
    m, p, h, hdrs = matching(rules[1])
    good = record(m, p, h, hdrs)
    big = record(m, p, h, [(b"x-big", b"b" * 9000)] + hdrs)  # > program.h L7M_HTTP_MAX_STAGE: read from HBM
    out = [good, record(None, p, h, hdrs), record(m, None, h, hdrs), record(m, p, None, hdrs),
           record(None, None, None, []), good,
           record(m, p, h, hdrs, rec_len=len(good) + 4), good,                   # a wrong rec_len
           record(m, p, h, [(b"x-a", b"1")] + hdrs, dir_add=1), good,            # a directory that does not add up
           record(m, p, h, [(b"x-a", b"1")], rec_len=8), good,
           record(m, p, h, hdrs, policy=1), good, big, good, big, big, good]
    return out


def batch(rules):
    recs = length_records() + header_records(rules) + odd_records(rules)
    traffic, toffs = W.requests(2, 0, 1200, n_rules=50)
    ends = list(toffs[1:]) + [traffic.nbytes]
    recs += [traffic[int(a):int(b)].tobytes() for a, b in zip(toffs, ends)]
    order = np.random.default_rng(7).permutation(len(recs))  # bad and large records land inside ordinary tiles
    recs = [recs[i] for i in order]
    assert len(recs) <= 4096
    return L.pack_records(recs), [struct.unpack_from("<I", r, 16)[0] >> 16 for r in recs]


# ---- rule sets -------------------------------------------------------------------
def config2_rules():
    """Config-2-shaped: its generator's rules, a header literal and a presence-only header."""
    return W.rules(2, n_rules=50) + [L.PortRuleHTTP(Headers=["x-tenant: " + LIT]),
                                     L.PortRuleHTTP(Path="/api/sjqvjzik/.*", Headers=["x-flag"])]


def length_rules():
    """One literal rule per field and length, so the field's last bytes decide."""
    rules = []
    for field, base in (("Method", UPPER), ("Path", LOWER), ("Host", HOSTC)):
        rules += [L.PortRuleHTTP(**{field: base[:n].decode()}) for n in LENGTHS if n]
    rules += [L.PortRuleHTTP(Headers=["x-val: " + DIGITS[:n].decode()]) for n in range(1, 10)]
    return rules + [L.PortRuleHTTP(Path="/zz", Headers=["x-flag"])]


def expected(oracle, arena, offs, policies):
    exp = oracle.eval(arena, offs, threads=8)
    # (HttpOracle has no endpoint policies: include/l7match.h, a record naming a policy the map lacks is denied)
    exp[np.array(policies) != 0] = L.VERDICT_DENY
    return exp


def check(rs, arena, offs, exp, hits):
    h = np.zeros(rs.n_counters, dtype=np.uint64) if hits else None
    got = rs.eval(arena, offs, h)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, [(int(i), int(exp[i]), int(got[i])) for i in bad[:10]]
    if hits:
        want = np.zeros(rs.n_counters, dtype=np.uint64)
        want[0] = (exp == L.VERDICT_DENY).sum()
        want[1] = (exp <= L.VERDICT_PARSE_ERROR).sum()
        np.add.at(want, 2 + exp[(exp >= 0) & (exp < L.VERDICT_ALLOW_NO_PORT_POLICY)], 1)
        assert np.array_equal(h, want)


@pytest.fixture(scope="module")
def cases():
    """Per lean rule set: the rules, the shared batch and the oracle's verdicts (computed once)."""
    out = {}
    for name, rules in (("config2", config2_rules()), ("lengths", length_rules())):
        (arena, offs), policies = batch(config2_rules())
        exp = expected(HttpOracle(rules), arena, offs, policies)
        out[name] = (rules, arena, offs, exp, policies)
    return out


def compile_both(rules, monkeypatch, **kw):
    lean = L.RuleSet.compile_http(rules, **kw)
    monkeypatch.setenv("L7M_HTTP_GENERIC", "1")
    generic = L.RuleSet.compile_http(rules, **kw)
    monkeypatch.delenv("L7M_HTTP_GENERIC")
    return lean, generic


@pytest.mark.parametrize("name", ["config2", "lengths"])
@pytest.mark.parametrize("hits", [False, True])
def test_lean_and_generic_equal_the_oracle(gpu, cases, monkeypatch, name, hits):
    rules, arena, offs, exp, _ = cases[name]
    lean, generic = compile_both(rules, monkeypatch)
    assert lean.http_lean and not generic.http_lean
    # (every rule of the set decides some record; the three bad records are parse errors)
    assert len(np.unique(exp[exp >= 0])) >= 42 and (exp == L.VERDICT_DENY).any()
    assert (exp == L.VERDICT_PARSE_ERROR).sum() == 3
    for rs in (lean, generic):
        check(rs, arena, offs, exp, hits)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches(gpu, cases, monkeypatch, n):
    """A batch of n records (one wave, a tile of n or 64 + 1), taken where the odd records are."""
    rules, arena, offs, exp, policies = cases["config2"]
    lean, generic = compile_both(rules, monkeypatch)
    first = int(np.nonzero(exp == L.VERDICT_PARSE_ERROR)[0][0])
    lo = max(0, min(first - n // 2, len(offs) - n))
    sub = offs[lo:lo + n] - offs[lo]
    end = int(offs[lo + n]) if lo + n < len(offs) else arena.nbytes
    sub_arena = arena[int(offs[lo]):end]
    for rs in (lean, generic):
        for hits in (False, True):
            check(rs, sub_arena, sub, exp[lo:lo + n], hits)


def _not_lean_sets():
    base = config2_rules()
    return {
        "five_value_dfas": (base + [L.PortRuleHTTP(Headers=["x-val: 12"])], {}, {}),
        "out_of_lds": (base, {"lds_budget_bytes": 1024}, {}),
        "forced_capture": (base + [L.PortRuleHTTP(Path="/(\\w+)/\\1(/.*)?")], {}, {}),
        "re2_dialect": (base, {"dialect": L.DIALECT_RE2_SEARCH}, {"dialect": L.DIALECT_RE2_SEARCH}),
        "slow_path_rule": (base + [L.PortRuleHTTP(Path="/(a|bb)+-\\1")], {}, {}),
    }


def _clauses_failed(rs):
    """The clauses of l7m_dispatch.h http_program_lean that the rule set's program fails."""
    P = HttpProgram(rs.program())
    h, value = P.h, P.dfas[:P.h["n_dfas"]]
    failed = set()
    if not h["single_entry"] or h["allow_no_l7"]:
        failed.add("entry")
    if h["search"]:
        failed.add("search")
    if h["lds_dcap"] != KNONE:
        failed.add("dcap")
    if h["n_slow"]:
        failed.add("slow")
    if h["n_dfas"] > 4:
        failed.add("n_dfas")
    if any(d["kind"] != 0 or d["lit_tab"] != KNONE for d in value):
        failed.add("kind")
    if any(d["lds_table"] == KNONE or d["lds_es"] != 0xFFFFFFFE or d["lds_skip"] != KNONE for d in value):
        failed.add("lds")
    return failed


# the clause each rule set is built to fail (the RE2 dialect also splits the automata)
_NOT_LEAN_CLAUSE = {"five_value_dfas": {"n_dfas"}, "out_of_lds": {"lds"}, "forced_capture": {"dcap"},
                    "re2_dialect": {"search"}, "slow_path_rule": {"slow"}}


@pytest.mark.parametrize("kind", ["five_value_dfas", "out_of_lds", "forced_capture", "re2_dialect", "slow_path_rule"])
def test_programs_outside_the_class_are_not_lean(gpu, cases, kind):
    rules, ckw, okw = _not_lean_sets()[kind]
    rs = L.RuleSet.compile_http(rules, **ckw)
    assert not rs.http_lean
    failed = _clauses_failed(rs)
    assert _NOT_LEAN_CLAUSE[kind] <= failed, (kind, failed)
    # ... and that clause alone (a forced capture's R automaton and the RE2 dialect's search
    # automata are also walked from the program, so those two fail further clauses)
    if kind not in ("forced_capture", "re2_dialect"):
        assert failed == _NOT_LEAN_CLAUSE[kind], (kind, failed)
    _, arena, offs, _, policies = cases["config2"]
    extra = [record(b"GET", p) for p in (b"/ab/ab", b"/ab/ab/c", b"/ab/ac", b"/bb-bb", b"/abb-a", b"/a-bb")]
    (xa, xo) = L.pack_records(extra)
    arena2 = np.concatenate([arena, xa])
    offs2 = np.concatenate([offs, xo + np.uint64(arena.nbytes)])
    exp = expected(HttpOracle(rules, **okw), arena2, offs2, policies + [0] * len(extra))
    check(rs, arena2, offs2, exp, True)


def test_two_endpoint_policies_are_not_lean(gpu, cases):
    rules, arena, offs, _, _ = cases["config2"]
    pols = [L.NetworkPolicy(Name=f"ep{i}", Ingress=[L.PortNetworkPolicy(Port=80, Rules=[
        L.PortNetworkPolicyRule(HttpRules=r)])]) for i, r in enumerate((rules, length_rules()))]
    rs = L.RuleSet.compile_http_policies(pols)
    assert not rs.http_lean
    assert "entry" in _clauses_failed(rs)  # (the two policies' rule sets also add up to more than four automata)
    assert _clauses_failed(L.RuleSet.compile_http(rules)) == set()
    exp = PolicyOracle(pols).eval(arena, offs, threads=8)
    assert (exp >= 0).any() and (exp == L.VERDICT_DENY).any()
    check(rs, arena, offs, exp, True)


def test_matching_helper_builds_allowed_requests(gpu, cases):
    """The crafted requests do reach the rules they were derived from (the
    header records are not all denials)."""
    rules = config2_rules()
    recs = [record(*matching(r)) for r in rules[:50]]
    arena, offs = L.pack_records(recs)
    exp = HttpOracle(rules).eval(arena, offs, threads=8)
    assert (exp >= 0).all() and (exp <= np.arange(50)).all()
    check(L.RuleSet.compile_http(rules), arena, offs, exp, True)
