"""GPU parity of the dense class-compressed DFA kind (program.h kDfaDense,
l7m_http_impl.h walk_dense, the kFeatDense instantiations).  Every test
compiles the same rules twice, dense (l7m_opts.flags) and packed, and requires
dense == packed == the CPU oracle on every verdict and on the rule_hits
counters; the dense compile must hold dense automata, so nothing here passes
without the kind."""
import struct
import threading

import numpy as np
import pytest

import regex_ext_cases as X
from cilium_amd import l7match as L
from cilium_amd import workloads as W
from oracle import HttpOracle, PolicyOracle
from policy_cases import random_policies, random_requests
from program_interp import KNONE
from program_interp_dense import DFA_DENSE, DenseHttpProgram

pytestmark = pytest.mark.gpu


def _eval_checked(rs, arena, offs, exp):
    h = np.zeros(rs.n_counters, dtype=np.uint64)
    got = rs.eval(arena, offs, h)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, [(int(i), int(exp[i]), int(got[i])) for i in bad[:10]]
    # counters as tests/test_regex_ext_gpu.py _check
    assert int(h[0]) == int((exp == -1).sum())
    for r in np.unique(exp[exp >= 0])[:64]:
        assert int(h[2 + r]) == int((exp == r).sum())
    assert int(h.sum()) == len(exp)
    return got


def _check(rules, arena, offs, dense_dfa, exp=None, want_dense=True, **kw):
    """dense == packed == oracle; returns the dense rule set."""
    if exp is None:
        exp = HttpOracle(rules).eval(arena, offs, threads=8)
    rd = L.RuleSet.compile_http(rules, dense_dfa=dense_dfa, **kw)
    rp = L.RuleSet.compile_http(rules, **kw)
    assert rp.info.n_dense_dfas == 0
    assert (rd.info.n_dense_dfas > 0) == want_dense
    _eval_checked(rd, arena, offs, exp)
    _eval_checked(rp, arena, offs, exp)
    return rd


def _budget_where(rules, pred):
    """The smallest LDS budget (bytes, 128-byte steps) whose dense compile satisfies pred(program):
    what lands in LDS depends on the fixed part of the image, so tests look the budget up."""
    for budget in range(1024, 65536, 128):
        P = DenseHttpProgram(L.RuleSet.compile_http(rules, dense_dfa=2, lds_budget_bytes=budget).program())
        if pred(P):
            return budget
    raise AssertionError("no budget gives the wanted placement")


def _lds_maps(P):
    return [k for k in P.dense_dfas if P.dfas[k]["lds_cmap"] != KNONE]


def test_random_extended_rule_sets(gpu):
    """Look-ahead / \\b / back-reference rule sets, the shape at which the dense
    table already is the smaller one (12 such rules: 37 KB packed, 1 KB dense)."""
    rng = np.random.default_rng(7)
    for trial in range(8):
        rules = X.random_rules(rng, int(rng.integers(1, 24)), backrefs=trial % 2 == 1)
        arena, offs = L.pack_http(X.random_requests(rng, 4000))
        _check(rules, arena, offs, dense_dfa=1, lds_budget_bytes=1)


@pytest.mark.parametrize("n_rules", [40, 400])
def test_tail_sharing_and_latch_recovery(gpu, n_rules):
    """Config 2's shape: a prefix trie of multi-pattern states (400 rules: 104)
    in front of one shared latched tail (700 states); the pattern comes from
    latch[slot of the transition that left the multi-pattern region].  Budget
    1: every automaton from the program, class maps too; a few KiB: the path
    automaton dense beside automata walked from LDS, a class map in LDS;
    default: everything is walked from LDS, so nothing is eligible."""
    rules = W.rules(2, n_rules=n_rules)
    arena, offs = W.requests(2, 7_000_000, 20_000, n_rules=n_rules)
    exp = HttpOracle(rules).eval(arena, offs, threads=8)
    assert (exp >= 0).sum() > 1000 and (exp == -1).sum() > 1000
    rd = _check(rules, arena, offs, 2, exp=exp, lds_budget_bytes=1)
    P = DenseHttpProgram(rd.program())
    assert rd.info.n_dense_dfas == 4 and all(P.dfas[k]["lds_cmap"] == KNONE for k in P.dense_dfas)
    mixed = _budget_where(rules, lambda P: P.dfas[1]["kind"] == DFA_DENSE and _lds_maps(P) and
                          any(d["lds_table"] != KNONE for d in P.dfas[:4]))
    _check(rules, arena, offs, 2, exp=exp, lds_budget_bytes=mixed)
    _check(rules, arena, offs, 2, exp=exp, want_dense=False)


def _pack_raw(reqs):
    """(method, path or None, host, [(name, value)]) byte tuples -> (arena, offsets)."""
    recs = []
    for method, path, host, hdrs in reqs:
        flags = 1 | (2 if path is not None else 0) | 4
        path = path or b""
        body = b"".join(struct.pack("<I", len(n) | len(v) << 16) for n, v in hdrs)
        body += method + path + host + b"".join(n + v for n, v in hdrs)
        rec = struct.pack("<5I", 20 + len(body), 0, 80 | flags << 16 | len(hdrs) << 24, len(method) | len(path) << 16,
                          len(host)) + body
        recs.append(rec + b"\0" * (-len(rec) % 4))
    return L.pack_records(recs)


def _byte_strings(rng, n):
    """Values of every length 0-17 and 31-33 (the walk's 8-byte blocks, its
    4-byte block and its 1-3 byte tail), over NUL, high bytes and a few
    letters; some are built to match."""
    lens = list(range(0, 18)) + [31, 32, 33]
    al = np.frombuffer(b"ab/\x00\x80\xfe\xff", dtype=np.uint8)
    out = []
    for i in range(n):
        ln = lens[i % len(lens)]
        r = rng.random()
        if r < 0.35:
            s = (b"/a" + b"\xff" * 40)[:ln]
        elif r < 0.55:
            s = (b"\x00" * 40)[:ln]
        elif r < 0.7:
            s = (b"/" + b"\x80\x81" * 20)[:max(ln - 2, 0)] + b"/b"[:min(ln, 2)]
        else:
            s = bytes(rng.choice(al, ln))
        out.append(s)
    return out


@pytest.mark.parametrize("single", [False, True])
def test_field_lengths_and_bytes(gpu, single):
    """Paths (regexes) and the values of a referenced header (literals, as
    Envoy matches them) of every length 0-17 and 31-33 with NUL and high bytes;
    requests without a :path, without the header, with an empty value."""
    rng = np.random.default_rng(90)
    if single:  # one pattern per automaton: the start state is latched
        rules = [L.PortRuleHTTP(Path="/a[\\x80-\\xff]*", Headers=[b"x-k: /a\xff\xff\xff"])]
    else:
        lits = [(b"/a" + b"\xff" * 40)[:n] for n in (1, 3, 8, 9, 16, 17, 31, 32, 33)]
        lits += [(b"/" + b"\x80\x81" * 20)[:n - 2] + b"/b" for n in (4, 12, 33)]
        rules = [L.PortRuleHTTP(Path="\\x00*", Method="GET"), L.PortRuleHTTP(Path="/[\\x80-\\xff]{2,}/b", Method="PUT"),
                 L.PortRuleHTTP(Path="[ab/]*\\xfe.*", Headers=["x-k"])]
        rules += [L.PortRuleHTTP(Path="/a[\\x80-\\xff]*" if j % 2 else "", Headers=[b"x-k: " + v])
                  for j, v in enumerate(lits)]
        rules += [L.PortRuleHTTP(Path="/a[\\x80-\\xff]*")]
    paths, vals = _byte_strings(rng, 2100), _byte_strings(rng, 2100)
    reqs = []
    for i, (p, v) in enumerate(zip(paths, vals)):
        hdrs = [(b"x-k", v)] if i % 5 else []          # every fifth request: no such header
        if i % 7 == 3:
            hdrs = [(b"x-j", b"zz")] + hdrs + [(b"x-k", b"v")]  # first occurrence wins
        reqs.append(([b"GET", b"PUT"][i % 2], None if i % 11 == 5 else p, b"h", hdrs))  # every eleventh: no :path
    arena, offs = _pack_raw(reqs)
    exp = HttpOracle(rules).eval(arena, offs, threads=8)
    assert len(set(exp.tolist())) >= (2 if single else 12)
    # class maps from the program, then the path's (at least) from LDS
    for budget in (1, _budget_where(rules, lambda P: 1 in _lds_maps(P))):
        rd = _check(rules, arena, offs, 2, exp=exp, lds_budget_bytes=budget)
        P = DenseHttpProgram(rd.program())
        assert 1 in P.dense_dfas and (1 in _lds_maps(P)) == (budget > 1)
        if single:
            assert all(P.dfas[k]["start_latch"] != KNONE and P.dfas[k]["region"] == 1 for k in P.dense_dfas)


def test_records_outside_the_stage(gpu):
    """Records the wave's LDS stage does not hold are walked by the same code
    reading HBM directly (GlbSrc): a record with a 9 KiB header value, and a
    batch whose offsets are not contiguous."""
    rng = np.random.default_rng(91)
    big_ok = "ab" * 4600 + "d"  # 9 KiB: longer than a wave's stage
    big_no = "ab" * 4600 + "e"
    rules = [L.PortRuleHTTP(Path="/svc[0-9]+/.*", Headers=["x-big: " + big_ok]),  # (header values are literals)
             L.PortRuleHTTP(Path="/(?!admin).*", Headers=["x-big: abd"]),
             L.PortRuleHTTP(Path="/admin/[a-z]+", Method="GET"),
             L.PortRuleHTTP(Path="/big/(ab|c)*d")]
    reqs = []
    for i in range(3000):
        r = i % 100
        val = big_ok if r in (7, 31) else big_no if r == 53 else str(rng.choice(["abd", "x zz", "ab", ""]))
        path = str(rng.choice(["/svc1/x", "/admin/x", "/svc22/", "/other", "/admin/1"]))
        if r == 77:
            path = "/big/" + (big_ok if i % 200 < 100 else big_no)
        reqs.append(L.HTTPRequest(str(rng.choice(["GET", "POST"])), path, "h", [("x-big", val)] if val else []))
    arena, offs = L.pack_http(reqs)
    exp = HttpOracle(rules).eval(arena, offs, threads=8)
    assert {0, 1, 2, 3, -1} <= set(exp.tolist())
    _check(rules, arena, offs, 2, exp=exp, lds_budget_bytes=1)
    perm = rng.permutation(len(offs))  # non-contiguous offsets: every lane reads HBM
    _check(rules, arena, offs[perm], 2, exp=exp[perm], lds_budget_bytes=1)


@pytest.mark.parametrize("n_fields", [1, 4, 8])
def test_end_code_storage(gpu, n_fields):
    """<= 4, 5-8 and > 8 value automata: end codes in 4 registers, 8 registers
    or LDS columns (Codes<4>, <8>, <0>), every value automaton dense; the
    header-name automaton stays packed and is walked from the program."""
    rng = np.random.default_rng(7100 + n_fields)
    names = [f"x-h{j}" for j in range(n_fields)]
    rules = []
    for i in range(60):
        hs = []
        for j in rng.choice(n_fields, size=min(n_fields, 1 + int(rng.integers(0, 3))), replace=False):
            hs.append(f"{names[j]}: v{int(rng.integers(0, 4))}[0-9]*" if rng.random() < 0.7 else names[j])
        rules.append(L.PortRuleHTTP(Path=f"/p{i % 7}/.*" if rng.random() < 0.8 else "",
                                    Method=["GET", "POST", ""][i % 3], Headers=hs))
    reqs = []
    for _ in range(3000):
        hs = []
        for _k in range(int(rng.integers(0, 7))):
            r = rng.random()
            if r < 0.7:
                hs.append((names[int(rng.integers(0, n_fields))], f"v{int(rng.integers(0, 5))}"))
            else:
                hs.append((f"y-h{int(rng.integers(0, 9))}", "v1"))
        reqs.append(L.HTTPRequest(["GET", "POST", "PUT"][int(rng.integers(0, 3))],
                                  f"/p{int(rng.integers(0, 9))}/{int(rng.integers(0, 100))}", "h", hs))
    arena, offs = L.pack_http(reqs)
    rd = _check(rules, arena, offs, 2, lds_budget_bytes=1)
    P = DenseHttpProgram(rd.program())
    nd = P.h["n_dfas"]
    assert (nd <= 4) == (n_fields == 1) and (nd > 8) == (n_fields == 8)
    assert P.dense_dfas == list(range(nd)) and P.dfas[nd]["kind"] == 0 and P.h["lds_name_tab"] == KNONE


def test_forced_captures_and_slow_pass(gpu):
    """Forced-capture back-references walk their R automaton (dense here) in
    the first pass; rules that keep the slow path are deferred on a dense
    superset automaton and decided by http_slow_kernel."""
    rng = np.random.default_rng(62)
    n_dense_r = n_slow = 0
    for trial in range(3):
        rules = X.dcap_rules(rng, int(rng.integers(6, 16)))
        if trial == 2:
            rules = rules + W.rules(2, n_rules=100)
        arena, offs = L.pack_http(X.dcap_requests(rng, 20_000))
        rd = _check(rules, arena, offs, 2, lds_budget_bytes=1)
        P = DenseHttpProgram(rd.program())
        n_dense_r += sum(1 for sp in P.dcaps if sp[3] != KNONE and P.dfas[sp[3]]["kind"] == DFA_DENSE)
        n_slow += P.h["n_slow"]
        assert P.dfas[1]["kind"] == DFA_DENSE
    assert n_dense_r > 0 and n_slow > 0


def test_extended_workload(gpu):
    """bench.py --extended's rule set, the workload the kind is for: the 50 k-
    state :path automaton (50 MB packed, 4 MB dense) and the :authority
    automaton are dense under L7M_OPT_DENSE_DFA."""
    rng = np.random.default_rng(42)
    rules = list(X.REALISTIC) + W.rules(2)
    a1, o1 = W.requests(2, 3_000_000, 50_000)
    a2, o2 = L.pack_http(X.realistic_requests(rng, 5000))
    arena = np.concatenate([a1[:-64], a2])
    offs = np.concatenate([o1, o2 + np.uint64(len(a1) - 64)])
    exp = HttpOracle(rules).eval(arena, offs, threads=8)
    assert {0, 1, 2, 8, 9} <= set(exp.tolist())
    assert L.VERDICT_UNSUPPORTED not in exp.tolist()
    rd = _check(rules, arena, offs, 1, exp=exp)
    assert rd.info.n_dense_dfas == 2


def test_policy_map_entry_point(gpu):
    pols = random_policies(11, n_policies=4)
    arena, offs = L.pack_http(random_requests(11, 20_000, n_policies=4))
    exp = PolicyOracle(pols).eval(arena, offs, threads=8)
    rd = L.RuleSet.compile_http_policies(pols, dense_dfa=2, lds_budget_bytes=1)
    rp = L.RuleSet.compile_http_policies(pols, lds_budget_bytes=1)
    assert rd.info.n_dense_dfas > 0 and rp.info.n_dense_dfas == 0
    for rs in (rd, rp):
        h = np.zeros(rs.n_counters, dtype=np.uint64)
        got = rs.eval(arena, offs, h)
        assert got.tolist() == exp.tolist()
        counted = int(((got >= 0) & (got < L.VERDICT_ALLOW_NO_PORT_POLICY)).sum()) + int((got == -1).sum())
        assert int(h.sum()) == counted


def test_batcher_entry_point(gpu):
    """l7m_batcher_eval_http from 8 threads on a dense rule set equals rs.eval."""
    rng = np.random.default_rng(12)
    rules = list(X.REALISTIC) + W.rules(2, n_rules=100)
    reqs = X.realistic_requests(rng, 400)
    arena, offs = L.pack_http(reqs)
    rs = L.RuleSet.compile_http(rules, dense_dfa=2, lds_budget_bytes=1)
    assert rs.info.n_dense_dfas > 0
    exp = rs.eval(arena, offs)
    assert exp.tolist() == HttpOracle(rules).eval(arena, offs, threads=8).tolist()
    b = L.Batcher(rs, max_delay_us=100, in_flight=3)
    got = np.full(len(reqs), -100, dtype=np.int64)

    def worker(t):
        for i in range(t, len(reqs), 8):  # 50 requests per thread
            got[i] = b.eval_http(reqs[i])

    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    b.close()
    assert got.tolist() == exp.tolist()


def test_ablation_launches_refuse_dense_programs(gpu):
    """The diagnostic ablations have no dense build: L7M_EDEVICE, as for
    search programs; the packed compile of the same rules still has one."""
    rules = W.rules(2, n_rules=40)
    arena, offs = W.requests(2, 0, 2000, n_rules=40)
    rd = L.RuleSet.compile_http(rules, dense_dfa=2, lds_budget_bytes=1)
    assert rd.info.n_dense_dfas > 0
    for flag in (L.FLAG_DIAG_WALK_ONLY, L.FLAG_DIAG_COPY_ONLY):
        with pytest.raises(L.L7Error) as e:
            rd.eval(arena, offs, flags=flag)
        assert e.value.code == L.L7M_EDEVICE
    L.RuleSet.compile_http(rules, lds_budget_bytes=1).eval(arena, offs, flags=L.FLAG_DIAG_WALK_ONLY)
    exp = HttpOracle(rules).eval(arena, offs, threads=8)
    assert rd.eval(arena, offs).tolist() == exp.tolist()  # and the dense program still evaluates
