"""CPU tests of the dense class-compressed DFA kind (program.h kDfaDense,
l7m_opts.flags L7M_OPT_DENSE_DFA): the host builder against the packed walk
(tests/cpp/fuzz_dense.cc under ASan/UBSan), the option's off state (programs
byte-identical to a compile without opts), the selection rule, and the
compiled programs -- read by tests/program_interp_dense.py the way the kernel
reads them -- against the CPU oracle.  No GPU calls."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import regex_ext_cases as X
from cilium_amd import l7match as L
from cilium_amd import workloads as W
from oracle import HttpOracle, PolicyOracle
from policy_cases import random_policies, random_requests
from program_interp import KNONE
from program_interp_dense import DFA_DENSE, DenseHttpProgram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("L7M_DENSE_DFA", raising=False)


def _compile_no_opts(rules):
    """l7m_compile_http with opts == NULL (what every caller before the option passes)."""
    keep = []
    arr = (L._HttpRule * max(1, len(rules)))(*[L._http_rule_struct(r, keep) for r in rules])
    out = ctypes.c_void_p()
    err = ctypes.create_string_buffer(1024)
    rc = L.lib().l7m_compile_http(arr, len(rules), None, ctypes.byref(out), err, 1024)
    assert rc == L.L7M_OK, err.value
    return L.RuleSet(out.value, L.PROTO_HTTP)


def _compile_policies_no_opts(pols):
    keep = []
    arr = L._policies_struct(pols, keep)
    out = ctypes.c_void_p()
    err = ctypes.create_string_buffer(1024)
    rc = L.lib().l7m_compile_http_policies(arr, len(pols), None, ctypes.byref(out), err, 1024)
    assert rc == L.L7M_OK, err.value
    return L.RuleSet(out.value, L.PROTO_HTTP)


@pytest.fixture(scope="module")
def extended():
    """bench.py --extended's rule set, compiled packed and dense (shared, read-only)."""
    rules = list(X.REALISTIC) + W.rules(2)
    os.environ.pop("L7M_DENSE_DFA", None)
    return rules, L.RuleSet.compile_http(rules), L.RuleSet.compile_http(rules, dense_dfa=L.OPT_DENSE_DFA)


def _same(a, b):
    pa, pb = a.program(), b.program()
    return pa.shape == pb.shape and bool((pa == pb).all())


# ------------------------------------------------------------ host builder --
def test_dense_builder_differential_fuzz(tmp_path):
    """tests/cpp/fuzz_dense.cc: build_field_dfa, build_dense, then
    dense_walk == packed_walk on random and pattern-derived subjects, under
    AddressSanitizer and UBSan (a stand-alone host program)."""
    exe = str(tmp_path / "l7m_fuzz_dense")
    csrc = os.path.join(ROOT, "cilium_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "fuzz_dense.cc"), os.path.join(csrc, "regex_ecma.cc"),
                           os.path.join(csrc, "dfa_pack.cc"), os.path.join(csrc, "regex_vm.cc")])
    for seed in ("5", "6"):
        out = subprocess.run(["timeout", "240", exe, seed, "60", "150"], capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
        assert "mismatches=0" in out.stdout


# --------------------------------------------------------------- option off --
def test_option_off_is_byte_identical(extended):
    rules, packed, _ = extended
    assert packed.info.n_dense_dfas == 0
    assert _same(packed, _compile_no_opts(rules))
    cfg2 = W.rules(2)
    assert _same(L.RuleSet.compile_http(cfg2, dense_dfa=0), _compile_no_opts(cfg2))
    pols = random_policies(3)
    assert _same(L.RuleSet.compile_http_policies(pols, dense_dfa=0), _compile_policies_no_opts(pols))


def test_option_on_changes_nothing_where_nothing_is_eligible():
    # config 2 at the default budget: every automaton is walked from LDS
    cfg2 = W.rules(2)
    for flag in (L.OPT_DENSE_DFA, L.OPT_DENSE_DFA_ALWAYS):
        rs = L.RuleSet.compile_http(cfg2, dense_dfa=flag)
        assert rs.info.n_dense_dfas == 0 and _same(rs, _compile_no_opts(cfg2))
    # the RE2 dialect never is, whatever the budget
    for rules in (cfg2[:60], list(W.rules(2, n_rules=40))):
        for flag in (L.OPT_DENSE_DFA, L.OPT_DENSE_DFA_ALWAYS):
            a = L.RuleSet.compile_http(rules, dialect=L.DIALECT_RE2_SEARCH, lds_budget_bytes=1, dense_dfa=flag)
            b = L.RuleSet.compile_http(rules, dialect=L.DIALECT_RE2_SEARCH, lds_budget_bytes=1)
            assert a.info.n_dense_dfas == 0 and _same(a, b)


@pytest.mark.parametrize("flag", [1, 2])
def test_environment_variable_is_the_flag(monkeypatch, flag):
    rules = W.rules(2, n_rules=40)
    want = L.RuleSet.compile_http(rules, lds_budget_bytes=1, dense_dfa=flag)
    assert want.info.n_dense_dfas > 0
    monkeypatch.setenv("L7M_DENSE_DFA", str(flag))
    got = L.RuleSet.compile_http(rules, lds_budget_bytes=1)
    assert got.info.n_dense_dfas == want.info.n_dense_dfas and _same(got, want)
    pols = random_policies(4)
    got = L.RuleSet.compile_http_policies(pols, lds_budget_bytes=1)
    monkeypatch.delenv("L7M_DENSE_DFA")  # read at each compile, not cached
    assert _same(got, L.RuleSet.compile_http_policies(pols, lds_budget_bytes=1, dense_dfa=flag))
    assert L.RuleSet.compile_http(rules, lds_budget_bytes=1).info.n_dense_dfas == 0


# ----------------------------------------------------------- selection rule --
def _groups(rs):
    """(descriptor index, field, kind, table bytes) of every automaton."""
    P = DenseHttpProgram(rs.program())
    return P, [(k, d["field"], d["kind"], (2 if d["kind"] == DFA_DENSE else 4) * d["n_slots"])
               for k, d in enumerate(P.dfas)]


def test_selection_rule_config2_walked_from_hbm():
    """Config 2's 400 rules with nothing in LDS.  Its path automaton is a
    prefix trie with one shared tail -- 7 KB packed, 63 KB dense -- so
    L7M_OPT_DENSE_DFA keeps it packed and ..._ALWAYS converts it with the other
    three value automata; the header-name automaton stays packed under both.
    Under L7M_OPT_DENSE_DFA a group is dense exactly when its u16 table is
    smaller than its slot table (the three small automata -- method 494 B
    against 2,904 B, authority 722 B against 1,268 B, the header value 120 B
    against 1,076 B -- are, by that rule)."""
    rules = W.rules(2, n_rules=400)
    _, packed = _groups(L.RuleSet.compile_http(rules, lds_budget_bytes=1))
    rs1 = L.RuleSet.compile_http(rules, lds_budget_bytes=1, dense_dfa=1)
    rs2 = L.RuleSet.compile_http(rules, lds_budget_bytes=1, dense_dfa=2)
    P1, g1 = _groups(rs1)
    P2, g2 = _groups(rs2)
    assert len(packed) == 5 and packed[4][1] == KNONE  # four value automata, then the name automaton
    # the measured case: the path trie stays packed under 1 (7 KB against 63 KB)
    assert g1[1][1] == 1 and g1[1][2] == 0 and g1[1][3] == packed[1][3] < 8 << 10
    assert g2[1][2] == DFA_DENSE and 60 << 10 < g2[1][3] < 66 << 10
    # 2 converts the four value automata, never the name automaton
    assert [g[2] for g in g2] == [DFA_DENSE] * 4 + [0] and rs2.info.n_dense_dfas == 4
    assert g1[4][2] == 0
    # 1 converts exactly the groups whose dense table is the smaller one
    for k in range(4):
        assert (g1[k][2] == DFA_DENSE) == (g2[k][3] < packed[k][3]), (k, g2[k][3], packed[k][3])
    assert rs1.info.n_dense_dfas == sum(g[2] == DFA_DENSE for g in g1)
    d = P2.dfas[1]
    assert d["region"] == 1 + 104 and d["nstates"] > 800  # dead, 104 multi-pattern states, then the latched ones


def test_selection_rule_too_many_states():
    rng = np.random.default_rng(5)
    al = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)
    rules = [L.PortRuleHTTP(Path="/" + bytes(rng.choice(al, 40)).decode()) for _ in range(2000)]
    for flag in (1, 2):
        rs = L.RuleSet.compile_http(rules, dense_dfa=flag)
        assert rs.info.n_dense_dfas == 0
        assert rs.info.total_dfa_states > 65535


def test_selection_rule_extended_set(extended):
    _, packed, dense = extended
    P, g = _groups(dense)
    assert dense.info.n_dense_dfas == 2
    by_field = {}
    for k, f, kind, nbytes in g:  # a field's value automata come first (forced-capture R automata last)
        by_field.setdefault(f, (k, kind, nbytes))
    assert by_field[1][1] == DFA_DENSE and by_field[2][1] == DFA_DENSE  # :path, :authority
    assert P.dfas[by_field[1][0]]["acc_ncls"] == 42 and P.dfas[by_field[2][0]]["acc_ncls"] == 20
    assert by_field[1][2] < 4.5e6
    assert packed.info.program_bytes - dense.info.program_bytes > 40e6
    for k in P.dense_dfas:  # the default budget has room for the class maps
        assert P.dfas[k]["lds_cmap"] != KNONE


# ------------------------------------------------------- interpreter parity --
def _interp_vs_oracle(rules, arena, offs, **kw):
    rs = L.RuleSet.compile_http(rules, **kw)
    got = DenseHttpProgram(rs.program()).eval(arena, offs)
    exp = HttpOracle(rules).eval(arena, offs)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, [(int(i), int(exp[i]), int(got[i])) for i in bad[:10]]
    return rs, exp


@pytest.mark.parametrize("backrefs", [False, True])
def test_interp_random_extended_rules(backrefs):
    rng = np.random.default_rng(70 + backrefs)
    n_dense = 0
    for trial in range(6):
        rules = X.random_rules(rng, int(rng.integers(1, 24)), backrefs=backrefs)
        arena, offs = L.pack_http(X.random_requests(rng, 300))
        rs, _ = _interp_vs_oracle(rules, arena, offs, dense_dfa=1 + trial % 2, lds_budget_bytes=1 if trial < 4 else 0)
        n_dense += rs.info.n_dense_dfas
    assert n_dense > 6


def test_interp_forced_captures():
    rng = np.random.default_rng(72)
    n_dense_r = 0
    for trial in range(4):
        rules = X.dcap_rules(rng, int(rng.integers(2, 12)))
        arena, offs = L.pack_http(X.dcap_requests(rng, 400))
        rs, exp = _interp_vs_oracle(rules, arena, offs, dense_dfa=2, lds_budget_bytes=1)
        P = DenseHttpProgram(rs.program())
        n_dense_r += sum(1 for sp in P.dcaps if sp[3] != KNONE and P.dfas[sp[3]]["kind"] == DFA_DENSE)
        assert (exp >= 0).any()
    assert n_dense_r > 0  # forced-capture R automata are dense too


@pytest.mark.parametrize("n_rules", [40, 400])
def test_interp_config2_like(n_rules):
    rules = W.rules(2, n_rules=n_rules)
    arena, offs = W.requests(2, 1000, 400, n_rules=n_rules)
    rs, exp = _interp_vs_oracle(rules, arena, offs, dense_dfa=2, lds_budget_bytes=1)
    assert rs.info.n_dense_dfas == 4 and (exp >= 0).any() and (exp < 0).any()


def test_interp_extended_set(extended):
    rules, _, dense = extended
    rng = np.random.default_rng(73)
    a1, o1 = W.requests(2, 2000, 200)
    a2, o2 = L.pack_http(X.realistic_requests(rng, 200))
    arena = np.concatenate([a1[:-64], a2])
    offs = np.concatenate([o1, o2 + np.uint64(len(a1) - 64)])
    got = DenseHttpProgram(dense.program()).eval(arena, offs)
    exp = HttpOracle(rules).eval(arena, offs)
    assert got.tolist() == exp.tolist()
    assert {0, 1, 2, 8, 9} <= set(exp.tolist())


def test_interp_policy_map():
    pols = random_policies(2)
    rs = L.RuleSet.compile_http_policies(pols, dense_dfa=2, lds_budget_bytes=1)
    assert rs.info.n_dense_dfas > 0
    arena, offs = L.pack_http(random_requests(2, 500))
    got = DenseHttpProgram(rs.program()).eval(arena, offs)
    exp = PolicyOracle(pols).eval(arena, offs)
    assert got.tolist() == exp.tolist()
    assert len(set(exp.tolist())) > 3
