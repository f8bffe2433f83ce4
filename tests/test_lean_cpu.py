"""CPU tests of the lean class of HTTP programs (cilium_amd/csrc/l7m_dispatch.h
http_program_lean): tests/cpp/lean_test.cc, a stand-alone host program built
with plain g++ under AddressSanitizer and UBSan, and the query function on
compiled rule sets.  No GPU calls."""
import os
import subprocess
import sys

from cilium_amd import l7match as L
from cilium_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lean_predicate_clauses(tmp_path):
    """One synthetic program passes every clause; one per clause differs in
    that clause alone and is not lean."""
    exe = str(tmp_path / "l7m_lean_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "lean_test.cc")])
    out = subprocess.run(["timeout", "60", exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert "failures=0" in out.stdout


def test_config2_is_lean_and_others_are_not():
    """The flagship rule set (config 2, 1k rules) runs lean; the rule sets of
    the other classes do not."""
    assert L.RuleSet.compile_http(W.rules(2)).http_lean
    assert L.RuleSet.compile_http(W.rules(2, n_rules=50)).http_lean
    assert not L.RuleSet.compile_http(W.rules(2), dialect=L.DIALECT_RE2_SEARCH).http_lean
    assert not L.RuleSet.compile_http(W.rules(2), lds_budget_bytes=1024).http_lean
    assert not L.RuleSet.compile_http([]).http_lean  # allow_no_l7
    assert not L.RuleSet.compile_http(W.EXTENDED_RULES + W.rules(2, n_rules=50)).http_lean  # slow-path rules
    assert not L.RuleSet.compile_kafka(W.rules(3, n_rules=10)).http_lean


def test_environment_switch_forces_the_generic_kernels():
    """L7M_HTTP_GENERIC=1, read when a rule set is created, keeps it off the lean kernels."""
    code = ("from cilium_amd import l7match as L, workloads as W; "
            "print(int(L.RuleSet.compile_http(W.rules(2, n_rules=50)).http_lean))")
    for val, want in (("1", "0"), ("0", "1"), ("", "1")):
        env = dict(os.environ, L7M_HTTP_GENERIC=val, PYTHONPATH=ROOT)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip().splitlines()[-1] == want, (val, out.stdout)
