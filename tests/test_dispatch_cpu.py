"""CPU test of the launchers' value-to-template dispatcher
(cilium_amd/csrc/l7m_dispatch.h): tests/cpp/dispatch_test.cc, a stand-alone
host program built with plain g++ under AddressSanitizer and UBSan.  No GPU
calls."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_values(tmp_path):
    """Every listed value of the launchers' lists (hit modes, end-code
    registers, slow-pass tiers, Kafka's two bools, the resident kind) reaches
    the lambda as its own constant exactly once, nested dispatch covers the
    3 x 3, 3 x 2 x 2 and 3 x 2 products cell by cell, and an unlisted value
    returns the fallback without a call."""
    exe = str(tmp_path / "l7m_dispatch_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "dispatch_test.cc")])
    out = subprocess.run(["timeout", "60", exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert "failures=0" in out.stdout
