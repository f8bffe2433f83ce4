"""GPU parity tests of the lean HTTP kernel's walk jobs and verification phase
(l7m_http_impl.h: jobs 0-2 from the wave's scalars outside the job loop, the
header jobs behind them, the verification that follows).  As in
test_http_lean_tails_gpu.py every rule set is evaluated as compiled, by the
lean kernel, and, compiled under L7M_HTTP_GENERIC=1, by the generic kernel; both
must equal the CPU oracle bit for bit, verdicts and per-rule counters, with
hits on and off.  The cases and their conditions: tests/lean_job_cases.py."""
import numpy as np
import pytest

import lean_job_cases as C
from cilium_amd import l7match as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exp():
    return C.expectations()


@pytest.fixture(scope="module")
def rulesets():
    """{family: (as compiled, generic)}, compiled once."""
    mp = pytest.MonkeyPatch()
    out = {}
    for fam, mk in C.FAMILY_RULES.items():
        plain = L.RuleSet.compile_http(mk())
        mp.setenv("L7M_HTTP_GENERIC", "1")
        generic = L.RuleSet.compile_http(mk())
        mp.delenv("L7M_HTTP_GENERIC")
        assert plain.http_lean == (fam not in C.GENERIC) and not generic.http_lean, fam
        out[fam] = (plain, generic)
    return out


def counters(rs, exp):
    want = np.zeros(rs.n_counters, dtype=np.uint64)
    want[0] = (exp == L.VERDICT_DENY).sum()
    want[1] = (exp <= L.VERDICT_PARSE_ERROR).sum()
    np.add.at(want, 2 + exp[(exp >= 0) & (exp < L.VERDICT_ALLOW_NO_PORT_POLICY)], 1)
    return want


def check(rs, arena, offs, exp, hits):
    h = np.zeros(rs.n_counters, dtype=np.uint64) if hits else None
    got = rs.eval(arena, offs, h)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, [(int(i), int(exp[i]), int(got[i])) for i in bad[:10]]
    if hits:
        assert np.array_equal(h, counters(rs, exp))


@pytest.mark.parametrize("fam", list(C.FAMILY_RULES))
@pytest.mark.parametrize("hits", [False, True])
def test_shuffled_batch(gpu, exp, rulesets, fam, hits):
    """Every family's records in one seeded shuffled batch, under each family's rules."""
    (arena, offs, _), verdicts = exp
    for rs in rulesets[fam]:
        check(rs, arena, offs, verdicts[fam], hits)


@pytest.mark.parametrize("n", C.CUTS)
def test_batch_cut_at_the_tile_edges(gpu, exp, rulesets, n):
    """The batch's first n records.  One workgroup's 16 waves share them, so
    the cuts up to 65 leave a wave a few records and the cuts at 16 x 55 ...
    16 x 65 give every wave exactly 55 ... 65: one tile, or 64 and one more."""
    (arena, offs, _), verdicts = exp
    sub_arena, sub_offs = C.cut(arena, offs, n)
    for fam, both in rulesets.items():
        for rs in both:
            for hits in (False, True):
                check(rs, sub_arena, sub_offs, verdicts[fam][:n], hits)


def test_32_and_33_fields_give_the_same_verdicts(gpu, exp, rulesets):
    """The same verdicts but for the requests only the 33rd field's rule allows."""
    (arena, offs, _), verdicts = exp
    a, b = rulesets["f32"][0].eval(arena, offs), rulesets["f33"][0].eval(arena, offs)
    assert np.array_equal(a, np.where(b == 30, L.VERDICT_DENY, b))
