"""GPU parity tests of the lean HTTP kernel's field tails and header directory
(l7m_http_impl.h: a field's last 1-3 bytes from one word read, the first
referenced header found by the validation pass).  As in test_http_lean_gpu.py
every rule set is evaluated by the lean kernel and, compiled under
L7M_HTTP_GENERIC=1, by the generic one; both must equal the CPU oracle bit for
bit, verdicts and per-rule counters, with hits on and off.  The cases and
their conditions: tests/lean_tail_cases.py."""
import numpy as np
import pytest
import torch

import lean_tail_cases as C
from cilium_amd import l7match as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exp():
    return C.expectations()


@pytest.fixture(scope="module")
def rulesets():
    """{family: (lean, generic)}, compiled once."""
    mp = pytest.MonkeyPatch()
    out = {}
    for fam, mk in C.FAMILY_RULES.items():
        lean = L.RuleSet.compile_http(mk())
        mp.setenv("L7M_HTTP_GENERIC", "1")
        generic = L.RuleSet.compile_http(mk())
        mp.delenv("L7M_HTTP_GENERIC")
        assert lean.http_lean and not generic.http_lean, fam
        out[fam] = (lean, generic)
    return out


def check(rs, arena, offs, exp, hits):
    h = np.zeros(rs.n_counters, dtype=np.uint64) if hits else None
    got = rs.eval(arena, offs, h)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, [(int(i), int(exp[i]), int(got[i])) for i in bad[:10]]
    if hits:
        assert np.array_equal(h, counters(rs, exp))


def counters(rs, exp):
    want = np.zeros(rs.n_counters, dtype=np.uint64)
    want[0] = (exp == L.VERDICT_DENY).sum()
    want[1] = (exp <= L.VERDICT_PARSE_ERROR).sum()
    np.add.at(want, 2 + exp[(exp >= 0) & (exp < L.VERDICT_ALLOW_NO_PORT_POLICY)], 1)
    return want


@pytest.mark.parametrize("fam", ["tails", "after", "directory"])
@pytest.mark.parametrize("hits", [False, True])
def test_shuffled_batch(gpu, exp, rulesets, fam, hits):
    """Tail x alignment, bytes after the end and the directory shapes, all in
    one seeded shuffled batch, under each family's rules."""
    (arena, offs, _), verdicts, _ = exp
    for rs in rulesets[fam]:
        check(rs, arena, offs, verdicts[fam], hits)


@pytest.mark.parametrize("n", C.CUTS)
def test_batch_cut_at_the_tile_edges(gpu, exp, rulesets, n):
    """The batch's first n records.  One workgroup's 16 waves share them, so
    the cuts up to 65 leave a wave a few records and the cuts at 16 x 55 ...
    16 x 65 give every wave exactly 55 ... 65: one tile, or 64 and one more."""
    (arena, offs, _), verdicts, _ = exp
    sub_arena, sub_offs = C.cut(arena, offs, n)
    for fam, both in rulesets.items():
        for rs in both:
            for hits in (False, True):
                check(rs, sub_arena, sub_offs, verdicts[fam][:n], hits)


@pytest.mark.parametrize("staged", [True, False])
def test_last_record_of_the_arena(gpu, exp, rulesets, staged):
    """The last field ends at the arena's end and the buffer, exactly
    round_up(arena_bytes, 16) bytes, goes on with bytes that would complete a
    longer literal; staged, and in the last wave's tile behind a record larger
    than the stage, where it is read from HBM (lean_tail_cases.expectations
    asserts which, from the kernel's partition of the batch).  A read past the
    field shows as a wrong verdict."""
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    cases = [c for c in exp[2] if c[4] == staged]
    assert len(cases) == 84  # 2 fields x 3 tails x (X, Y) x (4 "whole" + 3 "cut" ends)
    for rs, hits in [(rs, hits) for rs in rulesets["after"] for hits in (False, True)]:
        got, want = [], []
        dh = torch.zeros(rs.n_counters, dtype=torch.int64, device=dev) if hits else None
        total = np.zeros(rs.n_counters, dtype=np.uint64)
        for full, arena_bytes, offs, v, _, _ in cases:
            da = torch.from_numpy(full).to(dev)
            assert da.numel() == (arena_bytes + 15) & ~15
            do = torch.from_numpy(offs.view(np.int64)).to(dev)
            dv = torch.empty(len(offs), dtype=torch.int32, device=dev)
            rs.eval_device(da, arena_bytes, do, len(offs), dv, dh, stream)
            torch.cuda.synchronize()
            got.append(dv.cpu().numpy())
            want.append(v)
            total += counters(rs, v)
        bad = [(i, w.tolist(), g.tolist()) for i, (w, g) in enumerate(zip(want, got)) if not np.array_equal(w, g)]
        assert not bad, bad[:5]
        if hits:
            assert np.array_equal(dh.cpu().numpy().view(np.uint64), total)
