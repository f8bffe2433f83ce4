"""GPU parity tests of the lean HTTP kernel's held verdict stores, its header
jobs and its inline matchers decided from the candidate entry
(l7m_http_impl.h).  As in test_http_lean_jobs_gpu.py every rule
set is evaluated as compiled, by the lean kernel, and, compiled under
L7M_HTTP_GENERIC=1, by the generic kernel; both must equal the CPU oracle bit
for bit, verdicts and per-rule counters, with hits on and off.  The cases and
their conditions: tests/lean_verify_cases.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import lean_verify_cases as C
from cilium_amd import l7match as L
from program_interp import HttpProgram

pytestmark = pytest.mark.gpu

GUARD = 96           # int32 guard elements on either side of the verdict buffer
GUARD_VALUE = -777   # no verdict has this value
# one tile per wave, 64 records and one more (two tiles, the last of one record), two full tiles
CUTS = C.CUTS + (16 * 128,)


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
        assert plain.http_lean and not generic.http_lean, fam
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


@pytest.mark.parametrize("n", CUTS)
def test_batch_cut_at_the_tile_edges(gpu, exp, rulesets, n):
    """The batch's first n records: one workgroup's 16 waves share them, so a
    wave has one tile, 64 records and one more, or two full tiles."""
    (arena, offs, _), verdicts = exp
    assert n <= len(offs)
    sub_arena, sub_offs = C.cut(arena, offs, n)
    for fam, both in rulesets.items():
        for rs in both:
            for hits in (False, True):
                check(rs, sub_arena, sub_offs, verdicts[fam][:n], hits)


def test_the_33_set_program_keeps_the_mask_rounds(gpu, rulesets):
    """33 sets: the program does not say kHttpInlineMasks, and the lean kernel
    (still its kernel) decides the inline matchers by the mask-table rounds."""
    for fam, want in C.INLINE_MASKS.items():
        rs = rulesets[fam][0]
        assert rs.http_lean
        assert bool(HttpProgram(rs.program()).h["single_entry"] & 2) == want, fam


def eval_guarded(rs, arena, offs, hits):
    """Verdicts of a device launch whose verdict buffer lies between guard elements; asserts the guards."""
    dev = torch.device("cuda:0")
    full = np.zeros((arena.nbytes + 15) & ~15, dtype=np.uint8)
    full[:arena.nbytes] = arena
    da = torch.from_numpy(full).to(dev)
    do = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).to(dev)
    n = len(offs)
    buf = torch.full((GUARD + n + GUARD,), GUARD_VALUE, dtype=torch.int32, device=dev)
    dh = torch.zeros(rs.n_counters, dtype=torch.int64, device=dev) if hits else None
    rs.eval_device(da, arena.nbytes, do, n, buf[GUARD:GUARD + n], dh, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:GUARD] == GUARD_VALUE).all() and (out[GUARD + n:] == GUARD_VALUE).all()
    return out[GUARD:GUARD + n], (dh.cpu().numpy().view(np.uint64) if hits else None)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 16 * 64, 16 * 65, 16 * 128])
@pytest.mark.parametrize("hits", [False, True])
def test_verdict_buffer_between_guards(gpu, exp, rulesets, n, hits):
    """Every verdict of the batch is stored, the held last tile's too, and nothing around them."""
    (arena, offs, _), verdicts = exp
    sub_arena, sub_offs = C.cut(arena, offs, n)
    for fam in ("among", "codes"):
        rs = rulesets[fam][0]
        got, h = eval_guarded(rs, sub_arena, sub_offs, hits)
        assert np.array_equal(got, verdicts[fam][:n]), fam
        if hits:
            assert np.array_equal(h, counters(rs, verdicts[fam][:n]))


@pytest.mark.parametrize("n", [1, 64, 65, 16 * 65 + 3])
def test_batch_of_parse_errors(gpu, rulesets, n):
    """No record reaches verification; the stores still happen, between untouched guards."""
    arena, offs = C.error_batch(n)
    want = np.full(n, L.VERDICT_PARSE_ERROR, dtype=np.int32)
    for rs in rulesets["codes"]:
        for hits in (False, True):
            check(rs, arena, offs, want, hits)
    got, h = eval_guarded(rulesets["codes"][0], arena, offs, True)
    assert np.array_equal(got, want) and np.array_equal(h, counters(rulesets["codes"][0], want))


def test_batcher_calls(gpu, exp, rulesets):
    """Single requests and batches of <= 64 through a batcher (the lean no-hits
    kernel with a DoneSignal, the speculative tile): the verdict is there when
    the completion flag is."""
    (arena, offs, where), verdicts = exp
    ends = np.append(offs[1:], np.uint64(arena.nbytes))
    for fam in ("among", "inline"):
        idx = where[C.RECORDS_OF.get(fam, fam)][:192]
        recs = [bytes(arena[int(offs[i]):int(ends[i])]) for i in idx]
        want = verdicts[fam][idx].tolist()
        b = L.Batcher(rulesets[fam][0], max_batch=64, max_delay_us=200)
        try:
            assert [b.eval(r) for r in recs[:48]] == want[:48]          # one caller: batches of one
            with ThreadPoolExecutor(32) as pool:                        # 32 callers: batches of up to 32
                assert list(pool.map(b.eval, recs)) == want
        finally:
            b.close()
