"""Verdict side effects of a Kafka batch that stays in device memory:
l7m_kafka_deny_responses_device and l7m_kafka_access_log_device must write,
byte for byte, what the host functions give (which
tests/test_kafka_side_cpu.py holds to responses and records built from the
cases' tuples), wherever the records lie and wherever the output starts."""
import numpy as np
import pytest

import kafka_side_cases as C
import kafka_wire as K
from cilium_amd import l7match as L
from cilium_amd import workloads as W

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
TILE = 256   # requests per workgroup tile (l7m_kafka_side.hip)
GUARD = 16   # sentinel bytes in front of the output
REC = L.KAFKA_LOG_RECORD_DTYPE.itemsize


def _to_device(arena, offs, verdicts):
    import torch
    d_arena = torch.zeros((arena.nbytes + 15) // 16 * 16 + 16, dtype=torch.uint8, device="cuda")
    d_arena[:arena.nbytes].copy_(torch.from_numpy(arena.copy()))
    d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64).copy()).cuda()
    d_verd = torch.from_numpy(np.ascontiguousarray(verdicts, dtype=np.int32).copy()).cuda()
    return d_arena, d_offs, d_verd


def _device(kind, arena, offs, verdicts, cap, shift=0, sizing=False, select=0):
    """kind "resp" (cap, shift in bytes) or "log" (cap in records) -> (output buffer incl. the
    sentinel bytes around d_out, offsets, total)."""
    import torch
    n = len(verdicts)
    unit = 1 if kind == "resp" else REC
    d_arena, d_offs, d_verd = _to_device(arena, offs, verdicts)
    d_buf = torch.full((GUARD + shift + cap * unit + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_eo = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    out = None if sizing else d_buf.data_ptr() + GUARD + shift
    stream = torch.cuda.current_stream().cuda_stream
    if kind == "resp":
        L.kafka_deny_responses_device(d_arena, arena.nbytes, d_offs, n, d_verd, out, 0 if sizing else cap, d_eo, d_total,
                                      stream)
    else:
        L.kafka_access_log_device(d_arena, arena.nbytes, d_offs, n, d_verd, out, 0 if sizing else cap, d_eo, d_total,
                                  stream, select=select)
    torch.cuda.synchronize()
    return d_buf.cpu().numpy(), d_eo.cpu().numpy().view(np.uint64), int(d_total.item())


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def _check_resp(arena, offs, verdicts, shift=0):
    exp = L.kafka_deny_responses(arena, offs, verdicts)
    total = sum(map(len, exp))
    buf, ro, got_total = _device("resp", arena, offs, verdicts, total, shift)
    assert got_total == total
    assert np.array_equal(ro, _offsets([len(e) for e in exp]))
    out = buf[GUARD + shift:].tobytes()
    bad = [i for i in range(len(exp)) if out[int(ro[i]):int(ro[i + 1])] != exp[i]]
    assert not bad, (len(bad), bad[:8])
    assert np.all(buf[:GUARD + shift] == SENTINEL)           # the byte before d_out
    assert np.all(buf[GUARD + shift + total:] == SENTINEL)   # every byte from the total onward
    return exp


def _check_log(arena, offs, verdicts, select=0):
    recs, first = C.host_log(arena, offs, verdicts, select)
    total = len(recs)
    buf, got_first, got_total = _device("log", arena, offs, verdicts, total, select=select)
    assert got_total == total
    assert np.array_equal(got_first, first)
    assert buf[GUARD:GUARD + total * REC].tobytes() == recs.tobytes()  # pad = 0 included
    assert np.all(buf[:GUARD] == SENTINEL)
    assert np.all(buf[GUARD + total * REC:] == SENTINEL)   # no record at or past the total
    return recs


def _check_both(arena, offs, verdicts, shift=0, select=0):
    return _check_resp(arena, offs, verdicts, shift), _check_log(arena, offs, verdicts, select)


@pytest.fixture(scope="module")
def table():
    cases = C.table_cases()
    return cases, C.build(cases)


@pytest.fixture(scope="module")
def fuzz():
    cases = C.fuzz_cases()
    return cases, C.build(cases)


def test_table_responses_match_host(gpu, table):
    cases, (arena, offs, verdicts) = table
    exp = _check_resp(arena, offs, verdicts)
    assert exp == C.table_responses(cases)
    assert any(exp) and not all(exp)


@pytest.mark.parametrize("select", [0, 1, 2, 3])
def test_table_log_matches_host(gpu, table, select):
    _, (arena, offs, verdicts) = table
    recs = _check_log(arena, offs, verdicts, select)
    assert set(recs["verdict"]) == {0: {0, 1}, 1: {0}, 2: {1}, 3: {0, 1}}[select]


def test_fuzz_responses_match_host(gpu, fuzz):
    _, (arena, offs, verdicts) = fuzz  # 2000 requests x 7 verdicts: 55 tiles, the last one partial
    exp = _check_resp(arena, offs, verdicts, shift=1)
    # two entries of the vector deny, and a quarter to three quarters of the requests have a response
    assert 2 * 2000 // 4 <= sum(1 for e in exp if e) <= 2 * 2000 * 3 // 4


@pytest.mark.parametrize("select", [0, 1, 2, 3])
def test_fuzz_log_matches_host(gpu, fuzz, select):
    _, (arena, offs, verdicts) = fuzz
    assert len(_check_log(arena, offs, verdicts, select)) > 100


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_batch_sizes_match_host(gpu, fuzz, n):
    _, (arena, offs, verdicts) = fuzz
    _check_both(arena, offs[100:100 + n], verdicts[100:100 + n], shift=n % 4)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_responses_at_any_alignment(gpu, fuzz, shift):
    _, (arena, offs, verdicts) = fuzz
    _check_resp(arena, offs[:700], verdicts[:700], shift=shift)


def test_unpadded_shuffled_repeated_and_descending_offsets_match_host(gpu, table, fuzz):
    """Records back to back (odd offsets), named in any order and several times."""
    both = table[0] + fuzz[0]
    arena, offs, verdicts = C.build(both, pad=False)
    assert int((offs % 2 == 1).sum()) > len(offs) // 4
    _check_both(arena, offs, verdicts, shift=3)
    rng = np.random.default_rng(3)
    pick = rng.integers(0, len(offs), 1500)
    pick[100:140] = pick[100]  # forty lanes of one tile on one record
    v = np.array([C.VERDICTS[k] for k in rng.integers(0, len(C.VERDICTS), len(pick))]).astype(np.uint32).view(np.int32)
    v[100:140] = L.VERDICT_DENY
    _check_both(arena, offs[pick], v, shift=2)
    order = np.arange(len(offs))[::-1].copy()  # descending: every record before its predecessor
    _check_both(arena, offs[order][:600], verdicts[order][:600], select=L.LOG_FORWARDED)


def _named(name):
    return next(c for c in C.TABLE if c["name"] == name)


def test_request_larger_than_any_stage_matches_host(gpu, fuzz):
    """The Produce with a 70,000-byte message set as the first and the last record of a tile and
    between small ones, denied and allowed."""
    big = _named("produce_70000_byte_message_set")
    small = fuzz[0]
    D, A = L.VERDICT_DENY, 0
    cases = ([(big, D)] + small[:TILE - 2] + [(big, A), (big, D)] + small[300:310] + [(big, D)] + small[400:420] +
             [(big, A)])
    assert cases[0][0] is big and cases[TILE - 1][0] is big and cases[TILE][0] is big
    for pad in (True, False):
        arena, offs, verdicts = C.build(cases, pad)
        exp, recs = _check_both(arena, offs, verdicts, shift=1)
        assert exp[0] == big["resp"] == exp[TILE] and exp[TILE - 1] == b""
        assert (recs["request"] == TILE - 1).sum() == 2


def test_300_topic_request_next_to_stubs_matches_host(gpu):
    many = _named("metadata_300_topics")
    stub = C.case("stub", C.with_correlation(K.metadata(0, "cc", []), 5), K.deny_response(K.METADATA, 0, 5, []),
                  (K.METADATA, 0, 5))
    assert len(stub["req"]) == 20
    cases = []
    for k in range(TILE + 40):
        cases.append((many if k % 50 == 7 else stub, [L.VERDICT_DENY, 0, L.VERDICT_DENY][k % 3]))
    arena, offs, verdicts = C.build(cases)
    exp, recs = _check_both(arena, offs, verdicts, shift=2)
    assert len(recs) == 300 * sum(1 for c, _ in cases if c is many)
    assert exp[57] == many["resp"] and exp[7] == b"" and exp[0] == stub["resp"]


def test_cap_one_short_leaves_the_output_untouched(gpu, fuzz):
    _, (arena, offs, verdicts) = fuzz
    exp = L.kafka_deny_responses(arena, offs, verdicts)
    total = sum(map(len, exp))
    for kw in (dict(cap=total - 1), dict(cap=total, sizing=True)):
        buf, ro, got_total = _device("resp", arena, offs, verdicts, shift=1, **kw)
        assert got_total == total
        assert np.array_equal(ro, _offsets([len(e) for e in exp]))
        assert np.all(buf == SENTINEL)
    recs, first = C.host_log(arena, offs, verdicts)
    for kw in (dict(cap=len(recs) - 1), dict(cap=len(recs), sizing=True)):
        buf, got_first, got_total = _device("log", arena, offs, verdicts, **kw)
        assert got_total == len(recs)
        assert np.array_equal(got_first, first)
        assert np.all(buf == SENTINEL)


def test_eval_responses_log_on_one_stream(gpu):
    """eval_device -> kafka_deny_responses_device -> kafka_access_log_device enqueued on one
    non-default stream with nothing between them equal the host chain on rs.eval's verdicts."""
    import torch
    rs = L.RuleSet.compile_kafka(W.rules(3, n_rules=2000))
    w_arena, w_offs = W.requests(3, 0, 4096, n_rules=2000)
    w_arena = w_arena[:w_arena.nbytes - 64]  # the generator's slack
    extra = [c["req"] for c in C.TABLE if c["resp"]]  # the table's well-formed cases
    x_arena, x_offs = L.pack_records(extra)
    base = (w_arena.nbytes + 3) & ~3
    arena = np.zeros(base + x_arena.nbytes, dtype=np.uint8)
    arena[:w_arena.nbytes] = w_arena
    arena[base:] = x_arena
    offs = np.concatenate([w_offs, x_offs + np.uint64(base)]).astype(np.uint64)
    n = len(offs)
    # the host chain
    h_verd = rs.eval(arena, offs)
    assert (h_verd == L.VERDICT_DENY).sum() > 100 and (h_verd >= 0).sum() > 100
    exp = L.kafka_deny_responses(arena, offs, h_verd)
    total = sum(map(len, exp))
    recs, first = C.host_log(arena, offs, h_verd)
    assert total and len(recs)

    d_arena, d_offs, _ = _to_device(arena, offs, h_verd)
    d_verd = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
    d_out = torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ro = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    d_recs = torch.full(((len(recs) + 2) * REC,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_first = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_nrec = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    rs.eval_device(d_arena, arena.nbytes, d_offs, n, d_verd, None, s.cuda_stream)
    L.kafka_deny_responses_device(d_arena, arena.nbytes, d_offs, n, d_verd, d_out, total, d_ro, d_total, s.cuda_stream)
    L.kafka_access_log_device(d_arena, arena.nbytes, d_offs, n, d_verd, d_recs, len(recs), d_first, d_nrec,
                              s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d_verd.cpu().numpy(), h_verd)
    assert int(d_total.item()) == total and int(d_nrec.item()) == len(recs)
    ro = d_ro.cpu().numpy().view(np.uint64)
    out = d_out.cpu().numpy()
    raw = out.tobytes()
    assert [raw[int(ro[i]):int(ro[i + 1])] for i in range(n)] == exp
    assert np.all(out[total:] == SENTINEL)
    assert np.array_equal(d_first.cpu().numpy().view(np.uint64), first)
    got = d_recs.cpu().numpy()
    assert got[:len(recs) * REC].tobytes() == recs.tobytes()
    assert np.all(got[len(recs) * REC:] == SENTINEL)
