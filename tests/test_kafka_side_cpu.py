"""The Kafka deny responses and log records of a decided batch, from the host
side (no GPU): the request walk shared by host and device
(cilium_amd/csrc/l7m_kafka_side.h) through l7m_kafka_deny_response,
l7m_kafka_deny_responses and l7m_kafka_access_log, against responses and
records built from the cases' tuples (tests/kafka_side_cases.py), and the
argument checks of the two device entry points, which answer before any device
work."""
import ctypes

import numpy as np
import pytest

import kafka_side_cases as C
from cilium_amd import l7match as L


@pytest.fixture(scope="module")
def table():
    return C.table_cases()


@pytest.fixture(scope="module")
def both(table):
    return table + C.fuzz_cases()


def _batch(arena, offs, verdicts, cap=None, sizing=False, slack=0):
    """l7m_kafka_deny_responses -> (return value, resp_offs, output buffer of cap + slack bytes of 0xA5)."""
    n = len(verdicts)
    ro = np.full(n + 1, 2 ** 64 - 1, dtype=np.uint64)
    out = np.full(max(1, (cap or 0) + slack), 0xA5, dtype=np.uint8)
    rc = L.lib().l7m_kafka_deny_responses(arena.ctypes.data, arena.nbytes, offs.ctypes.data, n, verdicts.ctypes.data,
                                          None if sizing else out.ctypes.data, 0 if sizing else cap, ro.ctypes.data)
    return rc, ro, out


def test_table_covers_the_decoded_kinds_and_the_malformed_records(table):
    names = [c["name"] for c in C.TABLE]
    assert len(set(names)) == len(names) and len(table) == len(C.TABLE) * len(C.VERDICTS)
    assert {c["head"][0] for c in C.TABLE if c["head"]} == {0, 1, 2, 3, 8, 9, 10}
    assert sum(1 for c in C.TABLE if not c["resp"]) >= 8 and sum(1 for c in C.TABLE if c["bad"]) == 3
    assert max(len(c["req"]) for c in C.TABLE) > 70_000
    # responses end at every byte phase
    assert {len(c["resp"]) % 4 for c in C.TABLE if c["resp"]} == {0, 1, 2, 3}


@pytest.mark.parametrize("c", [c for c in C.TABLE if not c["bad"]], ids=lambda c: c["name"])
def test_table_response_equals_deny_response(c):
    if c["resp"]:
        assert L.kafka_deny_response(c["req"]) == c["resp"]
    else:
        with pytest.raises(L.L7Error) as e:
            L.kafka_deny_response(c["req"])
        assert e.value.code in (L.L7M_EINVAL, L.L7M_EUNSUPPORTED)


@pytest.mark.parametrize("pad", [True, False], ids=["packed", "unpadded"])
def test_batch_equals_the_table(table, pad):
    arena, offs, verdicts = C.build(table, pad)
    assert pad or int((offs % 2 == 1).sum()) > len(offs) // 4
    assert L.kafka_deny_responses(arena, offs, verdicts) == C.table_responses(table)
    recs, _ = C.host_log(arena, offs, verdicts)
    assert C.log_tuples(arena, recs) == C.table_log(table)
    assert not recs["pad"].any()


@pytest.mark.parametrize("pad", [True, False], ids=["packed", "unpadded"])
def test_batch_equals_the_per_request_function(both, pad):
    arena, offs, verdicts = C.build(both, pad)
    exp = C.single_responses(arena, offs, verdicts)
    assert L.kafka_deny_responses(arena, offs, verdicts) == exp
    assert any(exp[len(both) - 14000:]) and not all(exp)


def test_fuzz_share_of_non_empty_responses():
    """Between a quarter and three quarters of the fuzz requests get a non-empty response under the
    verdict vector, which every request meets entry by entry; tests/kafka_side_cases.py asserts the
    same when it builds the set.  Seeds 0-7 give 64.4-66.1 %; the set keeps seed 0 (65.65 %).  The
    unmutated generator alone gives 7 typed kinds in 9, above the upper bound."""
    share = C.fuzz_response_share()
    print(f"share of fuzz requests with a non-empty response: {share:.4f}")
    assert 0.25 <= share <= 0.75
    cases = C.fuzz_cases()
    assert len(cases) == 2000 * len(C.VERDICTS)
    assert [v for _, v in cases[:len(C.VERDICTS)]] == C.VERDICTS and cases[0][0] is cases[6][0]


def test_sizing_call_exact_cap_and_one_byte_short(both):
    arena, offs, verdicts = C.build(both, pad=False)
    exp = C.single_responses(arena, offs, verdicts)
    total = sum(map(len, exp))
    want = np.concatenate([[0], np.cumsum([len(e) for e in exp])]).astype(np.uint64)
    rc, ro, out = _batch(arena, offs, verdicts, sizing=True)
    assert rc == total and np.array_equal(ro, want) and np.all(out == 0xA5)
    rc, ro, out = _batch(arena, offs, verdicts, cap=total, slack=32)
    assert rc == total and np.array_equal(ro, want)
    assert out[:total].tobytes() == b"".join(exp)
    assert np.all(out[total:] == 0xA5)  # bytes past the total untouched
    rc, ro, out = _batch(arena, offs, verdicts, cap=total - 1, slack=32)
    assert rc == L.L7M_ENOMEM and np.array_equal(ro, want)
    last = max(i for i, e in enumerate(exp) if e)
    assert out[:int(want[last])].tobytes() == b"".join(exp[:last])  # the responses that still fit
    assert np.all(out[int(want[last]):] == 0xA5)


def test_empty_batch_and_argument_errors(table):
    arena, offs, verdicts = C.build(table[:14])
    f = L.lib().l7m_kafka_deny_responses
    assert f(None, 0, None, 0, None, None, 0, None) == 0
    ro = np.full(1, 7, dtype=np.uint64)
    assert f(arena.ctypes.data, arena.nbytes, offs.ctypes.data, 0, verdicts.ctypes.data, None, 0, ro.ctypes.data) == 0
    assert L.kafka_deny_responses(arena, offs[:0], verdicts[:0]) == []
    ro = np.zeros(15, dtype=np.uint64)
    args = [arena.ctypes.data, arena.nbytes, offs.ctypes.data, 14, verdicts.ctypes.data, None, 0, ro.ctypes.data]
    assert f(*args) > 0
    for k in (0, 2, 4, 7):  # arena, offsets, verdicts, resp_offs
        bad = list(args)
        bad[k] = None
        assert f(*bad) == L.L7M_EINVAL


# ---- the device entry points' argument checks ---------------------------------
FAKE = 0x10000  # a 16-byte aligned address that is never dereferenced: the checks come first


def _resp_device(arena=FAKE, n=4, offs=FAKE, verdicts=FAKE, out=FAKE, cap=64, resp_offs=FAKE, total=FAKE):
    return L.lib().l7m_kafka_deny_responses_device(arena, 1024, offs, n, verdicts, out, cap, resp_offs, total, None)


def _log_device(arena=FAKE, n=4, offs=FAKE, verdicts=FAKE, select=0, out=FAKE, cap=64, first=FAKE, total=FAKE):
    return L.lib().l7m_kafka_access_log_device(arena, 1024, offs, n, verdicts, select, out, cap, first, total, None)


@pytest.mark.parametrize("kw", [dict(arena=FAKE + 4), dict(arena=FAKE + 1), dict(arena=None), dict(offs=None),
                                dict(verdicts=None), dict(resp_offs=None), dict(total=None), dict(total=None, n=0),
                                dict(out=None)], ids=lambda kw: "-".join(kw))
def test_responses_device_argument_checks(kw):
    assert _resp_device(**kw) == L.L7M_EINVAL


@pytest.mark.parametrize("kw", [dict(arena=FAKE + 8), dict(arena=None), dict(offs=None), dict(verdicts=None),
                                dict(first=None), dict(total=None), dict(total=None, n=0), dict(out=None),
                                dict(out=FAKE + 4), dict(out=FAKE + 1), dict(select=4), dict(select=0x80000001)],
                         ids=lambda kw: "-".join(kw))
def test_log_device_argument_checks(kw):
    assert _log_device(**kw) == L.L7M_EINVAL


def test_device_calls_without_device_fail_loudly():
    if L.device_count() > 0:
        pytest.skip("GPU present")
    assert _resp_device() == L.L7M_EDEVICE
    assert _resp_device(out=FAKE + 3) == L.L7M_EDEVICE  # responses go to any address
    assert _log_device(select=3) == L.L7M_EDEVICE
    with pytest.raises(L.L7Error) as e:
        L.kafka_deny_responses_device(FAKE, 1024, FAKE, 4, FAKE, None, 0, FAKE, FAKE)
    assert e.value.code == L.L7M_EDEVICE
    with pytest.raises(L.L7Error) as e:
        L.kafka_access_log_device(FAKE, 1024, FAKE, 4, FAKE, None, 0, FAKE, FAKE, select=L.LOG_DENIED)
    assert e.value.code == L.L7M_EDEVICE


def test_record_layout_and_abi_version():
    assert L.KAFKA_LOG_RECORD_DTYPE.itemsize == ctypes.sizeof(L._KafkaLogRecord) == 40
    for name, _ in L._KafkaLogRecord._fields_:
        assert L.KAFKA_LOG_RECORD_DTYPE.fields[name][1] == getattr(L._KafkaLogRecord, name).offset
    assert L.lib().l7m_abi_version() == 4
