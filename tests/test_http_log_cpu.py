"""The HttpLogEntry serialisation shared by the host function and the device
encoder (cilium_amd/csrc/l7m_http_log.h), from the host side (no GPU): the
host function against an independent encoder that works from the cases'
fields (tests/http_log_cases.py expected_entry), the host statistics against a
count of the same fields, and the argument checks of the two device entry
points, which answer before any device work."""
import ctypes

import pytest

import http_log_cases as C
from cilium_amd import l7match as L


@pytest.fixture(scope="module")
def table():
    cases = C.table_cases()
    return cases, C.build(cases)


@pytest.fixture(scope="module")
def fuzz():
    cases = C.fuzz_cases()
    return cases, C.build(cases)


def test_table_holds_malformed_and_well_formed_records(table):
    cases, (arena, offs, verdicts) = table
    assert len(cases) == len(C.TABLE) * len(C.VERDICTS)
    assert len({name for name, _ in C.TABLE}) == len(C.TABLE)
    assert sum(1 for f, _ in cases if f["bad"]) >= 10 * len(C.VERDICTS)
    assert arena.shape[0] % 4 == 0 and int(offs.max()) == 2 ** 63


def test_packer_and_struct_write_the_same_record():
    for name, f in C.TABLE:
        if not f["bad"] and not f["raw"]:
            assert C.record(f) == C.raw_record(f), name


@pytest.mark.parametrize("opts", C.OPTS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items())[:40] or "defaults")
def test_host_log_equals_independent_encoder_on_the_table(table, opts):
    cases, (arena, offs, verdicts) = table
    got = L.http_access_log(arena, offs, verdicts, **opts)
    exp = [C.expected_entry(f, v, **opts) for f, v in cases]
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (C.TABLE[i // len(C.VERDICTS)][0], cases[i][1])
    assert any(exp) and not all(exp)


def test_host_log_equals_independent_encoder_on_the_fuzz_set(fuzz):
    cases, (arena, offs, verdicts) = fuzz
    for opts in (C.OPTS[0], C.ALL_STRINGS):
        assert L.http_access_log(arena, offs, verdicts, **opts) == [C.expected_entry(f, v, **opts) for f, v in cases]
    bad = sum(1 for f, _ in cases if f["bad"])
    assert 0.03 * len(cases) < bad < 0.08 * len(cases)


def test_known_entries():
    f = C.fields(headers=[(b"", b"")], remote_id=0)
    assert C.expected_entry(f, 0) == bytes.fromhex("1001" "5a012f" "6203474554" "7200" "7801")
    assert C.expected_entry(f, -1) == bytes.fromhex("1001" "1802" "5a012f" "6203474554" "689303" "7200" "7801")
    arena, offs, v = C.build([(f, 0), (f, -1)])
    assert L.http_access_log(arena, offs, v) == [C.expected_entry(f, 0), C.expected_entry(f, -1)]


def test_host_stats_equal_a_count_of_the_fields(table, fuzz):
    t = L.ProxyStatsTable()
    for cases, (arena, offs, verdicts) in (table, fuzz):
        t.update(L.PROTO_HTTP, arena, offs, verdicts, port=4242, ingress=False)
    both = table[0] + fuzz[0]
    assert t.entries() == C.expected_stats(both, 4242, False)


def test_host_log_accepts_strings_longer_than_255(table):
    cases, (arena, offs, verdicts) = table
    long = "p" * 300
    got = L.http_access_log(arena[:64], offs[:1], verdicts[:1], policy_name=long)
    assert got == [C.expected_entry(cases[0][0], cases[0][1], policy_name=long)]


# ---- the device entry points' argument checks ---------------------------------
FAKE = 0x10000  # a 16-byte aligned address that is never dereferenced: the checks come first


def _log_device(arena=FAKE, n=4, offs=FAKE, verdicts=FAKE, out=FAKE, cap=64, entry_offs=FAKE, total=FAKE, select=0,
                **opts):
    o = L._AccessLogOpts(ctypes.sizeof(L._AccessLogOpts), 1, 0, L._b(opts.get("policy_name", "")), 0, 0,
                         L._b(opts.get("source_address")), L._b(opts.get("destination_address")))
    return L.lib().l7m_http_access_log_device(arena, 1024, offs, n, verdicts, ctypes.byref(o), select, out, cap,
                                              entry_offs, total, None)


def _stats_device(t, proto=L.PROTO_HTTP, arena=FAKE, offs=FAKE, verdicts=FAKE, n=4):
    return L.lib().l7m_proxy_stats_update_device(t._h, proto, arena, 1024, offs, verdicts, n, 80, 1, None)


@pytest.mark.parametrize("kw", [dict(arena=FAKE + 4), dict(arena=FAKE + 1), dict(arena=None), dict(offs=None),
                                dict(verdicts=None), dict(entry_offs=None), dict(total=None), dict(total=None, n=0),
                                dict(out=None), dict(select=4), dict(policy_name="p" * 256),
                                dict(source_address="s" * 256), dict(destination_address="d" * 256)],
                         ids=lambda kw: "-".join(kw))
def test_log_device_argument_checks(kw):
    assert _log_device(**kw) == L.L7M_EINVAL


@pytest.mark.parametrize("kw", [dict(proto=L.PROTO_KAFKA), dict(proto=0), dict(arena=FAKE + 8), dict(arena=None),
                                dict(offs=None), dict(verdicts=None)], ids=lambda kw: "-".join(kw))
def test_stats_device_argument_checks(kw):
    t = L.ProxyStatsTable()
    assert _stats_device(t, **kw) == L.L7M_EINVAL
    assert L.lib().l7m_proxy_stats_update_device(None, L.PROTO_HTTP, FAKE, 1024, FAKE, FAKE, 4, 80, 1, None) == L.L7M_EINVAL
    assert t.entries() == {}


def test_device_calls_without_device_fail_loudly():
    if L.device_count() > 0:
        pytest.skip("GPU present")
    assert _log_device() == L.L7M_EDEVICE
    assert _log_device(policy_name="p" * 255) == L.L7M_EDEVICE  # 255 bytes pass the check
    t = L.ProxyStatsTable()
    assert _stats_device(t) == L.L7M_EDEVICE
    assert t.entries() == {}
    with pytest.raises(L.L7Error) as e:
        L.http_access_log_device(FAKE, 1024, FAKE, 4, FAKE, None, 0, FAKE, FAKE, select=L.LOG_DENIED)
    assert e.value.code == L.L7M_EDEVICE
    with pytest.raises(L.L7Error) as e:
        t.update_device(L.PROTO_HTTP, FAKE, 1024, FAKE, FAKE, 4)
    assert e.value.code == L.L7M_EDEVICE


def test_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "l7match.h")).read()
    assert int(re.search(r"#define L7M_LOG_FORWARDED (\d+)u", hdr).group(1)) == L.LOG_FORWARDED
    assert int(re.search(r"#define L7M_LOG_DENIED\s+(\d+)u", hdr).group(1)) == L.LOG_DENIED
    assert L.lib().l7m_abi_version() == 4
