"""Verdict side effects of an HTTP batch that stays in device memory:
l7m_http_access_log_device must write, byte for byte, the entries of the host
function (which tests/test_http_log_cpu.py holds to an independent encoder)
wherever the output buffer starts, and l7m_proxy_stats_update_device must
leave a table as l7m_proxy_stats_update does."""
import numpy as np
import pytest

import http_log_cases as C
import http_wire_cases as W
import kafka_wire as K
from cilium_amd import l7match as L

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
TILE = 256         # requests per workgroup tile (l7m_http_log.hip kLogTile)
STAGE = 64 * 1024  # arena bytes a tile stages at once (kLogStage)
GUARD = 16         # sentinel bytes in front of the output


def _to_device(arena, offs, verdicts):
    import torch
    d_arena = torch.zeros((arena.nbytes + 15) // 16 * 16 + 16, dtype=torch.uint8, device="cuda")
    d_arena[:arena.nbytes].copy_(torch.from_numpy(arena.copy()))
    d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64).copy()).cuda()
    d_verd = torch.from_numpy(np.ascontiguousarray(verdicts, dtype=np.int32).copy()).cuda()
    return d_arena, d_offs, d_verd


def _device_log(arena, offs, verdicts, cap, select=0, shift=0, sizing=False, **opts):
    """-> (output buffer incl. the sentinel bytes around d_out, entry_offs, total)."""
    import torch
    n = len(verdicts)
    d_arena, d_offs, d_verd = _to_device(arena, offs, verdicts)
    d_buf = torch.full((GUARD + shift + cap + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_eo = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.http_access_log_device(d_arena, arena.nbytes, d_offs, n, d_verd, None if sizing else d_buf.data_ptr() + GUARD + shift,
                             0 if sizing else cap, d_eo, d_total, torch.cuda.current_stream().cuda_stream,
                             select=select, **opts)
    torch.cuda.synchronize()
    return d_buf.cpu().numpy(), d_eo.cpu().numpy().view(np.uint64), int(d_total.item())


def _host_entries(arena, offs, verdicts, select=0, **opts):
    entries = L.http_access_log(arena, offs, verdicts, **opts)
    if select:
        keep = ((verdicts >= 0) & bool(select & L.LOG_FORWARDED)) | ((verdicts == -1) & bool(select & L.LOG_DENIED))
        entries = [e if k else b"" for e, k in zip(entries, keep)]
    return entries


def _check_equals_host(arena, offs, verdicts, select=0, shift=0, **opts):
    exp = _host_entries(arena, offs, verdicts, select, **opts)
    total = sum(map(len, exp))
    buf, eo, got_total = _device_log(arena, offs, verdicts, total, select, shift, **opts)
    assert got_total == total
    assert np.array_equal(eo, np.concatenate([[0], np.cumsum([len(e) for e in exp])]).astype(np.uint64))
    out = buf[GUARD + shift:].tobytes()
    got = [out[int(eo[i]):int(eo[i + 1])] for i in range(len(exp))]
    bad = [i for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (len(bad), bad[:8])
    assert np.all(buf[:GUARD + shift] == SENTINEL)           # the byte before d_out
    assert np.all(buf[GUARD + shift + total:] == SENTINEL)   # every byte from the total onward
    return exp


@pytest.fixture(scope="module")
def table():
    cases = C.table_cases()
    return cases, C.build(cases)


@pytest.fixture(scope="module")
def fuzz():
    cases = C.fuzz_cases()
    return cases, C.build(cases)


@pytest.mark.parametrize("select", [0, 1, 2, 3])
def test_table_matches_host(gpu, table, select):
    _, (arena, offs, verdicts) = table
    for opts in C.OPTS if select == 0 else [C.ALL_STRINGS]:
        exp = _check_equals_host(arena, offs, verdicts, select, **opts)
        assert any(exp) and not all(exp)


@pytest.mark.parametrize("select", [0, 1, 2, 3])
def test_fuzz_matches_host(gpu, fuzz, select):
    _, (arena, offs, verdicts) = fuzz  # 2000 records: eight tiles, the last one partial
    exp = _check_equals_host(arena, offs, verdicts, select, **C.ALL_STRINGS)
    if select == L.LOG_DENIED:
        assert 0 < sum(1 for e in exp if e) < 600


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_batch_sizes_match_host(gpu, fuzz, n):
    _, (arena, offs, verdicts) = fuzz
    _check_equals_host(arena, offs[100:100 + n], verdicts[100:100 + n], shift=n % 4, **C.ALL_STRINGS)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_output_at_any_alignment(gpu, fuzz, shift):
    _, (arena, offs, verdicts) = fuzz
    _check_equals_host(arena, offs[:700], verdicts[:700], shift=shift, policy_name="p" * 255)


def _sized(k, size, verdict=0):
    """A case whose record takes exactly `size` bytes: values of up to 1000 bytes."""
    hdrs, left = [], size - L.HTTP_REC_FIXED - len(b"POST") - len(b"/big/%d" % k)
    while left:  # a header takes 4 bytes of directory, 3 of name and its value
        take = min(left, 1007)
        if 0 < left - take < 7:
            take -= 7
        hdrs.append((b"x-b", bytes([97 + (k + len(hdrs)) % 26]) * (take - 7)))
        left -= take
    f = C.fields(b"POST", b"/big/%d" % k, None, hdrs, remote_id=k, raw=True)
    assert len(C.record(f)) == size
    return f, verdict


def test_records_larger_than_the_stage_match_host(gpu, fuzz):
    """Records above the stage (read from global memory) as the first and the last record of a
    tile and between ordinary ones."""
    small = [c for c in fuzz[0] if not c[0]["bad"]]
    cases = ([_sized(0, STAGE + 3000)] + small[:TILE - 2] + [_sized(1, 100000, -1), _sized(2, STAGE + 4)] +
             small[300:310] + [_sized(3, STAGE + 5000, -1)])
    arena, offs, verdicts = C.build(cases)
    for i in (0, TILE - 1, TILE, len(cases) - 1):
        assert int(np.frombuffer(arena[int(offs[i]):int(offs[i]) + 4].tobytes(), dtype=np.uint32)[0]) > STAGE
    for select in (0, L.LOG_DENIED):
        _check_equals_host(arena, offs, verdicts, select, shift=1, **C.ALL_STRINGS)


def test_run_of_near_stage_size_records_matches_host(gpu, fuzz):
    """Records that fit the stage one or two at a time: the tile takes many windows."""
    small = [c for c in fuzz[0] if not c[0]["bad"]]
    cases = small[:5]
    cases += [_sized(k, STAGE - 2500) for k in range(4)]           # one per window
    cases += [_sized(10 + k, STAGE // 2 - 2000, -1) for k in range(6)]  # two per window
    # the window starts at a 16-byte boundary of the arena: whether the largest two are staged
    # or read from global memory depends on where they start
    cases += small[5:40] + [_sized(20, STAGE - 16), _sized(21, STAGE - 12)] + small[40:60]
    arena, offs, verdicts = C.build(cases)
    _check_equals_host(arena, offs, verdicts, shift=3, **C.ALL_STRINGS)


def test_shuffled_and_repeated_offsets_match_host(gpu, fuzz):
    """Offsets in any order, some records named several times: more windows, the same entries."""
    _, (arena, offs, verdicts) = fuzz
    rng = np.random.default_rng(3)
    pick = rng.integers(0, len(offs), 1500)
    pick[100:140] = pick[100]  # forty lanes of one tile on one record
    v = np.array([C.VERDICTS[k] for k in rng.integers(0, len(C.VERDICTS), len(pick))]).astype(np.uint32).view(np.int32)
    _check_equals_host(arena, offs[pick], v, shift=2, **C.ALL_STRINGS)
    order = np.arange(len(offs))[::-1].copy()  # descending: every record before its predecessor
    _check_equals_host(arena, offs[order][:600], verdicts[order][:600], select=L.LOG_FORWARDED)


def test_cap_one_byte_short_leaves_the_output_untouched(gpu, fuzz):
    _, (arena, offs, verdicts) = fuzz
    exp = _host_entries(arena, offs, verdicts, **C.ALL_STRINGS)
    total = sum(map(len, exp))
    want_eo = np.concatenate([[0], np.cumsum([len(e) for e in exp])]).astype(np.uint64)
    for kw in (dict(cap=total - 1), dict(cap=total, sizing=True)):
        buf, eo, got_total = _device_log(arena, offs, verdicts, shift=1, **kw, **C.ALL_STRINGS)
        assert got_total == total
        assert np.array_equal(eo, want_eo)
        assert np.all(buf == SENTINEL)


RULES = [
    L.PortRuleHTTP(Path="/api/v[0-9]+/.*", Method="GET"),
    L.PortRuleHTTP(Method="PUT|POST", Host="svc-1[0-9]?\\.example\\.com"),
    L.PortRuleHTTP(Path="/public/.*", Headers=["X-Token: secret"]),
]


def _e2e_heads():
    rng = np.random.default_rng(17)
    heads = list(W.fuzz_heads()[:500])  # refused heads among them
    for i in range(600):
        method = [b"GET", b"PUT", b"POST"][int(rng.integers(0, 3))]
        path = [b"/api/v%d/x" % int(rng.integers(0, 30)), b"/public/a", b"/private"][int(rng.integers(0, 3))]
        lines = [b"Host: svc-%d.example.com\r\n" % int(rng.integers(0, 25)), b"X-Forwarded-Proto: https\r\n",
                 b"x-token: secret\r\n"][:int(rng.integers(0, 4))]
        heads.append(method + b" " + path + b" HTTP/1.1\r\n" + b"".join(lines) + b"\r\n")
    return heads


def test_decode_eval_log_on_one_stream(gpu):
    import torch
    heads = _e2e_heads()
    n = len(heads)
    # random identity, port and direction; the rule set's own endpoint policy (index 0)
    metas = [(rid, dport, 0, ingress) for rid, dport, _, ingress in W.metas_for(n)]
    rs = L.RuleSet.compile_http(RULES)
    # the host chain
    h_arena, h_offs, h_status = L.decode_http_wire(heads, W.meta_array(metas))
    h_verd = rs.eval(h_arena, h_offs)
    assert (h_status < 0).sum() > 20 and (h_verd == L.VERDICT_DENY).sum() > 100 and (h_verd >= 0).sum() > 100
    exp = _host_entries(h_arena, h_offs, h_verd, L.LOG_DENIED, **C.ALL_STRINGS)
    total = sum(map(len, exp))

    wire, hoffs = L.join_heads(heads)
    cap = (L.http_wire_arena_bound(wire.nbytes, n) + 15) // 16 * 16
    d_wire = torch.from_numpy(wire.copy()).cuda()
    d_hoffs = torch.from_numpy(hoffs.view(np.int64)).cuda()
    d_meta = torch.from_numpy(W.meta_array(metas).view(np.uint8)).cuda()
    d_arena = torch.full((cap,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_bytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_verd = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
    d_out = torch.full((total + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_eo = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    # three enqueues on one non-default stream, nothing between them; the arena's size is not
    # known on the host, so the later stages are given its capacity
    L.decode_http_wire_device(d_wire, wire.nbytes, d_hoffs, n, d_meta, d_arena, cap, d_offs, d_status, d_bytes,
                              s.cuda_stream)
    rs.eval_device(d_arena, cap, d_offs, n, d_verd, None, s.cuda_stream)
    L.http_access_log_device(d_arena, cap, d_offs, n, d_verd, d_out, total, d_eo, d_total, s.cuda_stream,
                             select=L.LOG_DENIED, **C.ALL_STRINGS)
    s.synchronize()
    assert np.array_equal(d_verd.cpu().numpy(), h_verd)
    assert int(d_total.item()) == total
    eo = d_eo.cpu().numpy().view(np.uint64)
    out = d_out.cpu().numpy()
    raw = out.tobytes()
    assert [raw[int(eo[i]):int(eo[i + 1])] for i in range(n)] == exp
    assert np.all(out[total:] == SENTINEL)
    # and the statistics of the same device batch
    t_dev, t_host = L.ProxyStatsTable(), L.ProxyStatsTable()
    t_dev.update_device(L.PROTO_HTTP, d_arena, cap, d_offs, d_verd, n, port=1, ingress=False, stream=s.cuda_stream)
    t_host.update(L.PROTO_HTTP, h_arena, h_offs, h_verd, port=1, ingress=False)
    assert t_dev.entries() == t_host.entries()
    assert ("http", 1, False, True) in t_dev.entries()  # the refused heads' records: the caller's key


# ---- statistics -----------------------------------------------------------------
def _stats_both(batches, port=4242, ingress=False, tables=None):
    import torch
    t_dev, t_host = tables or (L.ProxyStatsTable(), L.ProxyStatsTable())
    for arena, offs, verdicts in batches:
        d_arena, d_offs, d_verd = _to_device(arena, offs, verdicts)
        torch.cuda.synchronize()
        t_dev.update_device(L.PROTO_HTTP, d_arena, arena.nbytes, d_offs, d_verd, len(verdicts), port, ingress,
                            torch.cuda.current_stream().cuda_stream)
        t_host.update(L.PROTO_HTTP, arena, offs, verdicts, port, ingress)
    assert t_dev.entries() == t_host.entries()
    return t_dev.entries()


def test_stats_fuzz_ports_match_host(gpu, fuzz):
    cases, batch = fuzz
    e = _stats_both([batch])
    assert e == C.expected_stats(cases, 4242, False)
    assert len(e) > 1500 and {k[2] for k in e} == {True, False}


def test_stats_one_contended_key(gpu):
    cases = [(C.fields(dport=443, raw=True), C.VERDICTS[i % len(C.VERDICTS)]) for i in range(4096)]
    e = _stats_both([C.build(cases)])
    assert list(e) == [("http", 443, True, True)] and e[("http", 443, True, True)]["received"] == 4096


def test_stats_malformed_records_use_the_callers_key(gpu, table):
    cases, batch = table
    for port, ingress in ((4242, False), (0, True), (65535, True)):
        e = _stats_both([batch], port, ingress)
        assert e == C.expected_stats(cases, port, ingress)
        assert e[("http", port, ingress, True)]["received"] >= sum(1 for f, _ in cases if f["bad"])


def test_stats_accumulate_over_calls_and_beside_kafka_entries(gpu, table, fuzz):
    tables = (L.ProxyStatsTable(), L.ProxyStatsTable())
    k_arena, k_offs = L.pack_records([K.metadata(0, "c", ["t"]), K.metadata(1, "c", ["u"])])
    for t in tables:
        t.update(L.PROTO_KAFKA, k_arena, k_offs, np.array([0, -1], dtype=np.int32), port=9092, ingress=True)
    e = _stats_both([table[1], fuzz[1], table[1]], tables=tables)
    assert e[("kafka", 9092, True, True)] == {"received": 2, "forwarded": 1, "denied": 1, "error": 0}
    assert sum(v["received"] for k, v in e.items() if k[0] == "http") == 2 * len(table[0]) + len(fuzz[0])


def test_stats_batch_sizes(gpu, fuzz):
    _, (arena, offs, verdicts) = fuzz
    for n in (0, 1, 63, 65, TILE + 1):
        _stats_both([(arena, offs[:n], verdicts[:n])])
