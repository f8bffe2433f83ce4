"""Device side of the HTTP/1.x wire path: l7m_http_wire_decode_device must
reproduce the host decoder byte for byte (which tests/test_http_wire_cpu.py
holds to the Python decoder), feed l7m_eval_device on the same stream, and
the batcher's raw-head call must agree with the batch evaluation."""
import threading

import numpy as np
import pytest

import http_wire_cases as C
from cilium_amd import l7match as L

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
TILE = 256         # heads per workgroup tile (l7m_http_wire.hip kWireTile)
STAGE = 64 * 1024  # wire bytes a tile stages at once (kWireStage)


def _device_decode(heads, metas=None, cap=None, stream=None, shift=3):
    """-> (arena uint8[alloc] incl. untouched sentinel bytes, offsets, status, total).
    The wire sits `shift` bytes off a 16-byte boundary: nothing promises its alignment."""
    import torch
    wire, hoffs = L.join_heads(heads)
    n = len(heads)
    d_buf = torch.zeros(wire.nbytes + shift + 16, dtype=torch.uint8, device="cuda")
    d_wire = d_buf[shift:shift + wire.nbytes]
    if wire.nbytes:
        d_wire.copy_(torch.from_numpy(wire.copy()))
    d_hoffs = torch.from_numpy(hoffs.view(np.int64)).cuda()
    d_meta = None if metas is None else torch.from_numpy(C.meta_array(metas).view(np.uint8)).cuda()
    if cap is None:
        cap = L.http_wire_arena_bound(wire.nbytes, n)
    alloc = (cap + 15) // 16 * 16 + 16
    d_arena = torch.full((alloc,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_offs = torch.full((max(1, n),), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((max(1, n),), 99, dtype=torch.int32, device="cuda")
    d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.decode_http_wire_device(d_wire, wire.nbytes, d_hoffs, n, d_meta, d_arena, cap, d_offs, d_status, d_total,
                              stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (d_arena.cpu().numpy(), d_offs.cpu().numpy().view(np.uint64)[:n], d_status.cpu().numpy()[:n],
            int(d_total.item()))


def _check_equals_host(heads, metas=None):
    h_arena, h_offs, h_status = L.decode_http_wire(heads, None if metas is None else C.meta_array(metas))
    total = h_arena.shape[0] if len(heads) else 0  # a record has 20 bytes at least
    arena, offs, status, got_total = _device_decode(heads, metas)
    assert got_total == total
    assert np.array_equal(status, h_status)
    assert np.array_equal(offs, h_offs)
    assert arena[:total].tobytes() == h_arena[:total].tobytes()
    assert np.all(arena[total:] == SENTINEL)  # nothing past the total, the pad of the last record included
    return h_status


@pytest.fixture(scope="module")
def fuzz():
    return C.fuzz_heads()


def test_table_matches_host(gpu):
    heads = C.table_heads()
    st = _check_equals_host(heads, C.metas_for(len(heads)))
    assert (st < 0).any() and (st >= 0).any()


def test_fuzz_matches_host(gpu, fuzz):
    _check_equals_host(fuzz)  # 2000 heads: eight tiles, the last one partial


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_batch_sizes_match_host(gpu, fuzz, n):
    _check_equals_host(fuzz[100:100 + n], C.metas_for(n, seed=n))


def _big(k, size):
    """An accepted head of exactly `size` bytes: values of up to 1000 bytes."""
    first = b"POST /big/%d HTTP/1.1\r\nHost: big-%d\r\n" % (k, k)
    left = size - len(first) - 2
    lines = []
    while left:
        take = left if left < 1015 else 1007  # a line is `x-b: ` + value + CRLF; the last one has a value
        lines.append(b"x-b: " + bytes([97 + (k + len(lines)) % 26]) * (take - 7) + b"\r\n")
        left -= take
    head = first + b"".join(lines) + b"\r\n"
    assert len(head) == size
    return head


def test_heads_larger_than_the_stage_match_host(gpu, fuzz):
    """One head above the stage (walked from global memory) between ordinary ones, also
    as the first and the last head of a tile, and one that is refused at its very end."""
    bad = _big(3, STAGE + 5000)[:-2] + b"\n\n"
    heads = [_big(0, STAGE + 3000)] + fuzz[:TILE - 2] + [_big(1, 100000), _big(2, STAGE + 1)] + fuzz[300:310] + [bad]
    assert all(len(heads[i]) > STAGE for i in (0, TILE - 1, TILE))
    st = _check_equals_host(heads)
    assert st[0] == len(heads[0]) and st[TILE - 1] == len(heads[TILE - 1]) and st[-1] == C.EBADHEADER


def test_run_of_near_stage_size_heads_matches_host(gpu, fuzz):
    """Heads that fit the stage one or two at a time: the tile takes many chunks."""
    heads = fuzz[:5]
    heads += [_big(k, STAGE - 2500) for k in range(4)]      # one per chunk
    heads += [_big(10 + k, STAGE // 2 - 2000) for k in range(6)]  # two per chunk
    heads += fuzz[5:40] + [_big(20, STAGE - 16), _big(21, STAGE - 15)] + fuzz[40:60]
    # the stage starts at a 16-byte boundary of the wire: whether the largest two are
    # staged or walked from global memory depends on where they start
    assert max(map(len, heads)) == STAGE - 15
    _check_equals_host(heads, C.metas_for(len(heads)))


def test_cap_one_byte_short_leaves_the_arena_untouched(gpu, fuzz):
    heads = fuzz[:600]
    h_arena, h_offs, h_status = L.decode_http_wire(heads)
    total = h_arena.shape[0]
    arena, offs, status, got_total = _device_decode(heads, cap=total - 1)
    assert got_total == total and got_total > total - 1
    assert np.all(arena == SENTINEL)
    assert np.array_equal(offs, h_offs) and np.array_equal(status, h_status)
    # and exactly enough is enough
    arena, offs, status, got_total = _device_decode(heads, cap=total)
    assert got_total == total and arena[:total].tobytes() == h_arena.tobytes()
    assert np.all(arena[total:] == SENTINEL)


RULES = [
    L.PortRuleHTTP(Path="/api/v[0-9]+/.*", Method="GET"),
    L.PortRuleHTTP(Method="PUT|POST", Host="svc-1[0-9]?\\.example\\.com"),
    L.PortRuleHTTP(Path="/public/.*", Headers=["X-Token: secret"]),
    L.PortRuleHTTP(Host="first\\.example"),
    L.PortRuleHTTP(Path="http://.*", Headers=["X-Present"]),
]


def _e2e_heads(fuzz):
    rng = np.random.default_rng(11)
    heads = list(fuzz[:700])
    for i in range(500):
        method = [b"GET", b"PUT", b"POST", b"HEAD"][int(rng.integers(0, 4))]
        path = [b"/api/v%d/x" % int(rng.integers(0, 30)), b"/public/a", b"/private", b"http://first.example/p",
                b"/api/vx/"][int(rng.integers(0, 5))]
        lines = [b"Host: svc-%d.example.com\r\n" % int(rng.integers(0, 25))] if rng.random() < 0.8 else []
        if rng.random() < 0.5:
            lines.append([b"x-token: secret\r\n", b"X-Token:  secret \r\n", b"x-token: Secret\r\n",
                          b"X-Present:\r\n"][int(rng.integers(0, 4))])
        rng.shuffle(lines)
        heads.append(method + b" " + path + b" HTTP/1.1\r\n" + b"".join(lines) + b"\r\n")
    # the Host header decides a Host rule wherever it stands, not the target's
    # authority and not a header that merely resembles it; a second one is an error
    heads += [b"GET /h HTTP/1.1\r\nHost: first.example\r\nx-host: other.example\r\n\r\n",
              b"GET /h HTTP/1.1\r\nx-host: first.example\r\nHost: other.example\r\n\r\n",
              b"GET /h HTTP/1.1\r\nx-a: 1\r\nx-b: 2\r\nhOST: first.example\r\n\r\n",
              b"GET http://other.example/h HTTP/1.1\r\nHost: first.example\r\n\r\n",
              b"GET http://first.example/h HTTP/1.1\r\nHost: other.example\r\n\r\n",
              b"GET http://first.example/h HTTP/1.1\r\n\r\n",
              b"GET /h HTTP/1.1\r\nHost: first.example\r\nHost: other.example\r\n\r\n",
              b"GET /h HTTP/1.1\r\nHost: other.example\r\nHost: first.example\r\n\r\n"]
    return heads


def test_decode_then_eval_on_one_stream(gpu, fuzz):
    import torch
    from oracle import HttpOracle
    heads = _e2e_heads(fuzz)
    n = len(heads)
    # expected: the oracle on the requests as the Python decoder parses them
    parsed = C.parsed_requests(heads)
    recs = [C.record(m, t, h, hd) for _, m, t, h, hd in parsed]
    o_arena, o_offs = L.pack_records(recs)
    exp = np.full(n, L.VERDICT_PARSE_ERROR, dtype=np.int32)
    exp[[p[0] for p in parsed]] = HttpOracle(RULES).eval(o_arena, o_offs)
    _, _, exp_status = C.decode(heads)

    rs = L.RuleSet.compile_http(RULES)
    wire, hoffs = L.join_heads(heads)
    cap = (L.http_wire_arena_bound(wire.nbytes, n) + 15) // 16 * 16
    d_wire = torch.from_numpy(wire.copy()).cuda()
    d_hoffs = torch.from_numpy(hoffs.view(np.int64)).cuda()
    d_arena = torch.full((cap,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_verd = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    # two enqueues on one non-default stream, nothing between them: the arena's size is
    # not known on the host, so the evaluator is given the capacity
    L.decode_http_wire_device(d_wire, wire.nbytes, d_hoffs, n, None, d_arena, cap, d_offs, d_status, d_total,
                              s.cuda_stream)
    rs.eval_device(d_arena, cap, d_offs, n, d_verd, None, s.cuda_stream)
    s.synchronize()
    got = d_verd.cpu().numpy()
    status = d_status.cpu().numpy()
    assert np.array_equal(status, exp_status)
    assert np.array_equal(got == L.VERDICT_PARSE_ERROR, status < 0)
    assert np.array_equal(got, exp)
    # the Host cases at the end: rule 3 (Host first.example) by the Host header alone
    assert got[-8:].tolist() == [3, -1, 3, 3, -1, -1, L.VERDICT_PARSE_ERROR, L.VERDICT_PARSE_ERROR]
    assert len(set(got.tolist())) >= 6  # every rule, deny and parse error occur


def test_batcher_eval_http_wire_from_8_threads(gpu, fuzz):
    heads = _e2e_heads(fuzz)[600:1208]
    rs = L.RuleSet.compile_http(RULES)
    arena, offs, status = L.decode_http_wire(heads)
    exp = rs.eval(arena, offs)
    assert np.array_equal(exp == L.VERDICT_PARSE_ERROR, status < 0)
    b = L.Batcher(rs, max_batch=64, max_delay_us=100)
    got = np.zeros(len(heads), dtype=np.int32)
    got_status = np.zeros(len(heads), dtype=np.int32)
    errors = []

    def work(k):
        try:
            for i in range(k, len(heads), 8):
                got[i], got_status[i] = b.eval_http_wire(heads[i])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    _, requests = b.stats()
    b.close()
    assert not errors
    assert np.array_equal(got_status, status)
    assert np.array_equal(got, exp)
    assert (status < 0).sum() > 20
    assert requests == int((status >= 0).sum())  # refused heads were not submitted


def test_batcher_eval_http_wire_meta(gpu):
    rs = L.RuleSet.compile_http([L.PortRuleHTTP(Path="/a", RemoteIDs=[7])])
    b = L.Batcher(rs, max_batch=8, max_delay_us=50)
    try:
        assert b.eval_http_wire(b"GET /a HTTP/1.1\r\n\r\n", remote_id=7) == (0, 19)
        assert b.eval_http_wire(b"GET /a HTTP/1.1\r\n\r\n", remote_id=8) == (L.VERDICT_DENY, 19)
        assert b.eval_http_wire(b"GET /a HTTP/1.1\r\n", remote_id=7) == (L.VERDICT_PARSE_ERROR, L.WIRE_EINCOMPLETE)
    finally:
        b.close()
