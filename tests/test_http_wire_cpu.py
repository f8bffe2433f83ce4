"""Host side of the HTTP/1.x wire path (l7m_http_wire_decode / _encode /
_arena_bound) against the pure-Python decoder of tests/http_wire_cases.py."""
import struct

import numpy as np
import pytest

import http_wire_cases as C
from cilium_amd import l7match as L
from raw_cases import pack_raw


@pytest.fixture(scope="module")
def fuzz():
    heads = C.fuzz_heads()
    return heads, C.decode(heads)


def _check(heads, metas=None, expected=None):
    exp_arena, exp_offs, exp_status = expected or C.decode(heads, metas)
    arena, offs, status = L.decode_http_wire(heads, None if metas is None else C.meta_array(metas))
    assert np.array_equal(status, exp_status)
    assert np.array_equal(offs, exp_offs)
    total = len(exp_arena)
    assert arena.shape[0] == max(4, total)
    assert arena[:total].tobytes() == exp_arena
    return arena, offs, status


def test_table_known_answers():
    """The table's expected status is what the Python decoder says (the table pins the grammar)."""
    seen = set()
    for name, head, want in C.TABLE:
        _, _, status = C.decode([head])
        if want is None:
            want = len(head)
        assert int(status[0]) == want, name
        seen.add(min(int(status[0]), 0))
    assert seen == {0, C.EINCOMPLETE, C.EBADLINE, C.EBADHEADER, C.EDUPHOST, C.ETOOMANY, C.ETOOLONG}


def test_constants_match():
    assert (L.WIRE_EINCOMPLETE, L.WIRE_EBADLINE, L.WIRE_EBADHEADER, L.WIRE_EDUPHOST, L.WIRE_ETOOMANY,
            L.WIRE_ETOOLONG) == (C.EINCOMPLETE, C.EBADLINE, C.EBADHEADER, C.EDUPHOST, C.ETOOMANY, C.ETOOLONG)


@pytest.mark.parametrize("name,head,want", C.TABLE, ids=[t[0] for t in C.TABLE])
def test_decode_table_one_by_one(name, head, want):
    _check([head])


def test_decode_table_batch_with_meta():
    heads = C.table_heads()
    _check(heads, C.metas_for(len(heads)))


def test_decode_fuzz(fuzz):
    heads, expected = fuzz
    _, _, status = _check(heads, expected=expected)
    # the set exercises both outcomes and most codes
    assert (status >= 0).sum() > 500 and (status < 0).sum() > 300
    assert {C.EINCOMPLETE, C.EBADLINE, C.EBADHEADER, C.EDUPHOST} <= set(status.tolist())


def test_decode_fuzz_with_meta(fuzz):
    heads = fuzz[0][:300]
    _check(heads, C.metas_for(len(heads)))


def test_decode_empty_batch():
    arena, offs, status = L.decode_http_wire([])
    assert offs.shape == (0,) and status.shape == (0,)


def test_decode_rejects_descending_offsets():
    wire = np.frombuffer(b"GET / HTTP/1.1\r\n\r\n", dtype=np.uint8)
    for hoffs in ([0, 19], [5, 2], [0, 10, 5]):
        with pytest.raises(L.L7Error) as e:
            L.decode_http_wire((wire, np.array(hoffs, dtype=np.uint64)))
        assert e.value.code == L.L7M_EINVAL


def test_encode_then_decode_reproduces_records(fuzz):
    heads, (exp_arena, exp_offs, exp_status) = fuzz
    arena = np.frombuffer(exp_arena, dtype=np.uint8)
    wire, hoffs, est = L.encode_http_wire(arena, exp_offs)
    # the encoder takes every record the decoder produced from an accepted head and no failed one
    assert np.array_equal(est >= 0, exp_status >= 0)
    assert np.array_equal(est[est >= 0].astype(np.uint64), np.diff(hoffs)[est >= 0])
    assert np.all(np.diff(hoffs)[est < 0] == 0)
    arena2, offs2, status2 = L.decode_http_wire((wire, hoffs))
    ok = np.flatnonzero(est >= 0)
    assert np.array_equal(status2[ok], est[ok])  # the whole head is consumed
    ends = np.append(exp_offs[1:], len(exp_arena)).astype(np.int64)
    ends2 = np.append(offs2[1:], arena2.shape[0]).astype(np.int64)
    for i in ok:
        a = exp_arena[int(exp_offs[i]):ends[i]]
        assert arena2[int(offs2[i]):ends2[i]].tobytes() == a, i


def test_encode_roundtrip_packed_requests():
    reqs = [L.HTTPRequest("GET", "/p/%d" % i, "h%d.example" % i if i % 3 else None,
                          [("X-K", "v%d" % i), ("accept", "")][: i % 3], remote_id=i, dport=80 + i, ingress=bool(i % 2),
                          policy=i % 5) for i in range(40)]
    arena, offs = L.pack_http(reqs)
    wire, hoffs, est = L.encode_http_wire(arena, offs)
    assert np.all(est > 0)
    metas = [(q.remote_id, q.dport, q.policy, int(q.ingress)) for q in reqs]
    arena2, offs2, status2 = L.decode_http_wire((wire, hoffs), C.meta_array(metas))
    assert np.array_equal(offs2, offs)
    assert arena2.tobytes() == arena.tobytes()
    assert np.array_equal(status2.astype(np.uint64), np.diff(hoffs))


REFUSED = [
    ("space in method", (b"G T", b"/", b"h", []), C.EBADLINE),
    ("empty method", (b"", b"/", b"h", []), C.EBADLINE),
    ("empty path", (b"GET", b"", b"h", []), C.EBADLINE),
    ("space in path", (b"GET", b"/a b", b"h", []), C.EBADLINE),
    ("nul in path", (b"GET", b"/a\0b", b"h", []), C.EBADLINE),
    ("header named host", (b"GET", b"/", b"h", [(b"host", b"x")]), C.EDUPHOST),
    ("leading ows in value", (b"GET", b"/", b"h", [(b"x-a", b" v")]), C.EBADHEADER),
    ("trailing ows in value", (b"GET", b"/", b"h", [(b"x-a", b"v\t")]), C.EBADHEADER),
    ("cr in value", (b"GET", b"/", b"h", [(b"x-a", b"a\rb")]), C.EBADHEADER),
    ("lf in value", (b"GET", b"/", b"h", [(b"x-a", b"a\nb")]), C.EBADHEADER),
    ("nul in value", (b"GET", b"/", b"h", [(b"x-a", b"a\0b")]), C.EBADHEADER),
    ("ows in authority", (b"GET", b"/", b" h", []), C.EBADHEADER),
    ("lf in authority", (b"GET", b"/", b"h\n", []), C.EBADHEADER),
    ("empty name", (b"GET", b"/", b"h", [(b"", b"v")]), C.EBADHEADER),
    ("colon in name", (b"GET", b"/", b"h", [(b"x:a", b"v")]), C.EBADHEADER),
    ("upper case in name", (b"GET", b"/", b"h", [(b"X-a", b"v")]), C.EBADHEADER),
]


@pytest.mark.parametrize("name,req,code", REFUSED, ids=[r[0] for r in REFUSED])
def test_encoder_refuses(name, req, code):
    good = (b"GET", b"/ok", b"h", [(b"x-a", b"v")])
    arena, offs = pack_raw([good, req, good])
    wire, hoffs, est = L.encode_http_wire(arena, offs)
    assert int(est[1]) == code
    assert hoffs[1] == hoffs[2]  # an empty head
    assert est[0] > 0 and est[2] > 0
    assert wire.tobytes() == b"GET /ok HTTP/1.1\r\nhost: h\r\nx-a: v\r\n\r\n" * 2


def test_encoder_refuses_failed_and_truncated_records():
    failed = C.failed_record()
    arena = np.frombuffer(failed + b"\x40\0\0\0", dtype=np.uint8)
    _, hoffs, est = L.encode_http_wire(arena, np.array([0, 20], dtype=np.uint64))
    assert est.tolist() == [C.EBADHEADER, C.EBADHEADER] and hoffs.tolist() == [0, 0, 0]


def test_arena_bound_holds_over_fuzz(fuzz):
    heads, (exp_arena, exp_offs, _) = fuzz
    assert len(exp_arena) <= L.http_wire_arena_bound(sum(map(len, heads)), len(heads))
    sizes = np.diff(np.append(exp_offs, len(exp_arena)).astype(np.int64))
    for h, s in zip(heads, sizes):
        assert s <= L.http_wire_arena_bound(len(h), 1), h
    for _, h, _ in C.TABLE:
        assert len(C.decode([h])[0]) <= L.http_wire_arena_bound(len(h), 1)


def test_arena_bound_is_met_by_the_worst_case_head():
    """Derivation (include/l7match.h): every header line `a:CRLF` spends 4 wire
    bytes on a 5-byte record share, method and target one byte each, and the
    record's size before padding is 1 mod 4: bound(W, 1) bytes exactly."""
    assert L.http_wire_arena_bound(0, 0) == 0 and L.http_wire_arena_bound(0, 3) == 60
    for h in (3, 7, 255):
        head = b"G / HTTP/1.1\r\n" + b"a:\r\n" * h + b"\r\n"
        arena, _, status = C.decode([head])
        assert status[0] == len(head)
        bound = L.http_wire_arena_bound(len(head), 1)
        assert len(arena) == bound == 20 + len(head) + len(head) // 4 - 15
        got, _, _ = L.decode_http_wire([head], cap=bound)
        assert got.tobytes() == arena
        # ... and beside empty slices, which cost their 20 bytes each
        heads = [b"", head, b""]
        assert len(C.decode(heads)[0]) == L.http_wire_arena_bound(len(head), 3)


def test_cap_one_byte_short(fuzz):
    heads = fuzz[0][:50]
    exp_arena, exp_offs, exp_status = C.decode(heads)
    with pytest.raises(L.L7Error) as e:
        L.decode_http_wire(heads, cap=len(exp_arena) - 1)
    assert e.value.code == L.L7M_ENOMEM and e.value.needed == len(exp_arena)
    arena, offs, status = L.decode_http_wire(heads, cap=len(exp_arena))
    assert arena.tobytes() == exp_arena


def test_cap_short_still_reports_offsets_and_status():
    import ctypes
    heads = C.table_heads()[:12]
    exp_arena, exp_offs, exp_status = C.decode(heads)
    wire, hoffs = L.join_heads(heads)
    n = len(heads)
    cap = len(exp_arena) - 1
    arena = np.full(cap + 8, 0xA5, dtype=np.uint8)
    offs = np.zeros(n, dtype=np.uint64)
    status = np.zeros(n, dtype=np.int32)
    used = ctypes.c_size_t(0)
    rc = L.lib().l7m_http_wire_decode(wire.ctypes.data, wire.nbytes, hoffs.ctypes.data, n, None, arena.ctypes.data,
                                      cap, offs.ctypes.data, status.ctypes.data, ctypes.byref(used))
    assert rc == L.L7M_ENOMEM and used.value == len(exp_arena)
    assert np.array_equal(offs, exp_offs) and np.array_equal(status, exp_status)
    assert np.all(arena[cap:] == 0xA5)  # nothing past cap


def test_failed_record_layout():
    metas = [(0xDEADBEEF, 8080, 7, 0), (1, 2, 3, 1)]
    arena, offs, status = L.decode_http_wire([b"GET", b"\n"], C.meta_array(metas))
    assert status.tolist() == [C.EINCOMPLETE, C.EBADLINE] and offs.tolist() == [0, 20]
    assert struct.unpack("<5I", arena[:20].tobytes()) == (0, 0xDEADBEEF, 8080, 0, 7 << 16)
    assert struct.unpack("<5I", arena[20:40].tobytes()) == (0, 1, 2 | 8 << 16, 0, 3 << 16)
