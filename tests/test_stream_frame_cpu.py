"""Host side of stream framing (l7m_http_stream_frame, l7m_kafka_stream_frame
and their bounds) against the pure-Python framer of tests/stream_cases.py."""
import ctypes
import os
import struct

import numpy as np
import pytest

import http_wire_cases as W
import stream_cases as S
from cilium_amd import l7match as L

SENT = 0xA5


@pytest.fixture(scope="module")
def http_fuzz():
    conns = S.fuzz_http_conns()
    metas = W.metas_for(len(conns), seed=9)
    return conns, metas, S.frame_http(conns, metas)


@pytest.fixture(scope="module")
def kafka_fuzz():
    conns = S.fuzz_kafka_conns()
    ids = np.random.default_rng(3).integers(0, 1 << 32, size=len(conns), dtype=np.uint32)
    return conns, ids, S.frame_kafka(conns, ids)


def _meta_tuples(a):
    return [(int(m["remote_id"]), int(m["dport"]), int(m["policy"]), int(m["ingress"])) for m in a]


def check_http(conns, metas=None, expected=None):
    e_offs, e_conn, e_meta, e_status, e_consumed = expected or S.frame_http(conns, metas)
    wire, offs, hconn, hmeta, status, consumed = L.frame_http_streams(
        conns, None if metas is None else W.meta_array(metas))
    assert np.array_equal(status, e_status)
    assert np.array_equal(consumed, e_consumed)
    assert np.array_equal(offs, e_offs)
    assert np.array_equal(hconn, e_conn)
    if metas is None:
        assert hmeta is None
    else:
        assert _meta_tuples(hmeta) == e_meta
        assert not hmeta["reserved"].any()
    return wire, offs, hconn, status, consumed


def check_kafka(conns, ids=None, expected=None):
    e_arena, e_offs, e_conn, e_ids, e_status, e_consumed, _ = expected or S.frame_kafka(conns, ids)
    arena, offs, rconn, sids, status, consumed = L.frame_kafka_streams(conns, ids)
    assert np.array_equal(status, e_status)
    assert np.array_equal(consumed, e_consumed)
    assert np.array_equal(offs, e_offs)
    assert np.array_equal(rconn, e_conn)
    assert arena.shape[0] == max(4, len(e_arena))
    assert arena[:len(e_arena)].tobytes() == e_arena
    if ids is None:
        assert sids is None
    else:
        assert np.array_equal(sids, e_ids)
    return arena, offs, rconn, status, consumed


def test_constants_and_abi():
    assert L.lib().l7m_abi_version() == 4
    assert (L.STREAM_OK, L.STREAM_TUNNEL, L.STREAM_EBADHEAD, L.STREAM_EPARTIAL_HEAD, L.STREAM_EAMBIGUOUS,
            L.STREAM_EBADTE, L.STREAM_EBADLENGTH, L.STREAM_EBADCHUNK, L.STREAM_EPARTIAL_BODY,
            L.STREAM_EPARTIAL_FRAME, L.STREAM_EBADSIZE) == (
        S.OK, S.TUNNEL, S.EBADHEAD, S.EPARTIAL_HEAD, S.EAMBIGUOUS, S.EBADTE, S.EBADLENGTH, S.EBADCHUNK,
        S.EPARTIAL_BODY, S.EPARTIAL_FRAME, S.EBADSIZE)
    for name in ("l7m_http_stream_frame", "l7m_http_stream_frame_device", "l7m_kafka_stream_frame",
                 "l7m_kafka_stream_frame_device", "l7m_http_stream_heads_bound", "l7m_kafka_stream_records_bound",
                 "l7m_kafka_stream_arena_bound"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.lib(), name)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "l7match.h")) as f:
        header = f.read()
    for name, value in (("OK", S.OK), ("TUNNEL", S.TUNNEL), ("EBADHEAD", S.EBADHEAD), ("EPARTIAL_HEAD", S.EPARTIAL_HEAD),
                        ("EAMBIGUOUS", S.EAMBIGUOUS), ("EBADTE", S.EBADTE), ("EBADLENGTH", S.EBADLENGTH),
                        ("EBADCHUNK", S.EBADCHUNK), ("EPARTIAL_BODY", S.EPARTIAL_BODY),
                        ("EPARTIAL_FRAME", S.EPARTIAL_FRAME), ("EBADSIZE", S.EBADSIZE)):
        want = "#define L7M_STREAM_%s %s" % (name, value if value >= 0 else "(%d)" % value)
        assert want + " " in header or want + "\n" in header, name


def test_http_table_known_answers():
    """The table's answers are what the Python framer says (the table pins the rules), every code among them."""
    seen = set()
    for name, conn, status, starts, consumed in S.HTTP_TABLE:
        assert S.frame_http_conn(conn) == (starts, status, consumed), name
        seen.add(status)
    assert seen == {S.OK, S.TUNNEL, S.EBADHEAD, S.EPARTIAL_HEAD, S.EAMBIGUOUS, S.EBADTE, S.EBADLENGTH, S.EBADCHUNK,
                    S.EPARTIAL_BODY}


def test_kafka_table_known_answers():
    seen = set()
    for name, conn, status, frames, consumed in S.KAFKA_TABLE:
        assert S.frame_kafka_conn(conn) == (frames, status, consumed), name
        seen.add(status)
    assert seen == {S.OK, S.EBADSIZE, S.EPARTIAL_FRAME}
    starts = {s % 4 for _, _, _, frames, _ in S.KAFKA_TABLE for s, _ in frames}
    assert starts == {0, 1, 2, 3}


@pytest.mark.parametrize("name,conn,status,starts,consumed", S.HTTP_TABLE, ids=[t[0] for t in S.HTTP_TABLE])
def test_http_table_one_by_one(name, conn, status, starts, consumed):
    _, offs, _, st, used = check_http([conn])
    assert (int(st[0]), offs[:-1].tolist(), int(used[0])) == (status, starts, consumed)


def test_http_table_batch_with_meta():
    conns = S.http_table_conns()
    check_http(conns, W.metas_for(len(conns)))


@pytest.mark.parametrize("name,conn,status,frames,consumed", S.KAFKA_TABLE, ids=[t[0] for t in S.KAFKA_TABLE])
def test_kafka_table_one_by_one(name, conn, status, frames, consumed):
    _, offs, _, st, used = check_kafka([conn])
    assert (int(st[0]), int(used[0]), len(offs)) == (status, consumed, len(frames))


def test_kafka_table_batch_with_identities():
    conns = S.kafka_table_conns()
    check_kafka(conns, np.arange(100, 100 + len(conns), dtype=np.uint32))


def test_http_fuzz(http_fuzz):
    conns, metas, expected = http_fuzz
    _, _, _, status, _ = check_http(conns, metas, expected)
    assert {S.OK, S.TUNNEL, S.EBADHEAD, S.EPARTIAL_HEAD, S.EBADCHUNK, S.EPARTIAL_BODY} <= set(status.tolist())
    check_http(conns[:200])


def test_kafka_fuzz(kafka_fuzz):
    conns, ids, expected = kafka_fuzz
    _, _, _, status, _ = check_kafka(conns, ids, expected)
    assert {S.OK, S.EBADSIZE, S.EPARTIAL_FRAME} == set(status.tolist())
    check_kafka(conns[:200])


def test_fuzz_shares_hold_for_other_seeds():
    """Between a quarter and three quarters of the connections end OK (asserted as the sets are built)."""
    for seed in range(8):
        S.ok_shares(seed)


def test_empty_batches():
    wire, offs, hconn, hmeta, status, consumed = L.frame_http_streams([])
    assert offs.tolist() == [0] and hconn.shape == (0,) and status.shape == (0,)
    arena, offs, rconn, sids, status, consumed = L.frame_kafka_streams([])
    assert offs.shape == (0,) and status.shape == (0,)
    check_http([b"", b"", b""])
    check_kafka([b"", b""])


def test_http_slices_tile_the_connections(http_fuzz):
    """The slices of a connection tile its bytes; every non-empty connection yields at least one."""
    conns = S.http_table_conns() + http_fuzz[0]
    coffs = S.conn_offs(conns)
    wire, offs, hconn, _, status, consumed = L.frame_http_streams(conns)
    assert offs[-1] == coffs[-1] and (offs[0] == coffs[0])
    assert np.all(offs[1:] > offs[:-1])  # no empty slice
    assert np.all(hconn[1:] >= hconn[:-1])
    first = np.searchsorted(hconn, np.arange(len(conns)), side="left")
    last = np.searchsorted(hconn, np.arange(len(conns)), side="right")
    for c, conn in enumerate(conns):
        if not conn:
            assert first[c] == last[c] and status[c] == S.OK
            continue
        assert last[c] > first[c]
        assert offs[first[c]] == coffs[c] and offs[last[c]] == coffs[c + 1]
        assert consumed[c] <= len(conn)
        assert (status[c] == S.OK) == (consumed[c] == len(conn)) or status[c] == S.TUNNEL
    assert len(hconn) <= L.http_stream_heads_bound(int(coffs[-1]), len(conns))


def test_decoder_reports_the_code_the_status_implies(http_fuzz):
    """l7m_http_wire_decode over the framer's head_offs: every slice but a refused or partial last one
    decodes, and that one to the code the connection's status implies."""
    conns = S.http_table_conns() + http_fuzz[0]
    wire, offs, hconn, _, status, _ = L.frame_http_streams(conns)
    _, _, wstatus = L.decode_http_wire((wire, offs))
    last = np.searchsorted(hconn, np.arange(len(conns)), side="right") - 1
    is_last = np.zeros(len(hconn), dtype=bool)
    nonempty = np.array([len(c) > 0 for c in conns])
    is_last[last[nonempty]] = True
    cst = status[hconn]
    bad = is_last & ((cst == S.EBADHEAD) | (cst == S.EPARTIAL_HEAD))
    assert np.all(wstatus[~bad] >= 0)
    assert np.all(wstatus[is_last & (cst == S.EPARTIAL_HEAD)] == W.EINCOMPLETE)
    assert np.all(wstatus[is_last & (cst == S.EBADHEAD)] < W.EINCOMPLETE)
    assert bad.sum() > 50


def _http_call(wire, coffs, cap, with_arrays=True, meta=None):
    nc = len(coffs) - 1
    offs = np.full(cap + 1, SENT, dtype=np.uint64)
    hconn = np.full(cap, SENT, dtype=np.uint32)
    hmeta = np.full(cap * 12, SENT, dtype=np.uint8)
    status = np.full(nc, SENT, dtype=np.int32)
    consumed = np.full(nc, SENT, dtype=np.uint64)
    n = ctypes.c_size_t(12345)
    rc = L.lib().l7m_http_stream_frame(
        wire.ctypes.data, wire.nbytes, coffs.ctypes.data, nc, None if meta is None else meta.ctypes.data,
        offs.ctypes.data if with_arrays else None, hconn.ctypes.data if with_arrays else None,
        hmeta.ctypes.data if with_arrays and meta is not None else None, cap, status.ctypes.data,
        consumed.ctypes.data, ctypes.byref(n))
    return rc, n.value, offs, hconn, hmeta, status, consumed


def test_http_capacity_contract(http_fuzz):
    conns, metas, (e_offs, e_conn, _, e_status, e_consumed) = http_fuzz
    wire, coffs = L.join_conns(conns)
    meta = W.meta_array(metas)
    n = len(e_conn)
    rc, got, *_ , status, consumed = _http_call(wire, coffs, 0, with_arrays=False)  # the sizing call
    assert (rc, got) == (L.L7M_ENOMEM, n)
    assert np.array_equal(status, e_status) and np.array_equal(consumed, e_consumed)
    rc, got, offs, hconn, hmeta, status, consumed = _http_call(wire, coffs, n, meta=meta)  # exact capacity
    assert (rc, got) == (L.L7M_OK, n)
    assert np.array_equal(offs, e_offs) and np.array_equal(hconn, e_conn)
    assert hmeta.tobytes() == meta[e_conn].tobytes()
    rc, got, offs, hconn, hmeta, status, consumed = _http_call(wire, coffs, n - 1, meta=meta)  # one short
    assert (rc, got) == (L.L7M_ENOMEM, n)
    assert np.all(offs == SENT) and np.all(hconn == SENT) and np.all(hmeta == SENT)
    assert np.array_equal(status, e_status) and np.array_equal(consumed, e_consumed)


def _kafka_call(wire, coffs, cap_recs, cap_bytes, with_arrays=True, ids=None):
    nc = len(coffs) - 1
    arena = np.full(cap_bytes, SENT, dtype=np.uint8)
    offs = np.full(cap_recs, SENT, dtype=np.uint64)
    rconn = np.full(cap_recs, SENT, dtype=np.uint32)
    sids = np.full(cap_recs, SENT, dtype=np.uint32)
    status = np.full(nc, SENT, dtype=np.int32)
    consumed = np.full(nc, SENT, dtype=np.uint64)
    n, nb = ctypes.c_size_t(12345), ctypes.c_size_t(12345)
    rc = L.lib().l7m_kafka_stream_frame(
        wire.ctypes.data, wire.nbytes, coffs.ctypes.data, nc, None if ids is None else ids.ctypes.data,
        arena.ctypes.data if with_arrays and cap_bytes else None, cap_bytes, offs.ctypes.data if with_arrays else None,
        rconn.ctypes.data if with_arrays else None, sids.ctypes.data if with_arrays and ids is not None else None,
        cap_recs, status.ctypes.data, consumed.ctypes.data, ctypes.byref(n), ctypes.byref(nb))
    return rc, n.value, nb.value, arena, offs, rconn, sids, status, consumed


def test_kafka_capacity_contract(kafka_fuzz):
    conns, ids, (e_arena, e_offs, e_conn, e_ids, e_status, e_consumed, _) = kafka_fuzz
    wire, coffs = L.join_conns(conns)
    n, nb = len(e_conn), len(e_arena)
    rc, got, gotb, *_, status, consumed = _kafka_call(wire, coffs, 0, 0, with_arrays=False)  # the sizing call
    assert (rc, got, gotb) == (L.L7M_ENOMEM, n, nb)
    assert np.array_equal(status, e_status) and np.array_equal(consumed, e_consumed)
    rc, got, gotb, arena, offs, rconn, sids, status, consumed = _kafka_call(wire, coffs, n, nb, ids=ids)
    assert (rc, got, gotb) == (L.L7M_OK, n, nb)
    assert arena.tobytes() == e_arena and np.array_equal(offs, e_offs) and np.array_equal(rconn, e_conn)
    assert np.array_equal(sids, e_ids)
    for cap_recs, cap_bytes in ((n - 1, nb), (n, nb - 1)):  # one record short, one byte short
        rc, got, gotb, arena, offs, rconn, sids, status, consumed = _kafka_call(wire, coffs, cap_recs, cap_bytes, ids=ids)
        assert (rc, got, gotb) == (L.L7M_ENOMEM, n, nb)
        assert np.all(arena == SENT) and np.all(offs == SENT) and np.all(rconn == SENT) and np.all(sids == SENT)
        assert np.array_equal(status, e_status) and np.array_equal(consumed, e_consumed)


def test_bad_conn_offs_are_refused():
    wire = np.frombuffer(S.G, dtype=np.uint8)
    for coffs in ([0, 20], [5, 2], [0, 10, 5], [20, 20]):
        for fn in (L.frame_http_streams, L.frame_kafka_streams):
            with pytest.raises(L.L7Error) as e:
                fn((wire, np.array(coffs, dtype=np.uint64)))
            assert e.value.code == L.L7M_EINVAL
    # offsets that start inside the wire are fine
    _, offs, _, _, status, _ = L.frame_http_streams((np.frombuffer(b"xx" + S.G, dtype=np.uint8),
                                                    np.array([2, 21], dtype=np.uint64)))
    assert offs.tolist() == [2, 21] and status.tolist() == [S.OK]


def test_bounds_are_met():
    """Constructed inputs reach the three bounds exactly."""
    assert L.http_stream_heads_bound(0, 0) == 0 and L.kafka_stream_bounds(0) == (0, 0)
    least = b"G / HTTP/1.1\r\n\r\n"  # the smallest complete head: 16 bytes
    conns = [least * 5 + b"G", least * 2 + b"\r", b"x"]  # 7 whole heads and three connections with a tail
    _, offs, hconn, _, status, _ = L.frame_http_streams(conns)
    total = sum(len(c) for c in conns)
    assert total // 16 == 7
    assert len(hconn) == L.http_stream_heads_bound(total, len(conns)) == 10
    conns = [S.frame(8) * 11]  # 12-byte frames
    arena, offs, _, _, _, _ = L.frame_kafka_streams(conns)
    assert len(offs) == L.kafka_stream_bounds(132)[0] == 11
    one = [S.frame(9)]  # a 13-byte frame takes 16 arena bytes
    arena, offs, _, _, _, _ = L.frame_kafka_streams(one)
    assert arena.shape[0] == L.kafka_stream_bounds(13)[1] == 16


def test_kafka_arena_records(kafka_fuzz):
    """Records are dword aligned, padded with zeros and byte-equal to the frames."""
    conns, ids, expected = kafka_fuzz
    recs = expected[6]
    arena, offs, _, _, _, _ = L.frame_kafka_streams(conns, ids)
    assert len(recs) == len(offs) > 1000
    assert not (offs % 4).any()
    ends = np.append(offs[1:], np.uint64(arena.shape[0] if len(recs) else 0))
    lens = set()
    for r, o, e in zip(recs, offs.tolist(), ends.tolist()):
        assert arena[o:o + len(r)].tobytes() == r
        assert e - o == (len(r) + 3) // 4 * 4 and not arena[o + len(r):e].any()
        assert struct.unpack_from(">i", r)[0] == len(r) - 4
        lens.add(len(r) % 4)
    assert lens == {0, 1, 2, 3}
    parena, poffs = L.pack_records(recs)
    assert parena.tobytes() == arena.tobytes() and np.array_equal(poffs, offs)
