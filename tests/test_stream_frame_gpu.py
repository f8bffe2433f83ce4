"""Device side of stream framing: l7m_http_stream_frame_device and
l7m_kafka_stream_frame_device must reproduce the host framers byte for byte on
every output (tests/test_stream_frame_cpu.py holds those to the Python framer),
write nothing outside their outputs, and feed the decoder and the evaluator on
the same stream."""
import struct

import numpy as np
import pytest

import http_wire_cases as W
import stream_cases as S
from cilium_amd import l7match as L

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 64  # sentinel bytes in front of and behind every output
TILE = 256  # connections per workgroup tile (l7m_tile_scan.h kTileThreads)


class Out:
    """A device output of `nbytes` bytes, sentinel-filled, between two guard regions."""

    def __init__(self, nbytes):
        import torch
        self.nbytes = nbytes
        self.t = torch.full((2 * GUARD + (nbytes + 15) // 16 * 16,), SENT, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + GUARD

    def get(self, dtype=np.uint8):
        a = self.t.cpu().numpy()
        assert np.all(a[:GUARD] == SENT) and np.all(a[GUARD + self.nbytes:] == SENT), "a guard region was written"
        return a[GUARD:GUARD + self.nbytes].view(dtype)


def _upload(conns, shift):
    import torch
    wire, coffs = L.join_conns(conns)
    d_buf = torch.zeros(wire.nbytes + shift + 16, dtype=torch.uint8, device="cuda")
    d_wire = d_buf[shift:shift + wire.nbytes]
    if wire.nbytes:
        d_wire.copy_(torch.from_numpy(wire.copy()))
    return wire, coffs, d_buf, d_buf.data_ptr() + shift, torch.from_numpy(coffs.view(np.int64)).cuda()


def device_http(conns, metas=None, cap=None, shift=1):
    """-> (n_heads, head_offs, head_conn, head_meta bytes, status, consumed), every array whole
    (sentinels where nothing was written).  The wire sits `shift` bytes into its allocation."""
    import torch
    wire, coffs, keep, p_wire, d_coffs = _upload(conns, shift)
    nc = len(coffs) - 1
    d_meta = None if metas is None else torch.from_numpy(W.meta_array(metas).view(np.uint8)).cuda()
    if cap is None:
        cap = L.http_stream_heads_bound(wire.nbytes, nc)
    o_offs, o_conn, o_meta = Out(8 * (cap + 1)), Out(4 * cap), Out(12 * cap)
    o_status, o_consumed, o_n = Out(4 * nc), Out(8 * nc), Out(8)
    torch.cuda.synchronize()
    L.frame_http_streams_device(p_wire, wire.nbytes, d_coffs, nc, d_meta, o_offs.ptr, o_conn.ptr,
                                None if metas is None else o_meta.ptr, cap, o_status.ptr, o_consumed.ptr, o_n.ptr,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (int(o_n.get(np.uint64)[0]), o_offs.get(np.uint64), o_conn.get(np.uint32), o_meta.get(),
            o_status.get(np.int32), o_consumed.get(np.uint64))


def check_http(conns, metas=None, shift=1):
    _, h_offs, h_conn, h_meta, h_status, h_consumed = L.frame_http_streams(
        conns, None if metas is None else W.meta_array(metas))
    n, offs, hconn, hmeta, status, consumed = device_http(conns, metas, shift=shift)
    assert n == len(h_conn)
    assert np.array_equal(status, h_status) and np.array_equal(consumed, h_consumed)
    assert np.array_equal(offs[:n + 1], h_offs) and np.array_equal(hconn[:n], h_conn)
    assert np.all(offs[n + 1:].view(np.uint8) == SENT) and np.all(hconn[n:].view(np.uint8) == SENT)
    if metas is None:
        assert np.all(hmeta == SENT)
    else:
        assert hmeta[:12 * n].tobytes() == h_meta.tobytes() and np.all(hmeta[12 * n:] == SENT)
    return h_status, n


def device_kafka(conns, ids=None, cap_recs=None, cap_bytes=None, shift=1):
    """-> (n_recs, arena_bytes, arena, rec_offsets, rec_conn, src_identities, status, consumed)."""
    import torch
    wire, coffs, keep, p_wire, d_coffs = _upload(conns, shift)
    nc = len(coffs) - 1
    d_ids = None if ids is None else torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32).view(np.int32)).cuda()
    bound = L.kafka_stream_bounds(wire.nbytes)
    cap_recs = bound[0] if cap_recs is None else cap_recs
    cap_bytes = bound[1] if cap_bytes is None else cap_bytes
    o_arena, o_offs, o_conn, o_ids = Out(cap_bytes), Out(8 * cap_recs), Out(4 * cap_recs), Out(4 * cap_recs)
    o_status, o_consumed, o_n, o_nb = Out(4 * nc), Out(8 * nc), Out(8), Out(8)
    torch.cuda.synchronize()
    L.frame_kafka_streams_device(p_wire, wire.nbytes, d_coffs, nc, d_ids, o_arena.ptr, cap_bytes, o_offs.ptr,
                                 o_conn.ptr, None if ids is None else o_ids.ptr, cap_recs, o_status.ptr,
                                 o_consumed.ptr, o_n.ptr, o_nb.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (int(o_n.get(np.uint64)[0]), int(o_nb.get(np.uint64)[0]), o_arena.get(), o_offs.get(np.uint64),
            o_conn.get(np.uint32), o_ids.get(np.uint32), o_status.get(np.int32), o_consumed.get(np.uint64))


def check_kafka(conns, ids=None, shift=1):
    h_arena, h_offs, h_conn, h_ids, h_status, h_consumed = L.frame_kafka_streams(conns, ids)
    n, nb, arena, offs, rconn, sids, status, consumed = device_kafka(conns, ids, shift=shift)
    assert n == len(h_offs) and nb == (h_arena.shape[0] if n else 0)
    assert np.array_equal(status, h_status) and np.array_equal(consumed, h_consumed)
    assert np.array_equal(offs[:n], h_offs) and np.array_equal(rconn[:n], h_conn)
    assert arena[:nb].tobytes() == h_arena[:nb].tobytes()
    assert np.all(arena[nb:] == SENT)  # nothing past the total
    assert np.all(offs[n:].view(np.uint8) == SENT) and np.all(rconn[n:].view(np.uint8) == SENT)
    if ids is None:
        assert np.all(sids.view(np.uint8) == SENT)
    else:
        assert np.array_equal(sids[:n], h_ids) and np.all(sids[n:].view(np.uint8) == SENT)
    return h_status, n


@pytest.fixture(scope="module")
def http_fuzz():
    return S.fuzz_http_conns()


@pytest.fixture(scope="module")
def kafka_fuzz():
    return S.fuzz_kafka_conns()


def _ids(n, seed=3):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint32)


def test_http_table_matches_host(gpu):
    conns = S.http_table_conns()
    st, _ = check_http(conns, W.metas_for(len(conns)))
    assert len(set(st.tolist())) == 9  # every HTTP code
    check_http(conns)


def test_kafka_table_matches_host(gpu):
    conns = S.kafka_table_conns()
    st, _ = check_kafka(conns, _ids(len(conns)))
    assert set(st.tolist()) == {S.OK, S.EBADSIZE, S.EPARTIAL_FRAME}
    check_kafka(conns)


def test_http_fuzz_matches_host(gpu, http_fuzz):
    check_http(http_fuzz, W.metas_for(len(http_fuzz), seed=9))  # 600 connections: three tiles, the last partial


def test_kafka_fuzz_matches_host(gpu, kafka_fuzz):
    check_kafka(kafka_fuzz, _ids(len(kafka_fuzz)))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_connection_counts_match_host(gpu, http_fuzz, kafka_fuzz, n):
    """Wave and tile edges, and a scan over several tiles."""
    check_http(http_fuzz[40:40 + n], W.metas_for(n, seed=n))
    check_kafka(kafka_fuzz[40:40 + n], _ids(n, seed=n))


def test_many_tiles_match_host(gpu):
    """262,400 connections of one smallest head (frame) each: more tile sums than the scan has threads."""
    n = 1025 * TILE
    head = np.frombuffer(b"G / HTTP/1.1\r\n\r\n", dtype=np.uint8)
    conns = (np.tile(head, n), np.arange(n + 1, dtype=np.uint64) * 16)
    st, heads = check_http(conns)
    assert heads == n and not st.any()
    frame = np.frombuffer(S.frame(9), dtype=np.uint8)
    conns = (np.tile(frame, n), np.arange(n + 1, dtype=np.uint64) * 13)
    st, recs = check_kafka(conns)
    assert recs == n and not st.any()


def test_one_long_connection_matches_host(gpu, http_fuzz, kafka_fuzz):
    """300 pipelined requests in one connection, between two empty connections and a short one:
    the output spans tiles while its input is one lane."""
    good = [c for c in http_fuzz if c and S.frame_http_conn(c)[1] == S.OK]
    reqs = [S.G, S._CL5, S._CH] * 100
    conns = good[:TILE - 2] + [b"", b"".join(reqs), b"", S.G] + good[TILE:TILE + 10]
    st, n = check_http(conns, W.metas_for(len(conns)))
    assert st[TILE - 1] == S.OK and n > 300 + TILE
    frames = [S.frame(8 + k % 7, 0x30 + k % 10) for k in range(300)]
    conns = kafka_fuzz[:TILE - 2] + [b"", b"".join(frames), b"", S.frame(8)] + kafka_fuzz[TILE:TILE + 10]
    st, n = check_kafka(conns, _ids(len(conns)))
    assert st[TILE - 1] == S.OK and n > 300


def test_large_bodies_are_skipped(gpu):
    """A chunk of 70,000 data bytes and a counted body of 70,000: skipped by their size."""
    data = bytes(np.random.default_rng(5).integers(0, 256, size=70000, dtype=np.uint8))
    big_chunk = S.chunked(b"%x\r\n" % len(data) + data + b"\r\n0\r\n\r\n")
    counted = S.req(b"Content-Length: %d\r\n" % len(data), data)
    conns = [S.G + big_chunk + S.G, counted + S.G, counted[:-1], big_chunk[:-8], S.G]
    st, n = check_http(conns)
    assert st.tolist() == [S.OK, S.OK, S.EPARTIAL_BODY, S.EPARTIAL_BODY, S.OK] and n == 8
    conns = [S.frame(70000, 0x41) + S.frame(8), S.frame(8) + S.frame(70001, 0x42) + S.frame(9), S.frame(70000)[:-1]]
    st, n = check_kafka(conns)
    assert st.tolist() == [S.OK, S.OK, S.EPARTIAL_FRAME] and n == 5


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_wire_at_any_alignment_matches_host(gpu, http_fuzz, kafka_fuzz, shift):
    check_http(http_fuzz[:300], shift=shift)
    check_kafka(kafka_fuzz[:300], _ids(300), shift=shift)
    check_kafka(S.kafka_table_conns()[-2:], shift=shift)  # only whole frames: the copy's last unit ends the wire


def test_http_capacity_one_head_short(gpu, http_fuzz):
    _, h_offs, h_conn, _, h_status, h_consumed = L.frame_http_streams(http_fuzz)
    total = len(h_conn)
    metas = W.metas_for(len(http_fuzz))
    n, offs, hconn, hmeta, status, consumed = device_http(http_fuzz, metas, cap=total - 1)
    assert n == total
    assert np.all(offs.view(np.uint8) == SENT) and np.all(hconn.view(np.uint8) == SENT) and np.all(hmeta == SENT)
    assert np.array_equal(status, h_status) and np.array_equal(consumed, h_consumed)
    n, offs, hconn, hmeta, status, consumed = device_http(http_fuzz, metas, cap=total)  # exactly enough
    assert n == total and np.array_equal(offs, h_offs) and np.array_equal(hconn, h_conn)


def test_kafka_capacity_one_record_or_one_byte_short(gpu, kafka_fuzz):
    ids = _ids(len(kafka_fuzz))
    h_arena, h_offs, h_conn, h_ids, h_status, h_consumed = L.frame_kafka_streams(kafka_fuzz, ids)
    total, nbytes = len(h_offs), h_arena.shape[0]
    for cap_recs, cap_bytes in ((total - 1, nbytes), (total, nbytes - 1)):
        n, nb, arena, offs, rconn, sids, status, consumed = device_kafka(kafka_fuzz, ids, cap_recs, cap_bytes)
        assert (n, nb) == (total, nbytes)
        assert np.all(arena == SENT)
        for a in (offs, rconn, sids):
            assert np.all(a.view(np.uint8) == SENT)
        assert np.array_equal(status, h_status) and np.array_equal(consumed, h_consumed)
    n, nb, arena, offs, rconn, sids, status, consumed = device_kafka(kafka_fuzz, ids, total, nbytes)  # exactly enough
    assert (n, nb) == (total, nbytes) and arena.tobytes() == h_arena.tobytes()
    assert np.array_equal(offs, h_offs) and np.array_equal(rconn, h_conn) and np.array_equal(sids, h_ids)


def _readme_connections():
    """A few hundred connections of README-policy requests (workloads config 1), some with
    bodies, some ending in a cut or a refused head."""
    from cilium_amd import workloads as WL
    rng = np.random.default_rng(21)
    arena, offs = WL.requests(1, 0, 1500)
    wire, hoffs, st = L.encode_http_wire(arena, offs)
    heads = [wire[int(hoffs[i]):int(hoffs[i + 1])].tobytes() for i in range(len(offs)) if st[i] > 0]
    assert len(heads) > 1000
    conns, at = [], 0
    while at < len(heads):
        k = int(rng.integers(0, 9))
        parts = []
        for h in heads[at:at + k]:
            r = rng.random()
            if r < 0.2:
                body = bytes(rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8))
                h = h[:-2] + b"Content-Length: %d\r\n\r\n" % len(body) + body
            elif r < 0.3:
                h = h[:-2] + b"Transfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n0\r\n\r\n"
            parts.append(h)
        conn = b"".join(parts)
        r = rng.random()
        if r < 0.1 and conn:
            conn = conn[:int(rng.integers(1, len(conn)))]
        elif r < 0.2:
            conn += b"NOT A HEAD\r\n\r\n"
        conns.append(conn)
        at += k
    # a body cut short, a tunnel behind a request, and a smuggling attempt
    conns += [heads[0][:-2] + b"Content-Length: 10\r\n\r\nabc", heads[1] + S._CONNECT + b"\x16\x03",
              heads[2] + heads[3][:-2] + b"Content-Length: 1\r\nTransfer-Encoding: chunked\r\n\r\n0\r\n\r\n"]
    return conns


def test_http_frame_decode_eval_on_one_stream(gpu):
    import torch
    from cilium_amd import workloads as WL
    conns = _readme_connections()
    assert 200 < len(conns) < 1000
    rs = L.RuleSet.compile_http(WL.rules(1))
    # expected: host framer, host decoder, eval
    wire, h_offs, h_conn, _, h_status, _ = L.frame_http_streams(conns)
    h_arena, h_roffs, h_wstatus = L.decode_http_wire((wire, h_offs))
    exp = rs.eval(h_arena, h_roffs)
    assert len(set(h_status.tolist())) >= 4 and len(set(exp.tolist())) >= 3

    nc = len(conns)
    coffs = S.conn_offs(conns)
    cap = L.http_stream_heads_bound(wire.nbytes, nc)
    acap = (L.http_wire_arena_bound(wire.nbytes, cap) + 15) // 16 * 16
    d_wire = torch.from_numpy(wire.copy()).cuda()
    d_coffs = torch.from_numpy(coffs.view(np.int64)).cuda()
    d_hoffs = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
    d_hconn = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_cstatus = torch.zeros(nc, dtype=torch.int32, device="cuda")
    d_consumed = torch.zeros(nc, dtype=torch.int64, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_arena = torch.full((acap,), SENT, dtype=torch.uint8, device="cuda")
    d_roffs = torch.zeros(cap, dtype=torch.int64, device="cuda")
    d_wstatus = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_verd = torch.full((cap,), 12345, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        L.frame_http_streams_device(d_wire, wire.nbytes, d_coffs, nc, None, d_hoffs, d_hconn, None, cap, d_cstatus,
                                    d_consumed, d_n, s.cuda_stream)
        n = int(d_n.cpu()[0])  # the 8 bytes the decoder and the evaluator need on the host
        L.decode_http_wire_device(d_wire, wire.nbytes, d_hoffs, n, None, d_arena, acap, d_roffs, d_wstatus, d_total,
                                  s.cuda_stream)
        rs.eval_device(d_arena, acap, d_roffs, n, d_verd, None, s.cuda_stream)
    s.synchronize()
    assert n == len(h_conn)
    assert np.array_equal(d_cstatus.cpu().numpy(), h_status)
    assert np.array_equal(d_wstatus.cpu().numpy()[:n], h_wstatus)
    assert np.array_equal(d_verd.cpu().numpy()[:n], exp)


def _kafka_connections():
    """Config-3 requests grouped into connections with no padding, each with a source identity."""
    import selector_cases as SC
    from cilium_amd import workloads as WL
    entries, idmap = SC.random_map(11, n_rules=300, n_ids=12)
    arena, offs = WL.requests(3, 0, 2000, n_rules=300)
    frames = []
    for o in offs.tolist():
        size = struct.unpack_from(">i", arena, o)[0]
        frames.append(arena[o:o + 4 + size].tobytes())
    rng = np.random.default_rng(23)
    conns, at = [], 0
    while at < len(frames):
        k = int(rng.integers(0, 9))
        conns.append(b"".join(frames[at:at + k]))
        at += k
    return entries, idmap, conns, frames, SC.request_identities(13, len(conns), idmap)


def test_kafka_host_arena_evaluates_like_packed_records(gpu):
    """l7m_eval on the framer's arena gives the verdicts of l7m_eval on pack_records of the same frames."""
    entries, idmap, conns, frames, cids = _kafka_connections()
    rs = L.RuleSet.compile_kafka_map(entries, idmap)
    arena, offs, rconn, sids, status, _ = L.frame_kafka_streams(conns, cids)
    assert len(offs) == len(frames) and not status.any()
    p_arena, p_offs = L.pack_records(frames)
    exp = rs.eval(p_arena, p_offs, identities=cids[rconn])
    assert np.array_equal(rs.eval(arena, offs, identities=sids), exp)
    assert (exp >= 0).any() and (exp == -1).any()


def test_kafka_frame_eval_on_one_stream(gpu):
    import torch
    entries, idmap, conns, frames, cids = _kafka_connections()
    conns[5] = conns[5] + b"\0\0"  # one connection ends inside a size field
    rs = L.RuleSet.compile_kafka_map(entries, idmap)
    p_arena, p_offs = L.pack_records(frames)
    rec_conn = np.repeat(np.arange(len(conns)), [len(S.frame_kafka_conn(c)[0]) for c in conns])
    exp = rs.eval(p_arena, p_offs, identities=cids[rec_conn])

    wire, coffs = L.join_conns(conns)
    nc = len(conns)
    cap_recs, cap_bytes = L.kafka_stream_bounds(wire.nbytes)
    cap_bytes = (cap_bytes + 15) // 16 * 16
    d_buf = torch.zeros(wire.nbytes + 3, dtype=torch.uint8, device="cuda")
    d_wire = d_buf[3:]
    d_wire.copy_(torch.from_numpy(wire.copy()))
    d_coffs = torch.from_numpy(coffs.view(np.int64)).cuda()
    d_cids = torch.from_numpy(cids.view(np.int32)).cuda()
    d_arena = torch.full((cap_bytes + 64,), SENT, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(cap_recs, dtype=torch.int64, device="cuda")
    d_rconn = torch.zeros(cap_recs, dtype=torch.int32, device="cuda")
    d_sids = torch.zeros(cap_recs, dtype=torch.int32, device="cuda")
    d_cstatus = torch.zeros(nc, dtype=torch.int32, device="cuda")
    d_consumed = torch.zeros(nc, dtype=torch.int64, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_nb = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_verd = torch.full((cap_recs,), 12345, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        L.frame_kafka_streams_device(d_wire, wire.nbytes, d_coffs, nc, d_cids, d_arena, cap_bytes, d_offs, d_rconn,
                                     d_sids, cap_recs, d_cstatus, d_consumed, d_n, d_nb, s.cuda_stream)
        n = int(d_n.cpu()[0])
        rc = L.lib().l7m_eval_device_ids(rs._h, d_arena.data_ptr(), cap_bytes, d_offs.data_ptr(), n,
                                         d_sids.data_ptr(), d_verd.data_ptr(), None, s.cuda_stream, 0)
        assert rc == L.L7M_OK
    s.synchronize()
    assert n == len(frames)
    st = d_cstatus.cpu().numpy()
    assert st[5] == S.EPARTIAL_FRAME and not np.delete(st, 5).any()
    assert np.array_equal(d_rconn.cpu().numpy()[:n], rec_conn)
    assert np.array_equal(d_verd.cpu().numpy()[:n], exp)
    assert (exp >= 0).any() and (exp == -1).any()
