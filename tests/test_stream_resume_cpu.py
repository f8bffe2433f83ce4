"""Host side of streaming across calls (l7m_http_stream_frame_resume,
l7m_stream_carry): against the pure-Python framer and carry of
tests/stream_resume_cases.py, and against the one-shot framers on the uncut
connections (split invariance)."""
import ctypes
import os

import numpy as np
import pytest

import stream_cases as S
import stream_resume_cases as R
from cilium_amd import l7match as L

SENT = 0xA5


def sent(n, dtype):
    """n elements with every byte SENT."""
    return np.full(n * np.dtype(dtype).itemsize, SENT, dtype=np.uint8).view(dtype)


ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def decoded_heads(rounds_out, n_conns):
    """Per connection the (wire status, record bytes) of every head emitted over the
    rounds, each decoded from the slice as emitted (trailing foreign bytes included)."""
    per = [[] for _ in range(n_conns)]
    for conns, offs, hconn, *_ in rounds_out:
        wire, _ = L.join_conns(conns)
        arena, roffs, wstatus = L.decode_http_wire((wire, offs))
        ends = np.append(roffs[1:], np.uint64(arena.shape[0] if len(roffs) else 0))
        for i, c in enumerate(hconn.tolist()):
            per[c].append((int(wstatus[i]), arena[int(roffs[i]):int(ends[i])].tobytes()))
    return per


def one_shot_heads(conns):
    """The same of the one-shot framer, without a final EPARTIAL_HEAD slice; and its statuses."""
    wire, offs, hconn, _, status, _ = L.frame_http_streams(conns)
    arena, roffs, wstatus = L.decode_http_wire((wire, offs))
    ends = np.append(roffs[1:], np.uint64(arena.shape[0] if len(roffs) else 0))
    per = [[] for _ in range(len(conns))]
    for i, c in enumerate(hconn.tolist()):
        per[c].append((int(wstatus[i]), arena[int(roffs[i]):int(ends[i])].tobytes()))
    for c in range(len(conns)):
        if status[c] == S.EPARTIAL_HEAD:
            assert per[c][-1][0] == L.WIRE_EINCOMPLETE
            per[c].pop()
    return per, status


@pytest.fixture(scope="module")
def split_rounds():
    a, b, whole = R.split_set()
    return [list(a), list(b)], list(whole)


@pytest.fixture(scope="module")
def split_host(split_rounds):
    return R.http_loop(split_rounds[0], R.host_frame, R.host_carry)


def test_constants_and_abi():
    assert L.lib().l7m_abi_version() == 4
    assert (L.STREAM_MODE_HEAD, L.STREAM_MODE_BODY, L.STREAM_MODE_CHUNK_DATA, L.STREAM_MODE_CHUNK_LINE,
            L.STREAM_MODE_TRAILER, L.STREAM_MODE_CLOSED) == (R.HEAD, R.BODY, R.CHUNK_DATA, R.CHUNK_LINE, R.TRAILER,
                                                             R.CLOSED)
    assert L.STREAM_STATE_DTYPE == R.STATE_DTYPE and L.STREAM_STATE_DTYPE.itemsize == 16
    with open(os.path.join(ROOT, "include", "l7match.h")) as f:
        header = f.read()
    for name, value in (("HEAD", 0), ("BODY", 1), ("CHUNK_DATA", 2), ("CHUNK_LINE", 3), ("TRAILER", 4), ("CLOSED", 5)):
        assert "#define L7M_STREAM_MODE_%s %d " % (name, value) in header
    for name in ("l7m_http_stream_frame_resume", "l7m_http_stream_frame_resume_device", "l7m_stream_carry",
                 "l7m_stream_carry_device", "l7m_stream_carry_bound"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.lib(), name)
    assert L.stream_carry_bound(7, 9) == 16


def test_split_set_equals_the_python_reference(split_rounds, split_host):
    """Both rounds of every two-piece split: slices, head_conn, status, consumed, state out, next wire."""
    R.assert_rounds_equal(split_host, R.http_loop(split_rounds[0], R.py_frame, R.carry))
    assert len(split_rounds[1]) > 3000


def test_split_invariance(split_rounds, split_host):
    """The heads of both rounds together are the one-shot framer's on the whole connection (decoded
    from the slices as emitted: prefix stability), round 2's status is the one-shot's, none twice."""
    rounds, whole = split_rounds
    got = decoded_heads(split_host, len(whole))
    exp, status = one_shot_heads(whole)
    for c in range(len(whole)):
        assert got[c] == exp[c], (c, rounds[0][c], rounds[1][c])
    assert np.array_equal(split_host[1][3], status)
    refused = sum(1 for heads in got for st, _ in heads if st < 0)
    assert refused > 100 and sum(len(h) for h in got) > 3000


def test_head_metadata_follows_the_connection():
    import http_wire_cases as W
    conns = S.http_table_conns()
    metas = W.metas_for(len(conns))
    _, _, hconn, hmeta, _, _, _ = L.frame_http_streams_resume(conns, None, W.meta_array(metas))
    assert hmeta.tobytes() == W.meta_array(metas)[hconn].tobytes() and len(hconn) > 50


def _fuzz_loop_checks(frame, carry_fn):
    conns, rounds = R.fuzz_http_rounds()
    assert len(rounds[0]) < len(rounds[1]) == len(conns)  # some connections are opened in round 2
    got = R.http_loop(rounds, frame, carry_fn)
    R.assert_rounds_equal(got, R.http_loop(rounds, R.py_frame, R.carry))
    heads = decoded_heads(got, len(conns))
    exp, status = one_shot_heads(conns)
    assert heads == exp
    assert np.array_equal(got[-1][3], status)
    modes = {m for r in got[:-1] for _, m, _ in r[5]}
    assert modes == set(range(6))
    return got


def test_http_fuzz_three_rounds():
    _fuzz_loop_checks(R.host_frame, R.host_carry)


def kafka_loop(rounds, frame, carry_fn):
    """-> ([records as bytes], [rec_conn], final status) of the one-shot framer with carry.  The
    framer keeps no state, so the caller does what the contract asks of it: a connection's final
    status is the one that ended it, and from then on the caller, which closes it, supplies no
    more bytes for it (with bytes the carry would revive it mid-stream); else the last round's."""
    conns, recs, rconn = list(rounds[0]), [], []
    final = np.zeros(len(rounds[-1]), dtype=np.int32)
    ended = np.zeros(len(rounds[-1]), dtype=bool)
    for r in range(len(rounds)):
        arena, offs, rc, status, consumed = frame(conns)
        live = ~ended[:len(conns)]
        final[:len(conns)][live] = status[live]
        ended[:len(conns)] |= ~np.isin(status, R.OPEN)
        for i, o in enumerate(offs.tolist()):
            size = int.from_bytes(arena[o:o + 4].tobytes(), "big")
            recs.append(arena[o:o + 4 + size].tobytes())
        rconn += rc.tolist()
        if r + 1 < len(rounds):
            segs = [b"" if c < len(conns) and ended[c] else seg for c, seg in enumerate(rounds[r + 1])]
            conns, _ = carry_fn(conns, status, consumed, segs, None)
            assert not any(conns[c] for c in np.flatnonzero(ended))
    return recs, rconn, final


def _host_kafka_frame(conns):
    arena, offs, rconn, _, status, consumed = L.frame_kafka_streams(conns)
    return arena, offs, rconn, status, consumed


def check_kafka_loop(frame, carry_fn):
    conns, rounds = R.fuzz_kafka_rounds()
    assert len(rounds[0]) < len(rounds[1]) == len(conns)
    recs, rconn, status = kafka_loop(rounds, frame, carry_fn)
    _, _, e_conn, _, e_status, _, e_recs = S.frame_kafka(conns)
    # the rounds emit a connection's records in order, but round by round: order by connection (stable)
    order = np.argsort(np.array(rconn, dtype=np.int64), kind="stable")
    assert [recs[i] for i in order] == e_recs and np.array_equal(np.array(rconn)[order], e_conn)
    assert np.array_equal(status, e_status)
    assert len(recs) > 1000


def test_kafka_ended_connection_revives_with_new_bytes():
    """Without state the carry remembers nothing: the contract leaves closing to the caller."""
    conns = [S.frame(7), S.frame(8)]
    _, _, _, _, status, consumed = L.frame_kafka_streams(conns)
    assert status.tolist() == [S.EBADSIZE, S.OK]
    nxt, _ = R.host_carry(conns, status, consumed, [S.frame(9), b""])
    assert nxt == [b"", b""]  # ended: its segment of this round is dropped too
    _, _, _, _, status, consumed = L.frame_kafka_streams(nxt)
    assert status.tolist() == [S.OK, S.OK]  # the empty connection reports OK ...
    nxt, _ = R.host_carry(nxt, status, consumed, [S.frame(9), b""])
    assert nxt == [S.frame(9), b""]  # ... so bytes supplied after that are framed: the caller must not


def test_kafka_fuzz_three_rounds():
    check_kafka_loop(_host_kafka_frame, R.host_carry)
    # and the carry itself against the Python carry, round by round
    conns, rounds = R.fuzz_kafka_rounds()
    cur = list(rounds[0])
    for r in range(len(rounds) - 1):
        _, _, _, _, status, consumed, _ = S.frame_kafka(cur)
        nxt, _ = R.host_carry(cur, status, consumed, rounds[r + 1])
        assert nxt == R.carry(cur, status, consumed, rounds[r + 1])[0]
        cur = nxt


def test_bodies_never_enter_the_next_wire():
    head = S.req(b"Content-Length: 1000000000\r\n")
    conns = [head, S.G]
    _, offs, hconn, _, status, consumed, state = L.frame_http_streams_resume(conns)
    assert hconn.tolist() == [0, 1] and status.tolist() == [S.EPARTIAL_BODY, S.OK]
    assert consumed.tolist() == [len(head), 19]
    assert R.state_tuples(state) == [(10 ** 9, R.BODY, 0), R.FRESH]
    (wire, noffs), out = L.carry_streams(conns, status, consumed, [b"x" * 100, S.G[:7]], state)
    assert noffs.tolist() == [0, 0, 7] and wire.tobytes() == S.G[:7]
    assert R.state_tuples(out) == [(10 ** 9 - 100, R.BODY, 0), R.FRESH]
    assert R.state_tuples(state) == [(10 ** 9, R.BODY, 0), R.FRESH]  # the caller's array is not touched
    # the rest of the body in pieces, then the next request: framed without ever holding the body
    _, _, hconn, _, status, _, out2 = L.frame_http_streams_resume((wire, noffs), out)
    assert status.tolist() == [S.EPARTIAL_BODY, S.EPARTIAL_HEAD] and len(hconn) == 0
    out2["left"][0] = 3
    (wire, noffs), out3 = L.carry_streams((wire, noffs), status, np.array([0, 0], dtype=np.uint64),
                                          [b"xyz" + S.G, S.G[7:]], out2)
    assert wire.tobytes() == S.G + S.G and R.state_tuples(out3) == [R.FRESH, R.FRESH]


def _frame_call(wire, coffs, cap, states, with_arrays=True, alias=False):
    nc = len(coffs) - 1
    offs = sent(cap + 1, np.uint64)
    hconn = sent(cap, np.uint32)
    status = sent(nc, np.int32)
    consumed = sent(nc, np.uint64)
    sin = R.state_array(states)
    sout = sin if alias else sent(nc, R.STATE_DTYPE)
    n = ctypes.c_size_t(12345)
    rc = L.lib().l7m_http_stream_frame_resume(
        wire.ctypes.data, wire.nbytes, coffs.ctypes.data, nc, None, offs.ctypes.data if with_arrays else None,
        hconn.ctypes.data if with_arrays else None, None, cap, status.ctypes.data, consumed.ctypes.data,
        ctypes.byref(n), sin.ctypes.data, sout.ctypes.data)
    return rc, n.value, offs, hconn, status, consumed, R.state_tuples(sout)


def test_frame_capacity_contract_and_aliasing(split_rounds, split_host):
    """Round 2 of the split set (every mode enters): sizing call, exact, one head short, aliased state."""
    conns2, states_in = split_host[1][0], split_host[1][6]
    e_offs, e_conn, _, e_status, e_consumed, e_out = R.resume_http(conns2, states_in)
    wire, coffs = L.join_conns(conns2)
    n = len(e_conn)
    assert n > 1000
    for cap, arrays, alias in ((0, False, False), (n, True, False), (n - 1, True, False), (n, True, True),
                               (n - 1, True, True)):
        rc, got, offs, hconn, status, consumed, out = _frame_call(wire, coffs, cap, states_in, arrays, alias)
        assert got == n and rc == (L.L7M_OK if cap == n else L.L7M_ENOMEM)
        assert np.array_equal(status, e_status) and np.array_equal(consumed, e_consumed) and out == e_out
        if cap == n:
            assert np.array_equal(offs, e_offs) and np.array_equal(hconn, e_conn)
        else:
            assert np.all(offs.view(np.uint8) == SENT) and np.all(hconn.view(np.uint8) == SENT)


def test_closed_state_repeats_its_status():
    states = [(0, R.CLOSED, S.EBADCHUNK), (0, R.CLOSED, S.TUNNEL), R.FRESH, (7, 9, -44)]
    conns = [S.G, b"", S.G, S.G]
    offs, hconn, status, consumed, out = R.host_frame(conns, states)
    assert status.tolist() == [S.EBADCHUNK, S.TUNNEL, S.OK, -44]
    assert hconn.tolist() == [2] and offs.tolist() == [19, 57]
    assert consumed.tolist() == [19, 0, 19, 19] and out == states
    e = R.resume_http(conns, states)
    assert np.array_equal(offs, e[0]) and np.array_equal(status, e[3]) and np.array_equal(consumed, e[4]) and out == e[5]
    nxt, out = R.host_carry(conns, status, consumed, [b"a", b"b", b"c", b"d"], out)
    assert nxt == [b"", b"", b"c", b""] and out == states


def test_fresh_whole_connections_equal_the_one_shot():
    """All-zero state: the one-shot's answer apart from the documented differences."""
    conns = S.http_table_conns() + S.fuzz_http_conns()
    _, o_offs, o_conn, _, o_status, o_consumed = L.frame_http_streams(conns)
    _, offs, hconn, _, status, consumed, out = L.frame_http_streams_resume(conns)
    assert np.array_equal(status, o_status)
    coffs = S.conn_offs(conns)
    # the slices: the one-shot's without the partial head each EPARTIAL_HEAD connection ends with
    last = np.searchsorted(o_conn, np.arange(len(conns)), side="right") - 1
    drop = last[o_status == S.EPARTIAL_HEAD]
    keep = np.ones(len(o_conn), dtype=bool)
    keep[drop] = False
    assert np.array_equal(hconn, o_conn[keep]) and np.array_equal(offs[:-1], o_offs[:-1][keep])
    assert offs[-1] == coffs[-1]
    # consumed: the one-shot's unless a body was cut (then past the head, into the body)
    cut = (status == S.EPARTIAL_BODY) | (status == S.EBADCHUNK)
    assert np.array_equal(consumed[~cut], o_consumed[~cut])
    assert np.all(consumed[cut] > o_consumed[cut])
    modes = np.array([m for _, m, _ in R.state_tuples(out)])
    closing = ~np.isin(status, R.OPEN)
    assert np.all(modes[closing] == R.CLOSED) and np.all(modes[~closing] != R.CLOSED)
    assert np.all(modes[status == S.OK] == R.HEAD)


def _carry_call(conns, status, consumed, segs, states, cap, with_outputs=True, coffs=None, soffs=None,
                n_prev=None):
    wire, co = L.join_conns(conns)
    seg, so = L.join_conns(segs)
    coffs = co if coffs is None else np.array(coffs, dtype=np.uint64)
    soffs = so if soffs is None else np.array(soffs, dtype=np.uint64)
    n_prev = len(coffs) - 1 if n_prev is None else n_prev
    nc = len(soffs) - 1
    status = np.ascontiguousarray(status, dtype=np.int32)
    consumed = np.ascontiguousarray(consumed, dtype=np.uint64)
    st = None if states is None else R.state_array(states)
    nwire = sent(cap, np.uint8)
    noffs = sent(nc + 1, np.uint64)
    need = ctypes.c_uint64(12345)
    rc = L.lib().l7m_stream_carry(
        wire.ctypes.data, wire.nbytes, coffs.ctypes.data, n_prev, status.ctypes.data, consumed.ctypes.data,
        seg.ctypes.data, seg.nbytes, soffs.ctypes.data, nc, None if st is None else st.ctypes.data,
        nwire.ctypes.data if with_outputs else None, cap, noffs.ctypes.data if with_outputs else None,
        ctypes.byref(need))
    return rc, need.value, nwire, noffs, None if st is None else R.state_tuples(st)


def test_carry_capacity_contract(split_rounds, split_host):
    rounds, _ = split_rounds
    conns, _, _, status, consumed, states, _ = split_host[0]
    e_next, e_states = R.carry(conns, status, consumed, rounds[1], states)
    total = sum(len(x) for x in e_next)
    assert e_states != states and total > 10000
    rc, need, _, _, st = _carry_call(conns, status, consumed, rounds[1], states, 0, with_outputs=False)
    assert (rc, need) == (L.L7M_ENOMEM, total) and st == states  # the sizing call
    rc, need, nwire, noffs, st = _carry_call(conns, status, consumed, rounds[1], states, total)
    assert (rc, need) == (L.L7M_OK, total) and st == e_states
    assert nwire.tobytes() == b"".join(e_next) and np.array_equal(noffs, S.conn_offs(e_next))
    rc, need, nwire, noffs, st = _carry_call(conns, status, consumed, rounds[1], states, total - 1)
    assert (rc, need) == (L.L7M_ENOMEM, total) and st == states
    assert np.all(nwire == SENT) and np.all(noffs.view(np.uint8) == SENT)
    # a sizing call that fits (nothing to carry) still writes nothing but the total
    big = [(10, R.BODY, 0)]
    rc, need, _, _, st = _carry_call([b""], [S.EPARTIAL_BODY], [0], [b"abc"], big, 0, with_outputs=False)
    assert (rc, need) == (L.L7M_OK, 0) and st == big
    assert L.stream_carry_bound(len(b"".join(conns)), len(b"".join(rounds[1]))) >= total


def test_carry_refuses_bad_input():
    conns, segs = [S.G, S.G], [b"ab", b"cd", b"ef"]
    ok = dict(conns=conns, status=[0, 0], consumed=[19, 3], segs=segs, states=None, cap=64)
    assert _carry_call(**ok)[0] == L.L7M_OK
    for bad in (dict(coffs=[0, 19, 39]), dict(coffs=[5, 2, 38]), dict(coffs=[0, 20, 19]), dict(soffs=[0, 2, 4, 7]),
                dict(soffs=[0, 3, 2, 6]), dict(soffs=[7, 7, 7, 7]), dict(consumed=[20, 0]), dict(consumed=[0, 1 << 40]),
                dict(n_prev=4)):
        rc, need, nwire, noffs, _ = _carry_call(**{**ok, **bad})
        assert rc == L.L7M_EINVAL, bad
        assert np.all(nwire == SENT) and np.all(noffs.view(np.uint8) == SENT)
    with pytest.raises(L.L7Error) as e:
        L.frame_http_streams_resume((np.frombuffer(S.G, dtype=np.uint8), np.array([0, 20], dtype=np.uint64)))
    assert e.value.code == L.L7M_EINVAL


def test_empty_batches():
    _, offs, hconn, _, status, _, out = L.frame_http_streams_resume([])
    assert offs.tolist() == [0] and hconn.shape == (0,) and out.shape == (0,)
    (wire, noffs), out = L.carry_streams([], [], [], [], None)
    assert wire.shape == (0,) and noffs.tolist() == [0] and out is None
    (wire, noffs), out = L.carry_streams([], [], [], [S.G, b""], R.state_array([R.FRESH] * 2))
    assert wire.tobytes() == S.G and noffs.tolist() == [0, 19, 19]
