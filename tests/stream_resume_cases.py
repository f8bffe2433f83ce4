"""Streaming across calls (DESIGN.md "Streaming across calls"): a resumable
HTTP framer and a carry written from the normative text, independent of the
C++ (the head grammar is http_wire_cases.parse_head), and the connection sets
of the CPU and GPU tests: every two-piece split of the table connections and
seeded three-round cuts of the fuzz sets.  Shared by tests/test_stream_resume_cpu.py,
tests/test_stream_resume_gpu.py and the stand-alone sanitizer program
(tests/cpp/stream_carry_asan.cc)."""
import functools
import struct

import numpy as np

import http_wire_cases as W
import stream_cases as S

HEAD, BODY, CHUNK_DATA, CHUNK_LINE, TRAILER, CLOSED = range(6)
STATE_DTYPE = np.dtype([("left", "<u8"), ("mode", "<i4"), ("status", "<i4")])
FRESH = (0, HEAD, 0)
OPEN = (S.OK, S.EPARTIAL_HEAD, S.EPARTIAL_BODY, S.EPARTIAL_FRAME)
MAX_SPLIT_CONN = 768
CR, LF = 0x0D, 0x0A


class _Partial(Exception):
    pass


class _Bad(Exception):
    pass


def _line(conn, p, first):
    """One CRLF-terminated line of free text from conn[p]; `first` has read up
    to the text.  -> index behind the LF."""
    n = len(conn)

    def at(i):
        if i >= n:
            raise _Partial
        return conn[i]

    q = first(at, p)
    while at(q) != CR:
        if conn[q] in (LF, 0):
            raise _Bad
        q += 1
    if at(q + 1) != LF:
        raise _Bad
    return q + 2


def _size_line(conn, p):
    """-> (chunk size, index behind the line)."""
    size = [0]

    def first(at, q):
        while at(q) in S.HEX:
            if q - p == 15:
                raise _Bad  # a 16th digit
            q += 1
        if q == p:
            raise _Bad
        size[0] = int(conn[p:q], 16)
        if conn[q] == ord(";"):
            return q + 1
        if conn[q] != CR:
            raise _Bad
        return q

    return size, _line(conn, p, first)


def _trailer_line(conn, p):
    def first(at, q):
        while at(q) in W.TCHAR:
            q += 1
        if q == p or conn[q] != ord(":"):
            raise _Bad
        return q + 1

    return _line(conn, p, first)


def resume_http_conn(conn: bytes, state=FRESH):
    """-> (head starts, status, consumed, state out) of one connection entered in `state`
    = (left, mode, status)."""
    left, mode, status = state
    if not 0 <= mode < CLOSED:
        return [], status, len(conn), state
    starts, p, n = [], 0, len(conn)

    def close(code, consumed):
        return starts, code, consumed, (0, CLOSED, code)

    def pause(code, consumed, mode, left=0):
        return starts, code, consumed, (left, mode, 0)

    while True:
        if mode == HEAD:
            if p == n:
                return pause(S.OK, p, HEAD)
            try:
                used, method, _, _, headers = W.parse_head(conn[p:])
            except W.Refused as e:
                if e.code == W.EINCOMPLETE:
                    return pause(S.EPARTIAL_HEAD, p, HEAD)
                starts.append(p)
                return close(S.EBADHEAD, p)
            starts.append(p)
            if method == b"CONNECT":
                return close(S.TUNNEL, p + used)
            te = [v for k, v in headers if k == b"transfer-encoding"]
            cl = [v for k, v in headers if k == b"content-length"]
            if te and cl:
                return close(S.EAMBIGUOUS, p)
            if te:
                if len(te) != 1 or te[0].lower() != b"chunked":
                    return close(S.EBADTE, p)
                mode = CHUNK_LINE
            elif cl:
                if len(cl) != 1 or not 1 <= len(cl[0]) <= 18 or any(c not in b"0123456789" for c in cl[0]):
                    return close(S.EBADLENGTH, p)
                left = int(cl[0])
                if left:
                    mode = BODY
            p += used
        elif mode in (BODY, CHUNK_DATA):
            k = min(left, n - p)
            p, left = p + k, left - k
            if left:
                return pause(S.EPARTIAL_BODY, p, mode, left)
            if mode == BODY:
                mode = HEAD
                continue
            if n - p < 1 or (conn[p] == CR and n - p < 2):
                return pause(S.EPARTIAL_BODY, p, CHUNK_DATA)
            if conn[p:p + 2] != b"\r\n":
                return close(S.EBADCHUNK, p)
            p, mode = p + 2, CHUNK_LINE
        else:
            try:
                if mode == CHUNK_LINE:
                    size, q = _size_line(conn, p)
                    left = size[0]
                    mode = CHUNK_DATA if left else TRAILER
                elif p < n and conn[p] == CR:
                    if p + 1 >= n:
                        raise _Partial
                    if conn[p + 1] != LF:
                        raise _Bad
                    q, mode = p + 2, HEAD
                else:
                    q = _trailer_line(conn, p)
            except _Partial:
                return pause(S.EPARTIAL_BODY, p, mode)
            except _Bad:
                return close(S.EBADCHUNK, p)
            p = q


def state_array(states):
    a = np.zeros(len(states), dtype=STATE_DTYPE)
    for i, (left, mode, status) in enumerate(states):
        a[i] = (left, mode, status)
    return a


def state_tuples(a):
    return [(int(s["left"]), int(s["mode"]), int(s["status"])) for s in a]


def resume_http(conns, states=None, metas=None):
    """-> (head_offs u64[n + 1], head_conn u32[n], head metas or None, status i32, consumed u64, states out)."""
    offs, hconn, hmeta, status, consumed, out, base = [], [], [], [], [], [], 0
    for c, conn in enumerate(conns):
        starts, st, used, so = resume_http_conn(conn, FRESH if states is None else states[c])
        offs += [base + s for s in starts]
        hconn += [c] * len(starts)
        if metas is not None:
            hmeta += [metas[c]] * len(starts)
        status.append(st)
        consumed.append(used)
        out.append(so)
        base += len(conn)
    offs.append(base)
    return (np.array(offs, dtype=np.uint64), np.array(hconn, dtype=np.uint32), hmeta if metas is not None else None,
            np.array(status, dtype=np.int32).reshape(len(conns)),
            np.array(consumed, dtype=np.uint64).reshape(len(conns)), out)


def carry(conns, status, consumed, segs, states=None):
    """-> (the next round's connections, states out or None).  len(segs) >= len(conns)."""
    nxt, out = [], None if states is None else list(states)
    for c, seg in enumerate(segs):
        tail = conns[c][int(consumed[c]):] if c < len(conns) else b""
        st = int(status[c]) if c < len(conns) else S.OK
        left, mode, code = FRESH if states is None else states[c]
        if st not in OPEN or (states is not None and not 0 <= mode < CLOSED):
            nxt.append(b"")
        elif states is not None and mode in (BODY, CHUNK_DATA) and left > 0:
            k = min(left, len(seg))
            nxt.append(seg[k:])
            if k:
                left -= k
                out[c] = (left, HEAD if mode == BODY and left == 0 else mode, code)
        else:
            nxt.append(tail + seg)
    return nxt, out


# ---- connection sets ---------------------------------------------------------
# (name, connection): what the two-piece splits of stream_cases.HTTP_TABLE may
# miss: long trailers, several chunks, a body behind a chunked request.
RESUME_TABLE = [
    ("two chunks and two trailers", S.chunked(b"3\r\nabc\r\n10;x=y\r\n0123456789abcdef\r\n0\r\nA: 1\r\nBb: 22\r\n\r\n") + S.G),
    ("chunked then counted", S._CH + S._CL5 + S.G),
    ("counted body of 40", S.req(b"Content-Length: 40\r\n", b"x" * 40) + S.G),
    ("bad chunk after a good one", S.chunked(b"1\r\na\r\nZ\r\n")),
    ("bad trailer after a good one", S.chunked(b"0\r\nA: 1\r\nB\r\n\r\n")),
    ("tunnel after a body", S._CL5 + S._CONNECT + b"\x16\x03\x01"),
]


@functools.lru_cache(maxsize=None)
def split_set():
    """Every two-piece split of every table connection of at most MAX_SPLIT_CONN
    bytes (a longer one gives its first MAX_SPLIT_CONN bytes as a further
    connection): ([piece A], [piece B], [the whole]).  Every mode is left and
    resumed at every byte position of every table case."""
    base = S.http_table_conns() + [c for _, c in RESUME_TABLE]
    conns = [c for c in base if len(c) <= MAX_SPLIT_CONN] + [c[:MAX_SPLIT_CONN] for c in base if len(c) > MAX_SPLIT_CONN]
    a, b, whole = [], [], []
    for c in conns:
        for cut in range(len(c) + 1):
            a.append(c[:cut])
            b.append(c[cut:])
            whole.append(c)
    seen = {(mode, left == 0) for left, mode, _ in (resume_http_conn(x)[3] for x in a)}
    assert {m for m, _ in seen} == {HEAD, BODY, CHUNK_DATA, CHUNK_LINE, TRAILER, CLOSED}, seen
    assert (CHUNK_DATA, True) in seen and (CHUNK_DATA, False) in seen
    return a, b, whole


def cut_rounds(conns, rounds, seed, late_share=0.2):
    """Each connection cut at seeded uniformly random points into `rounds`
    pieces; the last `late_share` of the connections are opened in round 2
    (one piece fewer).  -> [round][connection] pieces (round 1 is shorter)."""
    rng = np.random.default_rng(seed)
    n = len(conns)
    n_late = int(n * late_share)
    out = [[] for _ in range(rounds)]
    for c, conn in enumerate(conns):
        first = 1 if c >= n - n_late else 0
        cuts = sorted(int(x) for x in rng.integers(0, len(conn) + 1, size=rounds - first - 1))
        edges = [0] + cuts + [len(conn)]
        for r in range(first, rounds):
            out[r].append(conn[edges[r - first]:edges[r - first + 1]])
    assert len(out[0]) == n - n_late and all(len(o) == n for o in out[1:])
    return out


FUZZ_ROUNDS = 3
FUZZ_CUT_SEED = 17


@functools.lru_cache(maxsize=None)
def fuzz_http_rounds():
    conns = S.fuzz_http_conns()
    return conns, cut_rounds(conns, FUZZ_ROUNDS, FUZZ_CUT_SEED)


@functools.lru_cache(maxsize=None)
def fuzz_kafka_rounds():
    conns = S.fuzz_kafka_conns()
    return conns, cut_rounds(conns, FUZZ_ROUNDS, FUZZ_CUT_SEED + 1)


def http_loop(rounds, frame, carry_fn, states0=None):
    """Runs frame / carry over the rounds' segments (states0: the states round 1 is
    entered with, default fresh).  frame(conns, states) ->
    (head_offs, head_conn, status, consumed, states out); carry_fn(conns, status,
    consumed, segs, states) -> (conns, states).  -> per round (conns, head_offs,
    head_conn, status, consumed, states out, states in)."""
    out, conns = [], list(rounds[0])
    states = list(states0) if states0 else [FRESH] * len(conns)
    for r in range(len(rounds)):
        entered = list(states)
        offs, hconn, status, consumed, states = frame(conns, states)
        out.append((conns, offs, hconn, status, consumed, states, entered))
        if r + 1 < len(rounds):
            segs = rounds[r + 1]
            states = list(states) + [FRESH] * (len(segs) - len(conns))
            conns, states = carry_fn(conns, status, consumed, segs, states)
    return out


def py_frame(conns, states):
    offs, hconn, _, status, consumed, out = resume_http(conns, states)
    return offs, hconn, status, consumed, out


def host_frame(conns, states, meta=None):
    """l7match.frame_http_streams_resume (the host function) in the shape http_loop takes."""
    from cilium_amd import l7match as L
    _, offs, hconn, hmeta, status, consumed, out = L.frame_http_streams_resume(conns, state_array(states), meta)
    return offs, hconn, status, consumed, state_tuples(out)


def host_carry(conns, status, consumed, segs, states=None):
    from cilium_amd import l7match as L
    (wire, offs), out = L.carry_streams(conns, status, consumed, segs, None if states is None else state_array(states))
    nxt = [wire[int(offs[c]):int(offs[c + 1])].tobytes() for c in range(len(segs))]
    return nxt, None if out is None else state_tuples(out)


def assert_rounds_equal(got, exp):
    assert len(got) == len(exp)
    for r, (g, e) in enumerate(zip(got, exp)):
        assert g[0] == e[0], "round %d: the wire" % r
        for k, what in ((1, "head_offs"), (2, "head_conn"), (3, "status"), (4, "consumed")):
            assert np.array_equal(g[k], e[k]), "round %d: %s" % (r, what)
        assert g[5] == e[5], "round %d: state out" % r


# ---- the sanitizer program's input --------------------------------------------
def dump(path, frame_cases, carry_cases):
    """frame_cases: (conns, states in); carry_cases: (conns, status, consumed,
    segs, states in or None).  Expected outputs come from the Python functions
    above.  Layout (little endian), per case:
      u32 kind (1 frame, 2 carry)
      frame: u32 n_conns, u64 conn_offs[n + 1], the wire, state in[n], i32 status[n],
             u64 consumed[n], state out[n], u64 n_heads, u64 head_offs[n_heads + 1], u32 head_conn[n_heads]
      carry: u32 n_prev, u32 n_conns, u32 has_state, u64 conn_offs[n_prev + 1], the wire,
             i32 status[n_prev], u64 consumed[n_prev], u64 seg_offs[n_conns + 1], the segments,
             state in[n_conns] (has_state), u64 next_bytes, u64 next_offs[n_conns + 1], the next wire,
             state out[n_conns] (has_state)."""
    with open(path, "wb") as f:
        for conns, states in frame_cases:
            offs, hconn, _, status, consumed, out = resume_http(conns, states)
            f.write(struct.pack("<II", 1, len(conns)) + S.conn_offs(conns).tobytes() + b"".join(conns))
            f.write(state_array(states).tobytes() + status.astype("<i4").tobytes() + consumed.astype("<u8").tobytes())
            f.write(state_array(out).tobytes() + struct.pack("<Q", len(hconn)) + offs.astype("<u8").tobytes() +
                    hconn.astype("<u4").tobytes())
        for conns, status, consumed, segs, states in carry_cases:
            nxt, out = carry(conns, status, consumed, segs, states)
            f.write(struct.pack("<IIII", 2, len(conns), len(segs), int(states is not None)))
            f.write(S.conn_offs(conns).tobytes() + b"".join(conns))
            f.write(np.asarray(status, dtype="<i4").tobytes() + np.asarray(consumed, dtype="<u8").tobytes())
            f.write(S.conn_offs(segs).tobytes() + b"".join(segs))
            if states is not None:
                f.write(state_array(states).tobytes())
            f.write(struct.pack("<Q", sum(len(x) for x in nxt)) + S.conn_offs(nxt).tobytes() + b"".join(nxt))
            if states is not None:
                f.write(state_array(out).tobytes())


def dump_cases():
    """The cases of the CPU tests as dump() takes them: both rounds of the split
    set, the three fuzz rounds of both protocols."""
    frames, carries = [], []
    a, b, _ = split_set()
    for rounds in ([list(a), list(b)], fuzz_http_rounds()[1]):
        conns, states = list(rounds[0]), [FRESH] * len(rounds[0])
        for r in range(len(rounds)):
            frames.append((conns, states))
            _, _, _, status, consumed, states = resume_http(conns, states)
            if r + 1 < len(rounds):
                segs = rounds[r + 1]
                states = states + [FRESH] * (len(segs) - len(conns))
                carries.append((conns, status, consumed, segs, states))
                conns, states = carry(conns, status, consumed, segs, states)
    rounds = fuzz_kafka_rounds()[1]
    conns = list(rounds[0])
    for r in range(len(rounds) - 1):
        _, _, _, _, status, consumed, _ = S.frame_kafka(conns)
        carries.append((conns, status, consumed, rounds[r + 1], None))
        conns, _ = carry(conns, status, consumed, rounds[r + 1])
    return frames, carries
