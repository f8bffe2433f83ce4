"""Connection byte streams for the stream-framing tests: a framer for both
protocols written from the rules in DESIGN.md ("Stream framing"), independent
of the C++ (the head grammar is http_wire_cases.parse_head), known-answer
tables and seeded fuzz sets.  Shared by the CPU and GPU tests and by the
stand-alone sanitizer program (tests/cpp/stream_frame_asan.cc)."""
import struct

import numpy as np

import http_wire_cases as W
import kafka_wire as K

OK, TUNNEL = 0, 1
(EBADHEAD, EPARTIAL_HEAD, EAMBIGUOUS, EBADTE, EBADLENGTH, EBADCHUNK, EPARTIAL_BODY, EPARTIAL_FRAME,
 EBADSIZE) = -1, -2, -3, -4, -5, -6, -7, -8, -9

KAFKA_MAX_FRAME = 100 * 65535  # maxParseBufSize
HEX = b"0123456789abcdefABCDEF"


class _Stop(Exception):
    def __init__(self, code):
        self.code = code


def _chunked_end(conn: bytes, q: int) -> int:
    """End of the chunked body that starts at conn[q]; raises _Stop(code)."""
    n = len(conn)

    def at(i):
        if i >= n:
            raise _Stop(EPARTIAL_BODY)
        return conn[i]

    def line_end(i):
        """conn[i] must be CR and conn[i + 1] LF; -> i + 2."""
        if at(i) != 0x0D or at(i + 1) != 0x0A:
            raise _Stop(EBADCHUNK)
        return i + 2

    def free_text(i):
        """Any byte but CR, LF and NUL up to a CR; -> its index."""
        while at(i) != 0x0D:
            if conn[i] in (0x0A, 0):
                raise _Stop(EBADCHUNK)
            i += 1
        return i

    while True:
        d0 = q
        while at(q) in HEX:
            q += 1
            if q - d0 > 15:
                raise _Stop(EBADCHUNK)
        if q == d0:
            raise _Stop(EBADCHUNK)
        size = int(conn[d0:q], 16)
        if conn[q] == ord(";"):
            q = free_text(q + 1)
        q = line_end(q)
        if size == 0:
            break
        if q + size > n:
            raise _Stop(EPARTIAL_BODY)
        q = line_end(q + size)
    while at(q) != 0x0D:
        n0 = q
        while at(q) in W.TCHAR:
            q += 1
        if q == n0 or conn[q] != ord(":"):
            raise _Stop(EBADCHUNK)
        q = line_end(free_text(q + 1))
    return line_end(q)


def frame_http_conn(conn: bytes):
    """-> (slice starts, status, consumed) of one connection."""
    starts, p, consumed = [], 0, 0
    while p < len(conn):
        starts.append(p)
        try:
            used, method, _, host, headers = W.parse_head(conn[p:])
        except W.Refused as e:
            return starts, (EPARTIAL_HEAD if e.code == W.EINCOMPLETE else EBADHEAD), consumed
        body = p + used
        if method == b"CONNECT":
            return starts, TUNNEL, body
        te = [v for k, v in headers if k == b"transfer-encoding"]
        cl = [v for k, v in headers if k == b"content-length"]
        if te and cl:
            return starts, EAMBIGUOUS, consumed
        if te:
            if len(te) != 1 or te[0].lower() != b"chunked":
                return starts, EBADTE, consumed
            try:
                p = _chunked_end(conn, body)
            except _Stop as e:
                return starts, e.code, consumed
        elif cl:
            if len(cl) != 1 or not 1 <= len(cl[0]) <= 18 or any(c not in b"0123456789" for c in cl[0]):
                return starts, EBADLENGTH, consumed
            if body + int(cl[0]) > len(conn):
                return starts, EPARTIAL_BODY, consumed
            p = body + int(cl[0])
        else:
            p = body
        consumed = p
    return starts, OK, consumed


def frame_http(conns, metas=None):
    """-> (head_offs u64[n + 1], head_conn u32[n], head metas or None, status i32, consumed u64)."""
    offs, hconn, hmeta, status, consumed, base = [], [], [], [], [], 0
    for c, conn in enumerate(conns):
        starts, st, used = frame_http_conn(conn)
        offs += [base + s for s in starts]
        hconn += [c] * len(starts)
        if metas is not None:
            hmeta += [metas[c]] * len(starts)
        status.append(st)
        consumed.append(used)
        base += len(conn)
    offs.append(base)
    return (np.array(offs, dtype=np.uint64), np.array(hconn, dtype=np.uint32), hmeta if metas is not None else None,
            np.array(status, dtype=np.int32).reshape(len(conns)), np.array(consumed, dtype=np.uint64).reshape(len(conns)))


def frame_kafka_conn(conn: bytes):
    """-> ([(start, frame bytes)], status, consumed) of one connection."""
    frames, p = [], 0
    while True:
        if len(conn) - p < 4:
            return frames, (OK if p == len(conn) else EPARTIAL_FRAME), p
        size = struct.unpack_from(">i", conn, p)[0]
        if size < 8 or size + 4 > KAFKA_MAX_FRAME:
            return frames, EBADSIZE, p
        if p + 4 + size > len(conn):
            return frames, EPARTIAL_FRAME, p
        frames.append((p, 4 + size))
        p += 4 + size


def frame_kafka(conns, identities=None):
    """-> (arena bytes, rec_offsets u64, rec_conn u32, src identities u32 or None, status i32,
    consumed u64, the frames as bytes objects)."""
    arena, offs, rconn, ids, status, consumed, recs = bytearray(), [], [], [], [], [], []
    for c, conn in enumerate(conns):
        frames, st, used = frame_kafka_conn(conn)
        for start, ln in frames:
            offs.append(len(arena))
            rconn.append(c)
            if identities is not None:
                ids.append(int(identities[c]))
            recs.append(conn[start:start + ln])
            arena += conn[start:start + ln] + b"\0" * (-ln % 4)
        status.append(st)
        consumed.append(used)
    return (bytes(arena), np.array(offs, dtype=np.uint64), np.array(rconn, dtype=np.uint32),
            np.array(ids, dtype=np.uint32) if identities is not None else None,
            np.array(status, dtype=np.int32).reshape(len(conns)),
            np.array(consumed, dtype=np.uint64).reshape(len(conns)), recs)


# ---- HTTP known answers ----------------------------------------------------
G = b"GET /a HTTP/1.1\r\n\r\n"  # 19 bytes, no body
_H = b"POST /p HTTP/1.1\r\nHost: h\r\n"


def req(lines=b"", body=b""):
    return _H + lines + b"\r\n" + body


def chunked(body, te=b"Transfer-Encoding: chunked\r\n"):
    return req(te, body)


_CL5 = req(b"Content-Length: 5\r\n", b"hello")
_CH = chunked(b"3;e\r\nabc\r\n0\r\nT: v\r\n\r\n")
_CH_HEAD = len(chunked(b""))
_CONNECT = b"CONNECT h:443 HTTP/1.1\r\nHost: h:443\r\n\r\n"

# (name, connection, status, slice starts, consumed)
HTTP_TABLE = [
    ("empty connection", b"", OK, [], 0),
    ("one head", G, OK, [0], 19),
    ("three heads", G * 3, OK, [0, 19, 38], 57),
    ("content-length 0", req(b"Content-Length: 0\r\n") + G, OK, [0, len(req(b"Content-Length: 0\r\n"))],
     len(req(b"Content-Length: 0\r\n")) + 19),
    ("length equal to the rest", _CL5, OK, [0], len(_CL5)),
    ("length then a request", _CL5 + G, OK, [0, len(_CL5)], len(_CL5) + 19),
    ("body that looks like a head", req(b"Content-Length: 19\r\n", G) + G, OK,
     [0, len(req(b"Content-Length: 19\r\n", G))], len(req(b"Content-Length: 19\r\n", G)) + 19),
    ("length one more than the rest", G + req(b"Content-Length: 6\r\n", b"hello"), EPARTIAL_BODY, [0, 19], 19),
    ("18 digits", req(b"Content-Length: 000000000000000005\r\n", b"hello"), OK, [0],
     len(req(b"Content-Length: 000000000000000005\r\n", b"hello"))),
    ("18 nines", req(b"Content-Length: 999999999999999999\r\n", b"hello"), EPARTIAL_BODY, [0], 0),
    ("19 digits", req(b"Content-Length: 0000000000000000005\r\n", b"hello"), EBADLENGTH, [0], 0),
    ("length +1", req(b"Content-Length: +1\r\n", b"h"), EBADLENGTH, [0], 0),
    ("length 1 2", req(b"Content-Length: 1 2\r\n", b"h"), EBADLENGTH, [0], 0),
    ("length empty", G + req(b"Content-Length:  \r\n", b"h"), EBADLENGTH, [0, 19], 19),
    ("length hex", req(b"Content-Length: 0x5\r\n", b"hello"), EBADLENGTH, [0], 0),
    ("two equal length lines", req(b"Content-Length: 5\r\nContent-Length: 5\r\n", b"hello"), EBADLENGTH, [0], 0),
    ("length ows stripped", req(b"Content-Length: \t5 \t\r\n", b"hello") + G, OK,
     [0, len(req(b"Content-Length: \t5 \t\r\n", b"hello"))], len(req(b"Content-Length: \t5 \t\r\n", b"hello")) + 19),
    ("names in mixed case", req(b"cOnTeNt-LeNgTh: 5\r\n", b"hello") + G, OK,
     [0, len(_CL5)], len(_CL5) + 19),
    ("te name in mixed case", req(b"TRANSFER-encoding: chunked\r\n", b"0\r\n\r\n"), OK, [0],
     len(req(b"TRANSFER-encoding: chunked\r\n", b"0\r\n\r\n"))),
    ("chunked in mixed case", chunked(b"0\r\n\r\n", b"Transfer-Encoding: ChUnKeD\r\n") + G, OK,
     [0, len(chunked(b"0\r\n\r\n"))], len(chunked(b"0\r\n\r\n")) + 19),
    ("gzip, chunked", chunked(b"0\r\n\r\n", b"Transfer-Encoding: gzip, chunked\r\n"), EBADTE, [0], 0),
    ("identity", chunked(b"", b"Transfer-Encoding: identity\r\n"), EBADTE, [0], 0),
    ("two transfer-encoding lines", chunked(b"0\r\n\r\n", b"Transfer-Encoding: chunked\r\nTransfer-Encoding: chunked\r\n"),
     EBADTE, [0], 0),
    ("transfer-encoding with content-length", G + req(b"Content-Length: 5\r\nTransfer-Encoding: chunked\r\n", b"0\r\n\r\n"),
     EAMBIGUOUS, [0, 19], 19),
    ("ambiguous before either value", req(b"Transfer-Encoding: gzip\r\nContent-Length: x\r\n"), EAMBIGUOUS, [0], 0),
    ("chunk size 0", chunked(b"0\r\n\r\n"), OK, [0], len(chunked(b"0\r\n\r\n"))),
    ("chunk size 000", chunked(b"000\r\n\r\n"), OK, [0], len(chunked(b"000\r\n\r\n"))),
    ("chunk size a", chunked(b"a\r\n0123456789\r\n0\r\n\r\n") + G, OK, [0, len(chunked(b"a\r\n0123456789\r\n0\r\n\r\n"))],
     len(chunked(b"a\r\n0123456789\r\n0\r\n\r\n")) + 19),
    ("chunk size A", chunked(b"A\r\n0123456789\r\n0\r\n\r\n"), OK, [0], len(chunked(b"A\r\n0123456789\r\n0\r\n\r\n"))),
    ("15 hex digits", chunked(b"00000000000000a\r\n0123456789\r\n000000000000000\r\n\r\n"), OK, [0],
     len(chunked(b"00000000000000a\r\n0123456789\r\n000000000000000\r\n\r\n"))),
    ("15 hex digits, all f", chunked(b"fffffffffffffff\r\nabc"), EPARTIAL_BODY, [0], 0),
    ("16 hex digits", chunked(b"000000000000000a\r\n0123456789\r\n0\r\n\r\n"), EBADCHUNK, [0], 0),
    ("16 zeros", chunked(b"0000000000000000\r\n\r\n"), EBADCHUNK, [0], 0),
    ("no chunk size", chunked(b"\r\n\r\n"), EBADCHUNK, [0], 0),
    ("chunk size g", chunked(b"g\r\n"), EBADCHUNK, [0], 0),
    ("extension", chunked(b"5;name=\"v\";\xff \t\r\nhello\r\n0;x\r\n\r\n") + G, OK,
     [0, len(chunked(b"5;name=\"v\";\xff \t\r\nhello\r\n0;x\r\n\r\n"))],
     len(chunked(b"5;name=\"v\";\xff \t\r\nhello\r\n0;x\r\n\r\n")) + 19),
    ("nul in extension", chunked(b"5;a\0b\r\nhello\r\n0\r\n\r\n"), EBADCHUNK, [0], 0),
    ("lf in extension", chunked(b"5;a\nb\r\nhello\r\n0\r\n\r\n"), EBADCHUNK, [0], 0),
    ("space before ;", chunked(b"5 ;x\r\nhello\r\n0\r\n\r\n"), EBADCHUNK, [0], 0),
    ("bare lf after size", G + chunked(b"5\nhello\r\n0\r\n\r\n"), EBADCHUNK, [0, 19], 19),
    ("cr without lf after size", chunked(b"5\rXhello\r\n0\r\n\r\n"), EBADCHUNK, [0], 0),
    ("data not followed by crlf", chunked(b"5\r\nhelloXX0\r\n\r\n"), EBADCHUNK, [0], 0),
    ("data followed by cr only", chunked(b"5\r\nhello\rX0\r\n\r\n"), EBADCHUNK, [0], 0),
    ("data holds crlf", chunked(b"4\r\n\r\n\r\n\r\n0\r\n\r\n") + G, OK, [0, len(chunked(b"4\r\n\r\n\r\n\r\n0\r\n\r\n"))],
     len(chunked(b"4\r\n\r\n\r\n\r\n0\r\n\r\n")) + 19),
    ("trailers", chunked(b"0\r\nX-T: 1\r\nY:\r\nz:\x01\xff\r\n\r\n") + G, OK,
     [0, len(chunked(b"0\r\nX-T: 1\r\nY:\r\nz:\x01\xff\r\n\r\n"))], len(chunked(b"0\r\nX-T: 1\r\nY:\r\nz:\x01\xff\r\n\r\n")) + 19),
    ("bad trailer name", chunked(b"0\r\nX T: 1\r\n\r\n"), EBADCHUNK, [0], 0),
    ("trailer without colon", chunked(b"0\r\nXT\r\n\r\n"), EBADCHUNK, [0], 0),
    ("trailer with bare lf", chunked(b"0\r\nX: 1\n\r\n"), EBADCHUNK, [0], 0),
    ("trailer with nul", chunked(b"0\r\nX: \0\r\n\r\n"), EBADCHUNK, [0], 0),
    ("last line cr without lf", chunked(b"0\r\n\rX"), EBADCHUNK, [0], 0),
    ("chunked then a request", _CH + G, OK, [0, len(_CH)], len(_CH) + 19),
    ("CONNECT", _CONNECT + b"\x16\x03\x01 opaque", TUNNEL, [0], len(_CONNECT)),
    ("CONNECT after a request", G + _CONNECT + G, TUNNEL, [0, 19], 19 + len(_CONNECT)),
    ("connect in lower case is no tunnel", _CONNECT.replace(b"CONNECT", b"connect") + b"\x16\x03", EBADHEAD,
     [0, len(_CONNECT)], len(_CONNECT)),
    ("CONNECTX is no tunnel", _CONNECT.replace(b"CONNECT", b"CONNECTX"), OK, [0], len(_CONNECT) + 1),
    ("refused head after two requests", G + _CL5 + b"BAD\r\n\r\n" + G, EBADHEAD, [0, 19, 19 + len(_CL5)], 19 + len(_CL5)),
    ("partial head after a request", G + b"GET /b HT", EPARTIAL_HEAD, [0, 19], 19),
    ("partial head alone", b"G", EPARTIAL_HEAD, [0], 0),
    ("refused head alone", b"\r\n" + G, EBADHEAD, [0], 0),
    ("http/1.0 with a length", b"POST /p HTTP/1.0\r\nContent-Length: 2\r\n\r\nhi" + G, OK,
     [0, len(b"POST /p HTTP/1.0\r\nContent-Length: 2\r\n\r\nhi")], len(b"POST /p HTTP/1.0\r\nContent-Length: 2\r\n\r\nhi") + 19),
] + [
    # a cut at every byte of a small chunked request, behind a complete one
    ("cut at %d" % k, G + _CH[:k], EPARTIAL_HEAD if k < _CH_HEAD else EPARTIAL_BODY, [0, 19], 19)
    for k in range(1, len(_CH))
]


def http_table_conns():
    return [c for _, c, _, _, _ in HTTP_TABLE]


# ---- Kafka known answers ---------------------------------------------------
def frame(size, fill=0x61, have=None):
    """A size field and `have` (default: size) bytes behind it."""
    return struct.pack(">i", size) + bytes([fill]) * (max(size, 0) if have is None else have)


_F8, _F9, _F10, _F11 = frame(8), frame(9, 0x62), frame(10, 0x63), frame(11, 0x64)

# (name, connection, status, [(start, frame bytes)], consumed)
KAFKA_TABLE = [
    ("empty connection", b"", OK, [], 0),
    ("size -1", frame(-1), EBADSIZE, [], 0),
    ("size 0", frame(0), EBADSIZE, [], 0),
    ("size 7", frame(7), EBADSIZE, [], 0),
    ("size 7 after a frame", _F8 + frame(7), EBADSIZE, [(0, 12)], 12),
    ("size 8", _F8, OK, [(0, 12)], 12),
    ("size min int", struct.pack(">I", 0x80000000) + b"x" * 16, EBADSIZE, [], 0),
    ("size max int", struct.pack(">I", 0x7FFFFFFF) + b"x" * 16, EBADSIZE, [], 0),
    ("largest frame", frame(KAFKA_MAX_FRAME - 4) + _F8, OK, [(0, KAFKA_MAX_FRAME), (KAFKA_MAX_FRAME, 12)],
     KAFKA_MAX_FRAME + 12),
    ("one more than the largest", frame(KAFKA_MAX_FRAME - 3, have=64), EBADSIZE, [], 0),
    ("largest frame cut", _F8 + frame(KAFKA_MAX_FRAME - 4, have=64), EPARTIAL_FRAME, [(0, 12)], 12),
    ("cut in the size field: 1", _F9 + b"\0", EPARTIAL_FRAME, [(0, 13)], 13),
    ("cut in the size field: 2", _F9 + b"\0\0", EPARTIAL_FRAME, [(0, 13)], 13),
    ("cut in the size field: 3", _F9 + b"\0\0\0", EPARTIAL_FRAME, [(0, 13)], 13),
    ("only a size field", struct.pack(">i", 8), EPARTIAL_FRAME, [], 0),
    ("cut in the frame", _F10 + frame(12, have=11), EPARTIAL_FRAME, [(0, 14)], 14),
    ("one byte alone", b"\0", EPARTIAL_FRAME, [], 0),
    # 13, 14, 15 and 12 byte frames: starts at 0, 13, 27, 42, 54, ...: every alignment modulo 4
    ("every alignment", (_F9 + _F10 + _F11 + _F8) * 3,
     OK, [(s, n) for s, n in zip(np.cumsum([0] + [13, 14, 15, 12] * 3)[:-1].tolist(), [13, 14, 15, 12] * 3)], 162),
    ("every alignment, other order", _F11 + _F11 + _F9 + _F9 + _F10 + _F8, OK,
     [(0, 15), (15, 15), (30, 13), (43, 13), (56, 14), (70, 12)], 82),
]


def kafka_table_conns():
    return [c for _, c, _, _, _ in KAFKA_TABLE]


# ---- seeded fuzz -------------------------------------------------------------
HTTP_MUTATION_RATE = 0.45   # share of the connections that get one mutation
KAFKA_MUTATION_RATE = 0.5
FUZZ_SEED = 11


def _request(rng):
    """A valid head (http_wire_cases) with no body, a counted body or a chunked one."""
    head = W._valid_head(rng)
    head = head[:W.parse_head(head)[0]]  # without the random bytes behind the empty line
    kind = rng.random()
    if kind < 0.4:
        return head
    data = bytes(rng.integers(0, 256, size=int(rng.integers(0, 60)), dtype=np.uint8))
    if kind < 0.7:
        name = [b"Content-Length", b"content-length", b"CONTENT-LENGTH"][int(rng.integers(0, 3))]
        return head[:-2] + name + b": %d\r\n\r\n" % len(data) + data
    body, at = b"", 0
    while at < len(data):
        k = int(rng.integers(1, 24))
        piece = data[at:at + k]
        ext = b";q=1" if rng.random() < 0.2 else b""
        body += (b"%x" if rng.random() < 0.5 else b"%X") % len(piece) + ext + b"\r\n" + piece + b"\r\n"
        at += k
    body += b"0\r\n" + (b"X-Sum: 1\r\n" if rng.random() < 0.3 else b"") + b"\r\n"
    return head[:-2] + b"Transfer-Encoding: chunked\r\n\r\n" + body


def _mutate(rng, conn, splices):
    c = bytearray(conn)
    if not c:
        return bytes(rng.integers(0, 256, size=int(rng.integers(1, 9)), dtype=np.uint8))
    r = rng.random()
    if r < 0.4:
        del c[int(rng.integers(0, len(c))):]
    elif r < 0.7:
        c[int(rng.integers(0, len(c)))] = int(rng.integers(0, 256))
    else:
        at = int(rng.integers(0, len(c) + 1))
        c[at:at] = splices[int(rng.integers(0, len(splices)))]
    return bytes(c)


_HTTP_SPLICE = [b"\r", b"\n", b"\r\n", b"\r\n\r\n", b" ", b";", b"0", b"\0", b"Content-Length: 3\r\n",
                b"Transfer-Encoding: chunked\r\n", b"f"]
_KAFKA_SPLICE = [b"\0", b"\0\0\0", b"\xff\xff\xff\xff", b"\0\0\0\x07", b"\x7f"]


def fuzz_http_conns(n=600, seed=FUZZ_SEED):
    """Connections of 0-12 requests, HTTP_MUTATION_RATE of them mutated (cut,
    one byte replaced, or a splice); between a quarter and three quarters of
    them must end with status OK."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        conn = b"".join(_request(rng) for _ in range(int(rng.integers(0, 13))))
        if rng.random() < 0.03:
            conn += _CONNECT + b"\x16\x03\x01"
        if rng.random() < HTTP_MUTATION_RATE:
            conn = _mutate(rng, conn, _HTTP_SPLICE)
        out.append(conn)
    share = sum(frame_http_conn(c)[1] == OK for c in out) / n
    assert 0.25 <= share <= 0.75, share
    return out


def fuzz_kafka_conns(n=600, seed=FUZZ_SEED):
    """Connections of 0-12 requests (kafka_wire.random_requests), KAFKA_MUTATION_RATE of them mutated."""
    rng = np.random.default_rng(seed)
    topics = ["t%d" % i for i in range(6)]
    clients = ["c%d" % i for i in range(4)]
    out = []
    for _ in range(n):
        conn = b"".join(K.random_requests(rng, int(rng.integers(0, 13)), topics, clients))
        if rng.random() < KAFKA_MUTATION_RATE:
            conn = _mutate(rng, conn, _KAFKA_SPLICE)
        out.append(conn)
    share = sum(frame_kafka_conn(c)[1] == OK for c in out) / n
    assert 0.25 <= share <= 0.75, share
    return out


def ok_shares(seed):
    """(HTTP, Kafka) share of the fuzz connections that end with status OK."""
    h = fuzz_http_conns(seed=seed)
    k = fuzz_kafka_conns(seed=seed)
    return (sum(frame_http_conn(c)[1] == OK for c in h) / len(h), sum(frame_kafka_conn(c)[1] == OK for c in k) / len(k))


def conn_offs(conns):
    offs = np.zeros(len(conns) + 1, dtype=np.uint64)
    if conns:
        offs[1:] = np.cumsum([len(c) for c in conns], dtype=np.uint64)
    return offs


def dump(path, http_sets, kafka_sets):
    """Connection sets with the expected outputs for the stand-alone sanitizer
    program.  Per set: u32 protocol (1 HTTP, 2 Kafka), u32 n_conns, u64
    conn_offs[n_conns + 1], the wire, i32 status[n_conns], u64 consumed[n_conns],
    u64 n, then HTTP: u64 head_offs[n + 1], u32 head_conn[n]; Kafka: u64
    arena bytes, u64 rec_offsets[n], u32 rec_conn[n], the arena."""
    with open(path, "wb") as f:
        for proto, sets in ((1, http_sets), (2, kafka_sets)):
            for conns in sets:
                f.write(struct.pack("<II", proto, len(conns)))
                f.write(conn_offs(conns).tobytes())
                f.write(b"".join(conns))
                if proto == 1:
                    offs, hconn, _, status, consumed = frame_http(conns)
                    f.write(status.astype("<i4").tobytes() + consumed.astype("<u8").tobytes())
                    f.write(struct.pack("<Q", len(hconn)) + offs.astype("<u8").tobytes() + hconn.astype("<u4").tobytes())
                else:
                    arena, offs, rconn, _, status, consumed, _ = frame_kafka(conns)
                    f.write(status.astype("<i4").tobytes() + consumed.astype("<u8").tobytes())
                    f.write(struct.pack("<QQ", len(rconn), len(arena)) + offs.astype("<u8").tobytes() +
                            rconn.astype("<u4").tobytes() + arena)
