"""HTTP/1.x request heads for the wire-decode tests: a decoder written from
the grammar in DESIGN.md ("HTTP/1.x wire decode"), independent of the C code,
a known-answer table and a seeded fuzz set.  Shared by the CPU and GPU tests
and by the stand-alone sanitizer program (tests/cpp/http_wire_asan.cc)."""
import struct

import numpy as np

EINCOMPLETE, EBADLINE, EBADHEADER, EDUPHOST, ETOOMANY, ETOOLONG = -1, -2, -3, -4, -5, -6

TCHAR = frozenset(b"!#$%&'*+-.^_`|~0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")
OWS = b" \t"
F_METHOD, F_PATH, F_AUTHORITY, F_INGRESS = 1, 2, 4, 8


class Refused(Exception):
    def __init__(self, code):
        self.code = code


def parse_head(head: bytes):
    """-> (consumed, method, target, host or None, [(lower-cased name, value)]);
    raises Refused(code).  One scan from the left: the first offending byte
    decides, running out of bytes is EINCOMPLETE."""
    n = len(head)

    def need(p):
        if p >= n:
            raise Refused(EINCOMPLETE)
        return head[p]

    p = 0
    while p < n and head[p] in TCHAR:
        p += 1
    if need(p) != 0x20 or p == 0:
        raise Refused(EBADLINE)
    if p > 65535:
        raise Refused(ETOOLONG)
    method = head[:p]
    p += 1
    t0 = p
    while p < n and head[p] > 0x20 and head[p] != 0x7F:
        p += 1
    if need(p) != 0x20 or p == t0:
        raise Refused(EBADLINE)
    if p - t0 > 65535:
        raise Refused(ETOOLONG)
    target = head[t0:p]
    p += 1
    for k, want in enumerate(b"HTTP/1.1\r\n"):
        c = need(p)
        if c != want and not (k == 7 and c == ord("0")):
            raise Refused(EBADLINE)
        p += 1
    host = None
    headers = []
    while True:
        c = need(p)
        if c == 0x0D:
            if need(p + 1) != 0x0A:
                raise Refused(EBADHEADER)
            p += 2
            break
        n0 = p
        while p < n and head[p] in TCHAR:
            p += 1
        if need(p) != ord(":") or p == n0:
            raise Refused(EBADHEADER)
        name = head[n0:p]
        if len(name) > 65535:
            raise Refused(ETOOLONG)
        p += 1
        while p < n and head[p] in OWS:
            p += 1
        v0 = p
        while True:
            c = need(p)
            if c == 0x0D:
                if need(p + 1) != 0x0A:
                    raise Refused(EBADHEADER)
                break
            if c in (0x0A, 0):
                raise Refused(EBADHEADER)
            p += 1
        value = head[v0:p].rstrip(OWS)
        p += 2
        if len(value) > 65535:
            raise Refused(ETOOLONG)
        if name.lower() == b"host":
            if host is not None:
                raise Refused(EDUPHOST)
            host = value
        else:
            if len(headers) == 255:
                raise Refused(ETOOMANY)
            headers.append((name.lower(), value))
    if p > 0x7FFFFFFF:
        raise Refused(ETOOLONG)
    return p, method, target, host, headers


def record(method, target, host, headers, meta=None):
    """The arena record (include/l7match.h), padded to 4 bytes."""
    remote_id, dport, policy, ingress = meta or (0, 0, 0, 1)
    flags = F_METHOD | F_PATH | (F_AUTHORITY if host is not None else 0) | (F_INGRESS if ingress else 0)
    host = host or b""
    body = b"".join(struct.pack("<I", len(k) | len(v) << 16) for k, v in headers)
    body += method + target + host + b"".join(k + v for k, v in headers)
    rec = struct.pack("<5I", 20 + len(body), remote_id, dport | flags << 16 | len(headers) << 24,
                      len(method) | len(target) << 16, len(host) | policy << 16) + body
    return rec + b"\0" * (-len(rec) % 4)


def failed_record(meta=None):
    remote_id, dport, policy, ingress = meta or (0, 0, 0, 1)
    return struct.pack("<5I", 0, remote_id, dport | (F_INGRESS if ingress else 0) << 16, 0, policy << 16)


def decode(heads, metas=None):
    """-> (arena bytes, offsets uint64[n], status int32[n]) as the library must produce them."""
    recs, status = [], []
    for i, h in enumerate(heads):
        meta = metas[i] if metas is not None else None
        try:
            used, method, target, host, headers = parse_head(h)
            recs.append(record(method, target, host, headers, meta))
            status.append(used)
        except Refused as e:
            recs.append(failed_record(meta))
            status.append(e.code)
    offs = np.zeros(len(heads), dtype=np.uint64)
    if heads:
        offs[1:] = np.cumsum([len(r) for r in recs[:-1]], dtype=np.uint64)
    return b"".join(recs), offs, np.array(status, dtype=np.int32).reshape(len(heads))


def parsed_requests(heads, metas=None):
    """The heads the grammar accepts as (index, method, target, host, headers)."""
    out = []
    for i, h in enumerate(heads):
        try:
            _, method, target, host, headers = parse_head(h)
            out.append((i, method, target, host, headers))
        except Refused:
            pass
    return out


def metas_for(n, seed=5):
    """(remote_id, dport, policy, ingress) per head."""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 16)),
             int(rng.integers(0, 2))) for _ in range(n)]


def meta_array(metas):
    from cilium_amd import l7match as L
    a = np.zeros(len(metas), dtype=L.WIRE_META_DTYPE)
    for i, (rid, dport, policy, ingress) in enumerate(metas):
        a[i] = (rid, dport, policy, ingress, (0, 0, 0))
    return a


def _many(k):
    return b"".join(b"x-%d: %d\r\n" % (i, i) for i in range(k))


RL = b"GET /a HTTP/1.1\r\n"

# (name, head, expected status: None = accepted with every byte consumed,
#  an int >= 0 = accepted with that many bytes consumed, < 0 = the code)
TABLE = [
    ("plain", RL + b"Host: h.example\r\nAccept: */*\r\n\r\n", None),
    ("empty value", RL + b"x-empty:\r\n\r\n", None),
    ("value only ows", RL + b"x-ows: \t  \t\r\n\r\n", None),
    ("htab as ows", RL + b"x-tab:\tv\t\r\n\r\n", None),
    ("inner ows kept", RL + b"x-in:  a \t b  \r\n\r\n", None),
    ("obs-text in value", RL + b"x-hi: caf\xc3\xa9 \xff\x80\r\n\r\n", None),
    ("ctl in value", RL + b"x-ctl: a\x01\x7fb\r\n\r\n", None),
    ("host mixed case", RL + b"hOsT: Example.COM\r\n\r\n", None),
    ("host first", RL + b"Host: a\r\nx-a: 1\r\nx-b: 2\r\n\r\n", None),
    ("host middle", RL + b"x-a: 1\r\nHost: a\r\nx-b: 2\r\n\r\n", None),
    ("host last", RL + b"x-a: 1\r\nx-b: 2\r\nHost: a\r\n\r\n", None),
    ("host empty", RL + b"Host:\r\n\r\n", None),
    ("no host", RL + b"x-a: 1\r\n\r\n", None),
    ("no headers", RL + b"\r\n", None),
    ("http/1.0", b"GET /a HTTP/1.0\r\nHost: a\r\n\r\n", None),
    ("absolute-form", b"GET http://u@h.example:8080/p?q=1#f HTTP/1.1\r\nHost: other\r\n\r\n", None),
    ("asterisk-form", b"OPTIONS * HTTP/1.1\r\nHost: a\r\n\r\n", None),
    ("authority-form", b"CONNECT h.example:443 HTTP/1.1\r\nHost: h.example:443\r\n\r\n", None),
    ("tchar method", b"M-!#$%&'*+.^_`|~9 /a HTTP/1.1\r\n\r\n", None),
    ("tchar name", RL + b"X_!#$%&'*+-.^`|~9Z: v\r\n\r\n", None),
    ("high bytes in target", b"GET /\x80\xff{}|\"<> HTTP/1.1\r\n\r\n", None),
    ("duplicate regular headers", RL + b"x-a: 1\r\nX-A: 2\r\nx-a: 3\r\n\r\n", None),
    ("255 headers", RL + _many(255) + b"\r\n", None),
    ("255 headers and host", RL + _many(100) + b"Host: h\r\n" + _many(155) + b"\r\n", None),
    ("256 headers", RL + _many(256) + b"\r\n", ETOOMANY),
    ("65535-byte value", RL + b"x-v: " + b"v" * 65535 + b"\r\n\r\n", None),
    ("65536-byte value", RL + b"x-v: " + b"v" * 65536 + b"\r\n\r\n", ETOOLONG),
    ("65536 bytes with ows trimmed", RL + b"x-v: " + b"v" * 65535 + b" \r\n\r\n", None),
    ("65535-byte target", b"GET /" + b"p" * 65534 + b" HTTP/1.1\r\n\r\n", None),
    ("65536-byte target", b"GET /" + b"p" * 65535 + b" HTTP/1.1\r\n\r\n", ETOOLONG),
    ("65536-byte name", RL + b"n" * 65536 + b": v\r\n\r\n", ETOOLONG),
    ("65536-byte method", b"M" * 65536 + b" / HTTP/1.1\r\n\r\n", ETOOLONG),
    ("body after head", RL + b"Host: a\r\n\r\n{\"k\": 1}\r\n\r\n", len(RL) + 11),
    ("pipelined request", RL + b"\r\nGET /b HTTP/1.1\r\n\r\n", len(RL) + 2),
    ("zero bytes", b"", EINCOMPLETE),
    ("only method", b"GET", EINCOMPLETE),
    ("no version", b"GET /a ", EINCOMPLETE),
    ("cut in version", b"GET /a HTTP/1.", EINCOMPLETE),
    ("cut after request line cr", b"GET /a HTTP/1.1\r", EINCOMPLETE),
    ("no empty line", RL + b"Host: a\r\n", EINCOMPLETE),
    ("cut in name", RL + b"Hos", EINCOMPLETE),
    ("cut in value", RL + b"Host: a", EINCOMPLETE),
    ("cut after value cr", RL + b"Host: a\r", EINCOMPLETE),
    ("cut after final cr", RL + b"Host: a\r\n\r", EINCOMPLETE),
    ("cr without lf in value", RL + b"x-a: 1\r2\r\n\r\n", EBADHEADER),
    ("cr without lf at end", RL + b"x-a: 1\r\n\rX", EBADHEADER),
    ("lf alone ends header", RL + b"x-a: 1\n\r\n", EBADHEADER),
    ("lf alone as empty line", RL + b"x-a: 1\r\n\n", EBADHEADER),
    ("lf alone ends request line", b"GET /a HTTP/1.1\nHost: a\r\n\r\n", EBADLINE),
    ("obs-fold sp", RL + b"x-a: 1\r\n 2\r\n\r\n", EBADHEADER),
    ("obs-fold htab", RL + b"x-a: 1\r\n\t2\r\n\r\n", EBADHEADER),
    ("space before colon", RL + b"x-a : 1\r\n\r\n", EBADHEADER),
    ("empty name", RL + b": 1\r\n\r\n", EBADHEADER),
    ("no colon", RL + b"x-a\r\n\r\n", EBADHEADER),
    ("nul in value", RL + b"x-a: 1\x002\r\n\r\n", EBADHEADER),
    ("non-tchar in name", RL + b"x(a): 1\r\n\r\n", EBADHEADER),
    ("high byte in name", RL + b"x\xc3\xa9: 1\r\n\r\n", EBADHEADER),
    ("duplicate host", RL + b"Host: a\r\nx-a: 1\r\nhost: a\r\n\r\n", EDUPHOST),
    ("empty method", b" /a HTTP/1.1\r\n\r\n", EBADLINE),
    ("non-tchar in method", b"GE(T /a HTTP/1.1\r\n\r\n", EBADLINE),
    ("empty target", b"GET  HTTP/1.1\r\n\r\n", EBADLINE),
    ("htab in request line", b"GET\t/a HTTP/1.1\r\n\r\n", EBADLINE),
    ("ctl in target", b"GET /a\x01b HTTP/1.1\r\n\r\n", EBADLINE),
    ("del in target", b"GET /a\x7fb HTTP/1.1\r\n\r\n", EBADLINE),
    ("http/2.0", b"GET /a HTTP/2.0\r\n\r\n", EBADLINE),
    ("http/1.2", b"GET /a HTTP/1.2\r\n\r\n", EBADLINE),
    ("lower-case version", b"GET /a http/1.1\r\n\r\n", EBADLINE),
    ("three spaces", b"GET /a b HTTP/1.1\r\n\r\n", EBADLINE),
    ("sp after version", b"GET /a HTTP/1.1 \r\n\r\n", EBADLINE),
    ("leading crlf", b"\r\n" + RL + b"\r\n", EBADLINE),
]


def table_heads():
    return [h for _, h, _ in TABLE]


_METHODS = [b"GET", b"POST", b"PUT", b"DELETE", b"HEAD", b"OPTIONS", b"PATCH"]
_NAMES = [b"Accept", b"User-Agent", b"X-Token", b"x-k", b"Content-Type", b"Cookie", b"X-Forwarded-Proto", b"a"]
_SPLICE = [b"\r", b"\n", b"\r\n", b"\r\n\r\n", b" ", b"\t", b":", b"\0", b"\r\n ", b"Host: x\r\n"]


def _valid_head(rng):
    path = b"/" + b"/".join(bytes(rng.choice(list(b"abcxyz019-_.~%"), size=int(rng.integers(0, 9))).astype(np.uint8))
                           for _ in range(int(rng.integers(0, 4))))
    lines = []
    for _ in range(int(rng.integers(0, 7))):
        val = bytes(rng.choice(list(b"abc XYZ019=;,/\t\xe9"), size=int(rng.integers(0, 24))).astype(np.uint8))
        lead = [b"", b" ", b"  ", b"\t"][int(rng.integers(0, 4))]
        trail = [b"", b"", b" ", b"\t "][int(rng.integers(0, 4))]
        lines.append(_NAMES[int(rng.integers(0, len(_NAMES)))] + b":" + lead + val + trail + b"\r\n")
    if rng.random() < 0.8:
        host = [b"Host", b"host", b"HOST"][int(rng.integers(0, 3))] + b": svc-%d.example.com\r\n" % int(
            rng.integers(0, 50))
        lines.insert(int(rng.integers(0, len(lines) + 1)), host)
    ver = b"HTTP/1.1" if rng.random() < 0.9 else b"HTTP/1.0"
    head = _METHODS[int(rng.integers(0, len(_METHODS)))] + b" " + path + b" " + ver + b"\r\n" + b"".join(lines) + b"\r\n"
    if rng.random() < 0.2:
        head += bytes(rng.integers(0, 256, size=int(rng.integers(1, 40)), dtype=np.uint8))  # a body
    return head


def fuzz_heads(n=2000, seed=7):
    """Valid heads, about half of them mutated: byte flips, truncation, spliced CR / LF and friends."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        h = bytearray(_valid_head(rng))
        r = rng.random()
        if r < 0.2:
            for _ in range(int(rng.integers(1, 4))):
                h[int(rng.integers(0, len(h)))] = int(rng.integers(0, 256))
        elif r < 0.35:
            del h[int(rng.integers(0, len(h))):]
        elif r < 0.5:
            at = int(rng.integers(0, len(h) + 1))
            h[at:at] = _SPLICE[int(rng.integers(0, len(_SPLICE)))]
        out.append(bytes(h))
    return out


def dump(path, heads):
    """Heads and the expected decode for the stand-alone sanitizer program: u32 n,
    u64 head_offs[n + 1], the wire bytes, i32 status[n], u64 arena bytes, the arena."""
    arena, _, status = decode(heads)
    offs = np.zeros(len(heads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(h) for h in heads], dtype=np.uint64)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(heads)))
        f.write(offs.tobytes())
        f.write(b"".join(heads))
        f.write(status.astype("<i4").tobytes())
        f.write(struct.pack("<Q", len(arena)))
        f.write(arena)
