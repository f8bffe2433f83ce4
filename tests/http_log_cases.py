"""HTTP records for the access-log and proxy-statistics tests: a table of
hand-built records (well-formed ones packed by l7m_pack_http, the others with
struct), seeded random ones, and an encoder of the expected HttpLogEntry that
works from a case's fields, not from its record bytes.  Used by
tests/test_http_log_cpu.py, tests/test_http_log_gpu.py and the stand-alone
sanitizer program tests/cpp/http_log_asan.cc (dump)."""
import struct

import numpy as np

from cilium_amd import l7match as L

VERDICTS = [0, 7, 0x7FFFFFFE, 0x7FFFFFFF, -1, -2, -3]
XFP = b"x-forwarded-proto"

# keyword options of L.http_access_log / L.http_access_log_device
ALL_STRINGS = dict(policy_name="ep-7", timestamp_ns=1_700_000_000_000, local_identity=99,
                   source_address="10.1.2.3:1", destination_address="10.9.8.7:80")
OPTS = [dict(), ALL_STRINGS, dict(timestamp_ns=0), dict(timestamp_ns=2 ** 63), dict(http_protocol=0),
        dict(http_protocol=2)]


def fields(method=b"GET", path=b"/", authority=None, headers=(), remote_id=5, dport=80, ingress=True, flags=None,
           bad=None, raw=False):
    """A case.  method / path / authority None: absent (flag clear, no bytes).  flags: override of the
    presence flags the fields imply.  bad: how the record or its offset is malformed.  raw: pack with
    struct although the record is well-formed (l7m_pack_http would lower-case a name)."""
    implied = ((L.F_METHOD if method is not None else 0) | (L.F_PATH if path is not None else 0) |
               (L.F_AUTHORITY if authority is not None else 0) | (L.F_INGRESS if ingress else 0))
    return dict(method=method, path=path, authority=authority, headers=list(headers), remote_id=remote_id,
                dport=dport, flags=implied if flags is None else flags, bad=bad, raw=raw or flags is not None)


def raw_record(f, rec_len_delta=0, dir_delta=0, n_hdr=None):
    """The record of a case written with struct; rec_len off by rec_len_delta, the first directory
    entry's value length off by dir_delta, the header count replaced by n_hdr."""
    m, p, a = f["method"] or b"", f["path"] or b"", f["authority"] or b""
    body = m + p + a + b"".join(n + v for n, v in f["headers"])
    rec_len = L.HTTP_REC_FIXED + 4 * len(f["headers"]) + len(body)
    out = struct.pack("<IIHBBHHHH", rec_len + rec_len_delta, f["remote_id"], f["dport"], f["flags"],
                      len(f["headers"]) if n_hdr is None else n_hdr, len(m), len(p), len(a), 0)
    for j, (n, v) in enumerate(f["headers"]):
        out += struct.pack("<HH", len(n), len(v) + (dir_delta if j == 0 else 0))
    return out + body


def record(f):
    if f["bad"] == "rec_len+1":
        return raw_record(f, rec_len_delta=1) + b"\0"  # the byte it claims exists: only the sum is wrong
    if f["bad"] == "rec_len-1":
        return raw_record(f, rec_len_delta=-1)
    if f["bad"] == "dir_sum":
        return raw_record(f, dir_delta=40)
    if f["bad"] == "dir_overrun":
        return raw_record(f, n_hdr=255)  # a directory of 1020 bytes in a record of some thirty
    if f["bad"] == "refused":
        return raw_record(f, rec_len_delta=-L.HTTP_REC_FIXED)  # rec_len 0 (l7m_http_wire.h wire_emit_failed)
    if f["raw"]:
        return raw_record(f)
    q = L.HTTPRequest(f["method"], f["path"], f["authority"], f["headers"], f["remote_id"], f["dport"],
                      bool(f["flags"] & L.F_INGRESS))
    arena, _ = L.pack_http([q])
    rec = arena.tobytes()
    return rec[:struct.unpack_from("<I", rec)[0]]


BIG = bytes(97 + i % 26 for i in range(65535))

TABLE = [
    ("no_headers", fields(authority=b"svc.example")),
    ("255_headers", fields(headers=[(b"x-h%d" % i, b"v" * (i % 7)) for i in range(255)])),
    ("one_xfp", fields(headers=[(b"accept", b"*/*"), (XFP, b"https"), (b"x-k", b"1")])),
    ("two_xfp", fields(headers=[(XFP, b"http"), (b"accept", b"*/*"), (XFP, b"https")])),
    ("xfp_empty_value", fields(headers=[(XFP, b""), (b"a", b"b")])),
    ("xfp_then_empty_xfp", fields(headers=[(XFP, b"https"), (XFP, b"")])),
    ("xfp_upper_case", fields(headers=[(b"X-Forwarded-Proto", b"https")], raw=True)),
    ("xfp_17_bytes_other", fields(headers=[(b"x-forwarded-protp", b"https"), (b"y-forwarded-proto", b"h")])),
    ("empty_name_and_value", fields(headers=[(b"", b""), (b"a", b"b"), (b"", b"")])),
    ("empty_value_only", fields(headers=[(b"x-empty", b"")])),
    ("empty_name_only", fields(headers=[(b"", b"v")])),
    ("no_method_flag", fields(method=None, authority=b"h")),
    ("no_path_flag", fields(path=None, authority=b"h")),
    ("no_authority_flag", fields(authority=None)),
    ("method_bytes_flag_clear", fields(authority=b"h", flags=L.F_PATH | L.F_AUTHORITY | L.F_INGRESS)),
    ("path_bytes_flag_clear", fields(authority=b"h", flags=L.F_METHOD | L.F_AUTHORITY | L.F_INGRESS)),
    ("authority_bytes_flag_clear", fields(authority=b"h", flags=L.F_METHOD | L.F_PATH | L.F_INGRESS)),
    ("empty_fields_flags_set", fields(method=b"", path=b"", authority=b"")),
    ("egress", fields(ingress=False, remote_id=77, authority=b"out.example", headers=[(b"a", b"b")])),
    ("value_65535", fields(headers=[(b"x-big", BIG), (b"after", b"1")])),
    ("path_65535", fields(path=BIG, authority=b"h")),
    ("remote_id_0", fields(remote_id=0)),
    ("remote_id_max", fields(remote_id=0xFFFFFFFF)),
    ("dport_65535", fields(dport=65535)),
    # the 20 bytes the wire decoder writes for a head it refuses: every length zero, rec_len too
    ("refused_head", fields(method=None, path=None, remote_id=3, dport=8080, bad="refused")),
    ("twenty_bytes_valid", fields(method=None, path=None, flags=L.F_INGRESS, remote_id=0, dport=0)),
    ("rec_len_one_too_large", fields(authority=b"h", headers=[(b"a", b"b")], bad="rec_len+1")),
    ("rec_len_one_too_small", fields(authority=b"h", headers=[(b"a", b"b")], bad="rec_len-1")),
    ("directory_overruns_rec_len", fields(headers=[(b"a", b"b"), (b"c", b"d")], bad="dir_overrun")),
    ("directory_sum_differs", fields(headers=[(b"a", b"b"), (b"c", b"d")], bad="dir_sum")),
    ("offset_not_aligned", fields(authority=b"h", bad="offset+2")),
    ("offset_at_arena_bytes", fields(bad="offset=end")),
    ("offset_past_arena_bytes", fields(bad="offset>end")),
    ("offset_far_past_arena_bytes", fields(bad="offset=2^63")),
    ("fixed_part_overruns_arena", fields(bad="offset=end-16")),
    # the arena's last record: a reader that trusted n_hdr would leave the arena
    ("directory_overruns_arena", fields(method=None, path=None, bad="dir_overrun")),
]


def build(cases):
    """cases: [(fields, verdict)] -> (arena, offs, verdicts).  Records back to back, 4-aligned,
    ascending; the offsets of the offset cases point where their name says."""
    recs = [record(f) for f, _ in cases]
    arena, offs = L.pack_records(recs)
    end = arena.shape[0]
    for i, (f, _) in enumerate(cases):
        bad = f["bad"]
        if bad == "offset+2":
            offs[i] += 2
        elif bad == "offset=end":
            offs[i] = end
        elif bad == "offset>end":
            offs[i] = end + 4
        elif bad == "offset=2^63":
            offs[i] = 2 ** 63
        elif bad == "offset=end-16":
            offs[i] = end - 16
    return arena, offs, np.array([v for _, v in cases]).astype(np.uint32).view(np.int32)


def table_cases():
    return [(f, v) for _, f in TABLE for v in VERDICTS]


_NAMES = [b"accept", b"user-agent", b"x-token", b"x-k", b"content-type", b"cookie", XFP, b"a", b""]


def fuzz_cases(n=2000, seed=13):
    """Random records: 0-12 headers, lengths 0-300, about 5 % malformed; random verdicts."""
    rng = np.random.default_rng(seed)
    bads = ["rec_len+1", "rec_len-1", "dir_overrun", "dir_sum", "offset+2", "offset=end", "offset>end", "refused"]
    out = []
    for _ in range(n):
        def blob(hi=300):
            k = int(rng.integers(0, hi + 1)) if rng.random() < 0.3 else int(rng.integers(0, 24))
            return bytes(rng.integers(33, 127, k, dtype=np.uint8))
        hdrs = [(_NAMES[int(rng.integers(0, len(_NAMES)))] if rng.random() < 0.7 else blob(40).lower(), blob())
                for _ in range(int(rng.integers(0, 13)))]
        bad = bads[int(rng.integers(0, len(bads)))] if rng.random() < 0.05 else None
        if bad == "dir_sum" and not hdrs:
            hdrs = [(b"a", b"b")]
        f = fields(method=[b"GET", b"POST", b"", None][int(rng.integers(0, 4))], path=blob() if rng.random() < 0.9 else None,
                   authority=blob(60) if rng.random() < 0.8 else None, headers=hdrs,
                   remote_id=int(rng.integers(0, 2 ** 32)) if rng.random() < 0.8 else 0,
                   dport=int(rng.integers(1, 65536)), ingress=bool(rng.random() < 0.6), bad=bad, raw=True)
        v = VERDICTS[int(rng.integers(0, len(VERDICTS)))] if rng.random() < 0.7 else int(rng.integers(0, 50))
        out.append((f, v))
    return out


# ---- the expected entry, from a case's fields ---------------------------------
def _varint(v):
    out = b""
    while v >= 0x80:
        out += bytes([v & 0x7F | 0x80])
        v >>= 7
    return out + bytes([v])


def _u(field, v):
    return bytes([field << 3]) + _varint(v) if v else b""


def _s(field, b):
    return bytes([field << 3 | 2]) + _varint(len(b)) + b if b else b""


def expected_entry(f, verdict, select=0, policy_name="", timestamp_ns=0, http_protocol=1, local_identity=0,
                   source_address=None, destination_address=None):
    """proto3 serialisation of the HttpLogEntry (envoy/cilium/accesslog.proto) of a case; b"" for a
    malformed one, a verdict at or below VERDICT_PARSE_ERROR or one outside `select`."""
    verdict = verdict - (1 << 32) if verdict >= 1 << 31 else verdict
    denied = verdict == L.VERDICT_DENY
    if f["bad"] or verdict <= L.VERDICT_PARSE_ERROR or (select and not select & (L.LOG_DENIED if denied else L.LOG_FORWARDED)):
        return b""
    ingress = bool(f["flags"] & L.F_INGRESS)
    schemes = [v for n, v in f["headers"] if n == XFP]
    out = _u(1, timestamp_ns) + _u(2, http_protocol) + _u(3, 2 if denied else 0) + _s(4, policy_name.encode())
    out += _u(6, f["remote_id"] if ingress else local_identity)
    out += _s(7, (source_address or "").encode()) + _s(8, (destination_address or "").encode())
    out += _s(9, schemes[-1] if schemes else b"")
    for field, flag, key in ((10, L.F_AUTHORITY, "authority"), (11, L.F_PATH, "path"), (12, L.F_METHOD, "method")):
        if f["flags"] & flag:
            out += _s(field, f[key] or b"")
    out += _u(13, 403 if denied else 0)
    for n, v in f["headers"]:
        if n != XFP:
            kv = _s(1, n) + _s(2, v)
            out += bytes([14 << 3 | 2]) + _varint(len(kv)) + kv
    return out + _u(15, 1 if ingress else 0)


def expected_stats(cases, port=0, ingress=True):
    """ProxyStatsTable.entries() after an HTTP update with these cases."""
    out = {}
    for f, v in cases:
        v = v - (1 << 32) if v >= 1 << 31 else v
        key = ("http", port, ingress, True) if f["bad"] else ("http", f["dport"], bool(f["flags"] & L.F_INGRESS), True)
        e = out.setdefault(key, {"received": 0, "forwarded": 0, "denied": 0, "error": 0})
        e["received"] += 1
        e["forwarded" if v >= 0 else "denied" if v == L.VERDICT_DENY else "error"] += 1
    return out


def dump(path, cases, **opts):
    """What tests/cpp/http_log_asan.cc reads: the batch and the entries expected_entry gives for it."""
    arena, offs, verdicts = build(cases)
    entries = [expected_entry(f, v, **opts) for f, v in cases]
    eo = np.zeros(len(cases) + 1, dtype=np.uint64)
    eo[1:] = np.cumsum([len(e) for e in entries], dtype=np.uint64)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<IQ", len(cases), arena.nbytes))
        fh.write(offs.tobytes() + arena.tobytes() + verdicts.tobytes() + eo.tobytes() + b"".join(entries))
