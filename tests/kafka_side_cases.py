"""Kafka requests for the deny-response and log-record tests: a table of
requests by construction (the request through kafka_wire's builders, the
expected response through kafka_wire.deny_response, neither through the
library), seeded random and mutated ones (expectation: the per-request host
function), and the verdict vector both meet.  Used by
tests/test_kafka_side_cpu.py, tests/test_kafka_side_gpu.py and the stand-alone
sanitizer program tests/cpp/kafka_side_asan.cc (dump)."""
import ctypes
import functools
import struct

import numpy as np

import kafka_wire as K
from cilium_amd import l7match as L

# every verdict class; each case of the table and each request of the fuzz set meets every entry
VERDICTS = [3, 0, L.VERDICT_DENY, L.VERDICT_DENY, L.VERDICT_PARSE_ERROR, L.VERDICT_UNSUPPORTED, L.VERDICT_ALLOW_NO_L7]
TOPICS = [("t1", [0, 3]), ("topic-two", [7])]
MS = K.message_set(["v"], version=1)


def with_correlation(req, correlation):
    return req[:8] + struct.pack(">i", correlation) + req[12:]


def request_of(kind, version, correlation, topics):
    """The request of a tuple: topics [(name, [partition ids])]."""
    if kind == K.PRODUCE:
        req = K.produce(version, "c", [(n, [(p, MS) for p in ps]) for n, ps in topics])
    elif kind == K.FETCH:
        req = K.fetch(version, "c", topics)
    elif kind == K.OFFSETS:
        req = K.offsets(version, "c", topics)
    elif kind == K.METADATA:
        req = K.metadata(version, "c", [n for n, _ in topics])
    elif kind == K.OFFSET_COMMIT:
        req = K.offset_commit(version, "c", "g", topics)
    elif kind == K.OFFSET_FETCH:
        req = K.offset_fetch(version, "c", "g", topics)
    elif kind == K.CONSUMER_METADATA:
        req = K.consumer_metadata(version, "c", "g")
    else:
        raise ValueError(kind)
    return with_correlation(req, correlation)


def response_of(kind, version, correlation, topics):
    """The response of a tuple; a null name (None) decodes to ""."""
    topics = [(n or "", ps) for n, ps in topics]
    return K.deny_response(kind, version, correlation, [n for n, _ in topics] if kind == K.METADATA else topics)


def case(name, req, resp=b"", head=None, names=(), bad=None):
    """req: the record's bytes.  resp: the response a denied request gets (b"": none).  head:
    (kind, version, correlation) and names: the topics its log records carry.  bad: how the record
    or its offset leaves the arena."""
    return dict(name=name, req=req, resp=resp, head=head, names=[n or "" for n in names], bad=bad)


def by_tuple(name, kind, version, correlation, topics):
    return case(name, request_of(kind, version, correlation, topics), response_of(kind, version, correlation, topics),
                (kind, version, correlation), [n for n, _ in topics])


def _produce_raw(version, name, n_partitions, partitions):
    """A Produce of one topic whose partition bytes are given as they stand."""
    body = (K.s(None) if version >= 3 else b"") + struct.pack(">hi", -1, 1000) + struct.pack(">i", 1)
    return K.request(K.PRODUCE, version, "c", body + K.s(name) + struct.pack(">i", n_partitions) + partitions)


def _table():
    kinds = [("produce", K.PRODUCE, 4), ("fetch", K.FETCH, 6), ("offsets", K.OFFSETS, 3), ("metadata", K.METADATA, 5),
             ("offset_commit", K.OFFSET_COMMIT, 3), ("offset_fetch", K.OFFSET_FETCH, 3),
             ("consumer_metadata", K.CONSUMER_METADATA, 2)]
    t = []
    for label, kind, versions in kinds:
        for v in range(versions):
            topics = [] if kind == K.CONSUMER_METADATA else TOPICS
            t.append(by_tuple(f"{label}_v{v}", kind, v, 0x01020304 + v, topics))
            if kind != K.CONSUMER_METADATA:
                t.append(by_tuple(f"{label}_v{v}_zero_topics", kind, v, -2, []))
    for label, kind, versions in kinds[:6]:
        v = versions - 1
        if kind != K.METADATA:
            t.append(by_tuple(f"{label}_topic_with_zero_partitions", kind, v, 7, [("a", []), ("bc", [1])]))
        t.append(by_tuple(f"{label}_empty_topic_name", kind, v, 8, [("", [4]), ("x", [5])]))
        t.append(by_tuple(f"{label}_null_topic_name", kind, v, 9, [(None, [4])]))
        for k in range(1, 6):  # responses that end at every byte phase
            t.append(by_tuple(f"{label}_name_of_{k}", kind, v, k, [("n" * k, [k])]))
    t.append(by_tuple("metadata_300_topics", K.METADATA, 1, 300, [(f"topic-{i}", []) for i in range(300)]))
    t.append(by_tuple("fetch_40_topics_25_partitions", K.FETCH, 5, 4025,
                      [(f"t{i}", list(range(i, i + 25))) for i in range(40)]))
    # readMessageSet stops inside a set; the next partition is read from there
    stop = K.message_set(["z"], version=1, compression=3)
    tail = struct.pack(">ii", 9, 0)  # read as the next partition's id and set size
    t.append(case("produce_attributes_3_with_tail", K.produce(1, "c", [("t", [(5, stop + tail)])]),
                  response_of(K.PRODUCE, 1, 1, [("t", [5])]), (K.PRODUCE, 1, 1), ["t"]))
    # a bad CRC in the first of two messages: what follows in the set (the second message: offset 1,
    # its size) is read as the next partition, id 0 with a set of one byte; the array of two ends
    # there and the partition the request wrote next (6) is never read
    bad = K.message_set(["a", "b"], version=0, bad_crc_at=0)
    good = K.message_set(["c"], version=0)
    t.append(case("produce_bad_crc_then_second_partition", K.produce(2, "c", [("t", [(5, bad), (6, good)])]),
                  response_of(K.PRODUCE, 2, 1, [("t", [5, 0])]), (K.PRODUCE, 2, 1), ["t"]))
    one_bad = K.message_set(["a"], version=0, bad_crc_at=0)
    t.append(case("produce_bad_crc_tail_read_as_second_partition",
                  _produce_raw(2, "t", 2, struct.pack(">ii", 5, len(one_bad + tail)) + one_bad + tail),
                  response_of(K.PRODUCE, 2, 1, [("t", [5, 9])]), (K.PRODUCE, 2, 1), ["t"]))
    big = K.message_set(["x" * 10_000] * 7, version=1)  # larger than any stage a kernel could hold
    assert len(big) >= 70_000
    t.append(case("produce_70000_byte_message_set", K.produce(3, "c", [("big", [(0, big)]), ("after", [(1, MS)])]),
                  response_of(K.PRODUCE, 3, 1, [("big", [0]), ("after", [1])]), (K.PRODUCE, 3, 1), ["big", "after"]))
    for kind, v in ((18, 0), (12, 0), (4, 1), (36, 2)):  # request == nil: no response, no records
        t.append(case(f"untyped_kind_{kind}", K.generic(kind, v)))
    t.append(case("six_byte_stub", b"\x00\x00\x00\x02\x00\x00"))
    t.append(case("fetch_cut_short", K.request(K.FETCH, 0, "c", K.fetch(0, "c", TOPICS)[15:40])))
    t.append(case("size_field_past_the_arena", K.fetch(0, "c", TOPICS), bad="size"))
    t.append(case("offset_past_the_arena", K.fetch(0, "c", TOPICS), bad="offset>end"))
    t.append(case("offset_two_before_the_end", K.fetch(0, "c", TOPICS), bad="offset=end-2"))
    return t


TABLE = _table()


def table_cases():
    return [(c, v) for c in TABLE for v in VERDICTS]


TOPIC_NAMES = ["orders", "payments", "t", "logs-eu-1", "x" * 40, ""]
CLIENTS = ["c", "client-7", ""]
FUZZ_SEED = 0  # the first seed whose share of answered requests lies inside FUZZ_SHARE (seeds 0-7 all do)
FUZZ_SHARE = (0.25, 0.75)


def fuzz_requests(n=2000, seed=FUZZ_SEED):
    """Random requests of every kind, every third one corrupted once."""
    rng = np.random.default_rng(seed)
    reqs = K.random_requests(rng, n, TOPIC_NAMES, CLIENTS)
    return [case(f"fuzz_{i}", K.mutate(rng, r) if i % 3 == 2 else r, resp=None) for i, r in enumerate(reqs)]


def fuzz_response_share(seed=FUZZ_SEED):
    """The share of the fuzz requests that get a non-empty response under VERDICTS, that is from the
    entries of it that deny: the others answer nobody."""
    arena, offs, verdicts = build([(c, L.VERDICT_DENY) for c in fuzz_requests(seed=seed)])
    resp = single_responses(arena, offs, verdicts)
    return sum(1 for r in resp if r) / len(resp)


@functools.lru_cache(maxsize=None)
def _fuzz_cases(seed):
    # a set of which nearly every or nearly no request had a response would exercise one branch only
    share = fuzz_response_share(seed)
    assert FUZZ_SHARE[0] <= share <= FUZZ_SHARE[1], f"seed {seed}: {share:.4f} of the fuzz requests get a response"
    return tuple((c, v) for c in fuzz_requests(seed=seed) for v in VERDICTS)


def fuzz_cases(seed=FUZZ_SEED):
    """The fuzz requests, each under every entry of VERDICTS (14,000 cases); asserts, once, that between
    a quarter and three quarters of the requests get a non-empty response."""
    return list(_fuzz_cases(seed))


def build(cases, pad=True):
    """cases: [(case, verdict)] -> (arena, offs, verdicts).  pad: records 4-aligned (pack_records);
    otherwise back to back, so most offsets are odd.  The cases that leave the arena are made to."""
    recs = []
    for c, _ in cases:
        r = c["req"]
        recs.append(struct.pack(">i", 0x7FFFFF00) + r[4:] if c["bad"] == "size" else r)
    if pad:
        arena, offs = L.pack_records(recs)
    else:
        arena = np.frombuffer(b"".join(recs) or b"\0", dtype=np.uint8).copy()
        offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])])[:-1].astype(np.uint64)
    end = arena.shape[0]
    for i, (c, _) in enumerate(cases):
        if c["bad"] == "offset>end":
            offs[i] = end + 4
        elif c["bad"] == "offset=end-2":
            offs[i] = end - 2
    return arena, offs, np.array([v for _, v in cases]).astype(np.uint32).view(np.int32)


def record_at(arena, off):
    """The size-prefixed request at an offset as the batch functions take it; None if it leaves the arena."""
    end, off = arena.shape[0], int(off)
    if off > end or end - off < 4:
        return None
    size = struct.unpack(">I", arena[off:off + 4].tobytes())[0]
    return arena[off:off + 4 + size].tobytes() if size <= end - off - 4 else None


def single_responses(arena, offs, verdicts):
    """What l7m_kafka_deny_responses owes: the per-request function's bytes for a denied request whose
    record lies in the arena, b"" where it answers anything but L7M_OK."""
    out = []
    for off, v in zip(offs, verdicts):
        rec = record_at(arena, off) if v == L.VERDICT_DENY else None
        try:
            out.append(L.kafka_deny_response(rec) if rec is not None else b"")
        except L.L7Error:
            out.append(b"")
    return out


def table_responses(cases):
    return [c["resp"] if v == L.VERDICT_DENY and not c["bad"] else b"" for c, v in cases]


def table_log(cases):
    """(request, verdict, error code, kind, version, correlation id, topic) of every record the table owes."""
    out = []
    for i, (c, v) in enumerate(cases):
        if c["head"] is None or c["bad"] or v in (L.VERDICT_PARSE_ERROR, L.VERDICT_UNSUPPORTED):
            continue
        fv = 1 if v == L.VERDICT_DENY else 0
        out += [(i, fv, 29 if fv else 0, *c["head"], n.encode()) for n in c["names"]]
    return out


def host_log(arena, offs, verdicts, select=0):
    """l7m_kafka_access_log's array -> (records as KAFKA_LOG_RECORD_DTYPE, first[n + 1]); select: only
    the records whose verdict is in it."""
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    v = np.ascontiguousarray(verdicts, dtype=np.int32)
    n = v.shape[0]
    f = L.lib().l7m_kafka_access_log
    need = f(arena.ctypes.data, arena.nbytes, offs.ctypes.data, n, v.ctypes.data, None, 0)
    assert need >= 0
    recs = np.zeros(need, dtype=L.KAFKA_LOG_RECORD_DTYPE)
    assert f(arena.ctypes.data, arena.nbytes, offs.ctypes.data, n, v.ctypes.data, recs.ctypes.data, need) == need
    if select:
        recs = recs[((recs["verdict"] == 0) & bool(select & L.LOG_FORWARDED)) |
                    ((recs["verdict"] == 1) & bool(select & L.LOG_DENIED))]
    first = np.zeros(n + 1, dtype=np.uint64)
    first[1:] = np.cumsum(np.bincount(recs["request"].astype(np.int64), minlength=n)[:n])
    return recs, first


def log_tuples(arena, recs):
    raw = arena.tobytes()
    return [(int(r["request"]), int(r["verdict"]), int(r["error_code"]), int(r["api_key"]), int(r["api_version"]),
             int(r["correlation_id"]), raw[int(r["topic_off"]):int(r["topic_off"]) + int(r["topic_len"])]) for r in recs]


def dump(path, cases):
    """What tests/cpp/kafka_side_asan.cc reads: the batch (records back to back, no padding), the
    responses (the table's by construction, the fuzz set's from the per-request function) and the
    log records l7m_kafka_access_log gives for it."""
    arena, offs, verdicts = build(cases, pad=False)
    single = single_responses(arena, offs, verdicts)
    resp = [s if c["resp"] is None else t for (c, _), s, t in zip(cases, single, table_responses(cases))]
    ro = np.zeros(len(cases) + 1, dtype=np.uint64)
    ro[1:] = np.cumsum([len(r) for r in resp], dtype=np.uint64)
    recs, _ = host_log(arena, offs, verdicts)
    assert recs.dtype.itemsize == ctypes.sizeof(L._KafkaLogRecord) == 40
    with open(path, "wb") as fh:
        fh.write(struct.pack("<IQQ", len(cases), arena.nbytes, len(recs)))
        fh.write(offs.tobytes() + arena.tobytes() + verdicts.tobytes() + ro.tobytes() + b"".join(resp) + recs.tobytes())
