"""Record-tile geometry of the two batch kernels (TEST INFRASTRUCTURE).

http_eval_body (cilium_amd/csrc/l7m_http_impl.h) and kafka_eval_body
(cilium_amd/csrc/l7m_kafka.hip) consume a wave's share of a batch in tiles of
<= 64 records; plan() stages the leading run of records that lie in order
inside a window of <= `stage` bytes and the rest is read from HBM.  This
module holds

  * a plain-Python model of that planner (plan_tiles, classify): NOT a
    reference for verdicts, only the proof that a test's inputs reach the
    planner branch the test is named after;
  * mirrors of the stage size each rule set gets (http_stage_bytes,
    kafka_stage_bytes);
  * generators of records of an exact size whose verdict is a function of a
    key and is decided by bytes at both ends of the record (http_record,
    kafka_record), the rule sets they are written for, and arena layouts
    built from them (layout).

The constants below restate the sources; tests/test_tile_geometry_cpu.py
reads them out of the sources and fails when they drift."""
import struct
from collections import Counter

import numpy as np

import kafka_wire as K
from cilium_amd import l7match as L
from raw_cases import pack_raw

# ---- geometry constants (pinned to the sources by the CPU test) -----------
HTTP_WAVES = 16            # program.h L7M_HTTP_WAVES
HTTP_MAX_STAGE = 8192      # program.h L7M_HTTP_MAX_STAGE
HTTP_MIN_STAGE = 2048      # program.h kHttpMinStage
HTTP_REG_DFAS = 8          # program.h kHttpRegDfas
MAX_LDS_COUNTERS = 8192    # program.h kMaxLdsCounters
MIN_STAGED_TAKE = 32       # l7m_http_impl.h kMinStagedTake
K_WAVES = 16               # l7m_kafka.hip kKWaves
K_MAX_STAGE = 6144         # l7m_kafka.hip kKMaxStage
LDS_BYTES = 160 * 1024     # program.h kLdsBytes, l7m_kafka.hip kKLdsBytes
WG_PER_CU = 1              # program.h L7M_HTTP_WG_PER_CU
NUM_CUS = 256
# l7m_kafka.hip / program.h: what the Kafka workgroup keeps in LDS before the stages
K_MAX_LDS_COUNTERS = 16384
K_KINDS = 65
K_SPAN_LDS = (4 * K_KINDS + 3) & ~3
K_KIND_OK_LDS = (2 * K_KINDS + 3) & ~3
K_TOPIC_Q = 4
K_CLIENT_SLOT_WORDS = 8
K_MAX_CLI_LDS_BYTES = 8192
SLOW_REC = 256             # l7m_http_impl.h kSlowRec: slow-pass LDS slot (records <= SLOW_REC - 32)

HTTP_CLASSES = ("full", "cut", "mixed", "prefetch_on", "prefetch_off", "none", "tail", "exact", "base_misaligned")
KAFKA_CLASSES = ("full", "partial", "none", "tail", "exact", "base_misaligned")


# ---- the planner model -----------------------------------------------------
def plan_tiles(offs, arena_bytes, stage, kernel):
    """[(wave, cur, m, k, take, bytes, base_misalign)] for every tile of the launch."""
    assert kernel in ("http", "kafka")
    offs = [int(x) for x in offs]
    n = len(offs)
    if n == 0:
        return []
    waves = HTTP_WAVES if kernel == "http" else K_WAVES
    per_block = 2 * 64 * waves
    blocks = min(NUM_CUS * (WG_PER_CU if kernel == "http" else 1), (n + per_block - 1) // per_block)
    nw = blocks * waves
    tiles = []
    for gw in range(nw):
        cur, end = n * gw // nw, n * (gw + 1) // nw
        while cur < end:
            m = min(64, end - cur)
            o0 = offs[cur]
            base = o0 & ~15
            k, nbytes = 0, 0
            for lane in range(m):
                o = offs[cur + lane]
                onext = offs[cur + lane + 1] if cur + lane + 1 < n else arena_bytes
                if not ((o & 3) == 0 and o >= o0 and onext >= o and onext <= arena_bytes and onext - base <= stage):
                    break
                k, nbytes = k + 1, onext - base
            if kernel == "http":
                take = k if k >= MIN_STAGED_TAKE else m
            else:
                take = k if k else 1
            tiles.append((gw, cur, m, k, take, nbytes, o0 & 15))
            cur += take
    return tiles


def classify(tiles, stage, kernel="http"):
    """Tiles per class (a tile may be in several)."""
    c = Counter({name: 0 for name in (HTTP_CLASSES if kernel == "http" else KAFKA_CLASSES)})
    for _, _, m, k, _, nbytes, mis in tiles:
        if k == 64:
            c["full"] += 1
        if kernel == "http":
            if 32 <= k < m:
                c["cut"] += 1
            if 0 < k < 32 and k < m:
                c["mixed"] += 1
                c["prefetch_on" if nbytes + 256 <= stage else "prefetch_off"] += 1
        elif 0 < k < m:
            c["partial"] += 1
        if k == 0:
            c["none"] += 1
        if m < 64:
            c["tail"] += 1
        if k and nbytes == stage:
            c["exact"] += 1
        if mis:
            c["base_misaligned"] += 1
    return c


# ---- stage mirrors -----------------------------------------------------------
_HTTP_HDR = {"n_rules": 1, "n_dfas": 3, "lds_image_words": 18, "search": 36}  # program_interp.HDR_FIELDS


def _http_hdr(program):
    if hasattr(program, "h"):  # program_interp.HttpProgram
        return program.h
    w = np.ascontiguousarray(program, dtype=np.uint32)
    return {name: int(w[i]) for name, i in _HTTP_HDR.items()}


def http_lds_bytes(program, stage):
    """l7m_kernels.hip http_lds_bytes."""
    h = _http_hdr(program)
    reg = h["n_dfas"] <= HTTP_REG_DFAS or h["search"] != 0
    ctr = (h["n_rules"] + 2 + 3) & ~3 if h["n_rules"] + 2 <= MAX_LDS_COUNTERS else 0
    return 4 * (h["lds_image_words"] + ctr + (0 if reg else h["n_dfas"] * 64 * HTTP_WAVES)) + HTTP_WAVES * (stage + 16)


def http_stage_bytes(program):
    """l7m_kernels.hip http_stage_bytes: what the LDS leaves after the tables."""
    lds = LDS_BYTES // WG_PER_CU
    fixed = http_lds_bytes(program, 0) - HTTP_WAVES * 16
    if fixed + HTTP_WAVES * (256 + 16) > lds:
        return 0
    s = ((lds - fixed) // HTTP_WAVES - 16) & ~15
    return min(s, HTTP_MAX_STAGE)


def kafka_stage_bytes(program, hits=True):
    """l7m_kafka.hip kafka_stage as launch_kafka calls it (KafkaHeader words:
    [1] n_rules, [10] n_clients)."""
    w = np.ascontiguousarray(program, dtype=np.uint32)
    n_ctr, n_clients = int(w[1]) + 2, int(w[10])
    cli_words = n_clients * K_CLIENT_SLOT_WORDS
    cli_lds = cli_words != 0 and cli_words * 4 <= K_MAX_CLI_LDS_BYTES
    lds_hits = hits and n_ctr <= K_MAX_LDS_COUNTERS
    fixed = 4 * (256 + K_SPAN_LDS + K_KIND_OK_LDS + (cli_words if cli_lds else 0) +
                 (((n_ctr + 3) & ~3) if lds_hits else 0)) + 2 * K_WAVES * 64 * K_TOPIC_Q
    s = ((LDS_BYTES - fixed) // K_WAVES - 16) & ~15
    return min(s, K_MAX_STAGE)


# ---- records of a controlled size ----------------------------------------------
def outcome(key):
    """key -> 0..5, aperiodic along a counter (splitmix64 finaliser)."""
    x = (int(key) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return int((x ^ (x >> 31)) % 6)


# Six outcomes over a front choice (A / B) and a tail choice (a / b / c), five
# verdicts.  Flipping the front (A <-> B) or the tail's last bit (a -> `, b <->
# c) of any of them gives another verdict:
#   0 (A,a) -> rule 0    1 (B,a) -> rule 1    2 (A,c) -> rule 2
#   3 (B,b) -> rule 3    4 (A,b) -> deny      5 (B,c) -> deny
_FRONT = (0, 1, 0, 1, 0, 1)
_TAIL = (b"a", b"a", b"c", b"b", b"b", b"c")
INTENDED = (0, 1, 2, 3, L.VERDICT_DENY, L.VERDICT_DENY)


def intended(key):
    return INTENDED[outcome(key)]


# HTTP: the method ("GET" / "FET", the first value byte of the record) and the
# value of the last header "k" (the last byte of the record) decide.
HTTP_METHODS = (b"GET", b"FET")
HTTP_MIN = 32
HTTP_MAX = 4 * HTTP_MAX_STAGE
# flavour 1's pad: the value of the referenced header "lit", the rule's literal
# up to its last byte (repeated for longer pads, so it never holds the literal)
LIT = (b"0123456789abcdefghijklmnopqrstuv" * 32)[:1000] + b"Z"  # (the pad of a 1040-byte record)
SLOW_PATH_HIT, SLOW_PATH_MISS = b"/abcaz", b"/abcbz"  # /(a)(b|c)*\1z


def http_core_rules():
    return [L.PortRuleHTTP(Method="GET", Headers=["k: a"]), L.PortRuleHTTP(Method="FET", Headers=["k: a"]),
            L.PortRuleHTTP(Method="GET", Headers=["k: c"]), L.PortRuleHTTP(Method="FET", Headers=["k: b"])]


def http_record_fields(size, key, flavour=0, path=b"/p"):
    """The (method, path, host, headers) of http_record."""
    oc = outcome(key)
    fixed = 20 + 4 + 3 + len(path) + 1 + 1 + 1  # header, directory entry, method, path, host "h", "k", value
    assert size % 4 == 0 and fixed <= size <= HTTP_MAX + 64, size
    rest = size - fixed
    host, hdrs = b"h", []
    name = b"lit" if flavour else b"p"
    if rest < 4 + len(name) + 1:
        host += b"x" * rest
    else:
        n = rest - 4 - len(name)
        pad = (LIT[:-1] * (n // (len(LIT) - 1) + 1))[:n - 1] + b"!" if flavour else bytes([0x41 + key % 26]) * n
        hdrs.append((name, pad))
    hdrs.append((b"k", _TAIL[oc]))
    return HTTP_METHODS[_FRONT[oc]], path, host, hdrs


def http_record(size, key, flavour=0, path=b"/p"):
    """An HTTP record of exactly `size` bytes (a multiple of 4, >= HTTP_MIN for
    the default path) whose verdict under http_core_rules() is intended(key).
    The pad is the value of an unreferenced header in front of the deciding
    one (flavour 0), or of the referenced header "lit": LIT with another last
    byte (flavour 1)."""
    arena, _ = pack_raw([http_record_fields(size, key, flavour, path)])
    rec = arena.tobytes()
    assert len(rec) == size and struct.unpack_from("<I", rec)[0] == size
    return rec


def http_front_index(rec):
    """Index of the first deciding byte (the method's first byte)."""
    return 20 + 4 * rec[11]


def http_rules(kind):
    """(rules, compile_http keywords, HttpOracle keywords) of a program kind."""
    core = http_core_rules()
    lit = [L.PortRuleHTTP(Path="/p", Headers=[b"lit: " + LIT])]
    if kind == "default":  # <= 4 value automata
        return core + lit, {}, {}
    if kind == "columns":  # > 8 value automata: end codes in LDS columns, a smaller stage
        extra = [L.PortRuleHTTP(Path="/p[0-9]*", Headers=[f"x-h{j}: v{j}[0-9]*", f"x-h{(j + 1) % 9}"])
                 for j in range(9)]
        return core + lit + extra, {}, {}
    if kind == "dense":
        return core + lit + [L.PortRuleHTTP(Path="/(?!q)[a-z]+", Method="PUT")], \
            {"dense_dfa": L.OPT_DENSE_DFA_ALWAYS, "lds_budget_bytes": 1}, {}
    if kind == "re2":
        return core + lit + [L.PortRuleHTTP(Path="bcb", Method="^FET$")], \
            {"dialect": L.DIALECT_RE2_SEARCH}, {"dialect": L.DIALECT_RE2_SEARCH}
    if kind == "slow":  # a back-reference with a loop inside the group: decided by http_slow_kernel
        return core + lit + [L.PortRuleHTTP(Path="/(a)(b|c)*\\1z")], {}, {}
    raise ValueError(kind)


HTTP_KINDS = ("default", "columns", "dense", "re2", "slow")
SLOW_RULE = 5  # index of the back-reference rule of kind "slow"


def http_paths(kind):
    """Paths the layouts of a kind draw from (by key)."""
    if kind == "slow":
        return (b"/p", SLOW_PATH_HIT, SLOW_PATH_MISS, SLOW_PATH_HIT)
    if kind == "re2":
        return (b"/p", b"/abcbz")
    return (b"/p",)


# Kafka: a Metadata request.  ApiVersion (0 / 1, bytes 6-7) at the front and
# the last topic name ("topic-b" + a / b / c, the last byte of the record)
# decide; the pad is the ClientID.
KAFKA_MIN = 28
KAFKA_MAX = KAFKA_MIN + 32767
_K_TOPIC = b"topic-b"


def kafka_rules():
    return [L.PortRuleKafka(APIKey="metadata", APIVersion="0", Topic="topic-ba"),
            L.PortRuleKafka(Role="consume", APIVersion="1", Topic="topic-ba"),
            L.PortRuleKafka(APIKey="metadata", APIVersion="0", Topic="topic-bc"),
            L.PortRuleKafka(Role="consume", APIVersion="1", Topic="topic-bb"),
            L.PortRuleKafka(APIKey="metadata", ClientID="BBBB", Topic="topic-qq"),
            L.PortRuleKafka(APIKey="produce", ClientID="some-other-client", Topic="topic-ba")]


def kafka_record(size, key):
    """A Kafka Metadata request of exactly `size` bytes (a multiple of 4, >=
    KAFKA_MIN) whose verdict under kafka_rules() is intended(key)."""
    oc = outcome(key)
    assert size % 4 == 0 and KAFKA_MIN <= size <= KAFKA_MAX, size
    client = bytes([0x41 + key % 26]) * (size - KAFKA_MIN)
    rec = K.metadata(_FRONT[oc], client, [_K_TOPIC + _TAIL[oc]])
    assert len(rec) == size
    return rec


KAFKA_FRONT_INDEX = 7  # low byte of ApiVersion
KAFKA_MANY = 16000  # further rules whose LDS hit counters leave a stage below kKMaxStage


# ---- layouts ---------------------------------------------------------------------
def _r4(x):
    return (int(x) + 3) & ~3


def segment_sizes(stage, kernel, seed=0, tail_run=True):
    """Record sizes of one layout: runs of uniform size around the stage's
    thresholds, a random mix of 24 B .. 4 x stage (no smaller than the smallest
    record the generators build), and a closing run of small records (the last
    staged run ends at arena_bytes)."""
    lo = HTTP_MIN if kernel == "http" else KAFKA_MIN
    rng = np.random.default_rng(1000 + seed)
    sizes = []

    def run(size, count):
        sizes.extend([max(lo, _r4(size))] * count)

    def windows(per, count):
        """`count` windows of `per` records that fill the stage exactly, the
        first at a 16-byte boundary (of a layout with lead 0): records of
        stage / per bytes; where that is no multiple of 16 the last record of
        each window takes the remainder."""
        pos = sum(sizes)
        if pos % 16:
            sizes.append(lo + (-(pos + lo)) % 16)
        s = (stage // per) & ~15
        sizes.extend(([s] * (per - 1) + [stage - (per - 1) * s]) * count)
        return s

    s64 = windows(64, 7)
    run(s64 + 4, 320)
    s32 = windows(32, 8)
    run(s32 + 4, 256)
    run(stage / 31, 192)
    run(stage // 2, 40)
    run(stage - 16, 24)
    windows(1, 24)
    run(stage + 4, 24)
    windows(64, 3)
    # the mix: log-uniform sizes, so most tiles hold a few small records in front of a large one
    mix = np.exp(rng.uniform(np.log(24), np.log(4 * stage), size=640))
    sizes.extend(max(lo, _r4(s)) for s in mix)
    run(stage // 4 + 4, 64)
    if tail_run:
        run(s64, 128)
    return sizes


def build_arena(records, lead=0):
    """(arena, offs): the records back to back, the first at offset `lead`
    (filler bytes in front of it), no slack after the last."""
    offs = np.zeros(len(records), dtype=np.uint64)
    total = lead
    for i, r in enumerate(records):
        assert len(r) % 4 == 0
        offs[i] = total
        total += len(r)
    arena = np.frombuffer(b"\xa5" * lead + b"".join(records), dtype=np.uint8).copy()
    assert arena.nbytes == total
    return arena, offs


def layout(stage, kernel, seed=0, lead=0, kind="default"):
    """(arena, offs) of <= 4096 records: segment_sizes(stage) filled with
    records keyed by a counter, the first record at arena offset `lead`."""
    sizes = segment_sizes(stage, kernel, seed)
    assert len(sizes) <= 4096
    if kernel == "kafka":
        recs = [kafka_record(s, 7919 * seed + i) for i, s in enumerate(sizes)]
        return build_arena(recs, lead)
    paths = http_paths(kind)
    reqs = []
    for i, s in enumerate(sizes):
        key = 7919 * seed + i
        path = paths[outcome(key * 31 + 5) % len(paths)]
        if s < _r4(30 + len(path)):  # (the smallest records have room for the short path only)
            path = b"/p"
        reqs.append(http_record_fields(s, key, flavour=(key // 3) & 1, path=path))
    arena, offs = pack_raw(reqs)
    if lead:
        arena = np.concatenate([np.full(lead, 0xA5, dtype=np.uint8), arena])
        offs = offs + np.uint64(lead)
    return arena, offs


def lookup(arena, offs, table):
    """Expected verdicts of an offsets array over an arena whose per-record
    oracle verdicts are `table` ({offset: verdict}); any other entry is bad."""
    return np.array([table.get(int(o), L.VERDICT_PARSE_ERROR) for o in offs], dtype=np.int32)
