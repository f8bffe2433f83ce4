"""The record-tile planner of http_eval_body (l7m_http_impl.h) and
kafka_eval_body (l7m_kafka.hip) at its edges: tiles of 31 / 32 / 33 / 63 / 64
staged records, windows that end exactly at the stage or 4 bytes past it,
tile bases 4 / 8 / 12 bytes below the first record, bad offsets at chosen
lanes, reordered, repeated, gapped and overlapping offsets, waves with empty
and one-record shares.

Both oracles decide a record from (arena, arena_bytes, offset) alone, so the
expected verdicts of any offsets array over an arena are a lookup in the
oracle's verdicts of that arena's records (bad entries: PARSE_ERROR).  Every
test first proves with the planner model (tile_geometry.plan_tiles) that its
input reaches the branch it is named after, then requires bit-exact verdicts
and hit counters.  The same records are evaluated from LDS in one test and
from HBM in another, by every program kind with Src-specific code."""
import functools
import struct

import numpy as np
import pytest

import tile_geometry as G
from cilium_amd import l7match as L
from oracle import HttpOracle, KafkaOracle
from program_interp import HttpProgram

pytestmark = pytest.mark.gpu

LEADS = (0, 4, 8, 12)
ERR = L.VERDICT_PARSE_ERROR
BATCH_SIZES = {1: {0, 1}, 2: {0, 1}, 15: {0, 1}, 16: {1}, 17: {1, 2}, 63: {3, 4}, 64: {4}, 65: {4, 5},
               1023: {63, 64}, 1024: {64}, 1025: {64, 65}, 2047: {127, 128}, 2048: {128}, 2049: {64, 65},
               4095: {127, 128}, 4096: {128}}  # n: the wave shares it gives


# ---- rule sets, arenas and oracle verdicts, built once ---------------------------
class _Http:
    kernel = "http"

    def __init__(self, kind):
        rules, ckw, okw = G.http_rules(kind)
        self.kind = kind
        self.rs = L.RuleSet.compile_http(rules, **ckw)
        self.orc = HttpOracle(rules, **okw)
        self.prog = HttpProgram(self.rs.program())
        self.stage = G.http_stage_bytes(self.prog)
        assert G.HTTP_MIN_STAGE <= self.stage <= G.HTTP_MAX_STAGE

    def oracle(self, arena, offs, ids=None):
        return self.orc.eval(arena, offs, threads=8)

    def layout(self, lead):
        return G.layout(self.stage, "http", seed=1, lead=lead, kind=self.kind)

    def records(self, sizes, seed):
        paths = G.http_paths(self.kind)
        out = []
        for i, s in enumerate(sizes):
            key = 104729 * seed + i
            path = paths[G.outcome(key * 31 + 5) % len(paths)]
            out.append(G.http_record(s, key, (key // 3) & 1, path if s >= 40 else b"/p"))
        return out


class _Kafka:
    kernel = "kafka"

    def __init__(self, kind):
        rules = G.kafka_rules()
        if kind == "many":
            rules = rules + [L.PortRuleKafka(APIKey="fetch", Topic=f"unused-{i}") for i in range(G.KAFKA_MANY)]
        self.kind = kind
        self.rs = L.RuleSet.compile_kafka(rules)
        self.orc = KafkaOracle(rules)
        self.stage = G.kafka_stage_bytes(self.rs.program())
        assert 1024 <= self.stage <= G.K_MAX_STAGE

    def oracle(self, arena, offs, ids=None):
        return self.orc.eval(arena, offs, threads=8, identities=ids)

    def layout(self, lead):
        return G.layout(self.stage, "kafka", seed=1, lead=lead)

    def records(self, sizes, seed):
        return [G.kafka_record(s, 104729 * seed + i) for i, s in enumerate(sizes)]


@functools.lru_cache(maxsize=None)
def _side(kernel, kind):
    return _Http(kind) if kernel == "http" else _Kafka(kind)


@functools.lru_cache(maxsize=None)
def _layout(kernel, kind, lead):
    """(arena, offs, oracle verdicts, {offset: verdict}) of one layout."""
    s = _side(kernel, kind)
    arena, offs = s.layout(lead)
    exp = s.oracle(arena, offs)
    assert set(G.INTENDED) <= set(exp.tolist()) and (exp != ERR).all()
    for a in (arena, offs, exp):
        a.setflags(write=False)
    return arena, offs, exp, dict(zip(offs.tolist(), exp.tolist()))


@functools.lru_cache(maxsize=None)
def _dense(kernel, kind, n=4096):
    """n small records in order (64 fill a stage exactly), a few large ones among them."""
    s = _side(kernel, kind)
    small = (s.stage // 64) & ~15
    sizes = [s.stage // 2 if i % 97 == 50 else s.stage + 4 if i % 211 == 100 else small for i in range(n)]
    arena, offs = G.build_arena(s.records(sizes, 2))
    exp = s.oracle(arena, offs)
    assert set(G.INTENDED) <= set(exp.tolist())
    for a in (arena, offs, exp):
        a.setflags(write=False)
    return arena, offs, exp, dict(zip(offs.tolist(), exp.tolist()))


SIDES = [("http", k) for k in G.HTTP_KINDS] + [("kafka", "default")]
SIDE_IDS = [f"{a}-{b}" for a, b in SIDES]
LAYOUT_SIDES = SIDES + [("kafka", "many")]


def _tiles(s, arena, offs):
    tiles = G.plan_tiles(offs, arena.nbytes, s.stage, s.kernel)
    assert sum(t[4] for t in tiles) == len(offs)
    return tiles


def _run(s, arena, offs, exp, ids=None):
    """rs.eval == exp bit for bit, and the hit counters count exp."""
    assert len(offs) <= 4096
    exp = np.asarray(exp, dtype=np.int32)
    h = np.zeros(s.rs.n_counters, dtype=np.uint64)
    got = s.rs.eval(arena, offs, h, identities=ids)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (len(bad), [(int(i), int(offs[i]), int(exp[i]), int(got[i])) for i in bad[:10]])
    assert (exp >= L.VERDICT_UNSUPPORTED).all() and (exp < s.rs.n_rules).all()
    assert int(h[0]) == int((exp == L.VERDICT_DENY).sum())
    assert int(h[1]) == int((exp <= ERR).sum())
    counts = np.bincount(exp[exp >= 0], minlength=s.rs.n_rules)
    assert h[2:2 + s.rs.n_rules].tolist() == counts.tolist()
    assert int(h.sum()) == len(exp)
    return got


# ---- the layouts ------------------------------------------------------------------------
def test_program_kinds():
    """The five HTTP programs are the kinds they are named after."""
    h = {k: _side("http", k) for k in G.HTTP_KINDS}
    assert h["default"].prog.h["n_dfas"] <= 4 and h["default"].stage == G.HTTP_MAX_STAGE
    assert h["columns"].prog.h["n_dfas"] > G.HTTP_REG_DFAS and h["columns"].stage < G.HTTP_MAX_STAGE
    assert h["dense"].rs.info.n_dense_dfas > 0
    assert h["re2"].prog.h["search"] != 0
    assert h["slow"].prog.h["n_slow"] > 0
    assert _side("kafka", "many").stage < _side("kafka", "default").stage == G.K_MAX_STAGE


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("kernel,kind", LAYOUT_SIDES, ids=SIDE_IDS + ["kafka-many"])
def test_layouts_match_oracle(gpu, kernel, kind, lead):
    s = _side(kernel, kind)
    arena, offs, exp, _ = _layout(kernel, kind, lead)
    assert int(offs[0]) == lead and arena.ctypes.data % 16 == 0
    tiles = _tiles(s, arena, offs)
    c = G.classify(tiles, s.stage, s.kernel)
    always = ("cut", "mixed", "prefetch_on", "prefetch_off", "none", "tail", "base_misaligned") \
        if kernel == "http" else ("partial", "none", "tail", "base_misaligned")
    assert all(c[name] >= 2 for name in always), c
    if lead == 0:  # the windows start at 16-byte boundaries: whole tiles that end exactly at the stage
        assert c["full"] >= 2 and c["exact"] >= 2, c
        assert tiles[0][2:] == (64, 64, 64, s.stage, 0)
    else:  # the same sizes `lead` bytes later: the window's last record no longer fits
        assert tiles[0][2:] == (64, 63, 63, int(offs[63]), lead), tiles[0]
    assert tiles[-1][2] == tiles[-1][3] and int(offs[-1]) < arena.nbytes  # the last staged run ends at arena_bytes
    if kind == "slow":
        assert (exp == G.SLOW_RULE).sum() > 50
    _run(s, arena, offs, exp)


def _gapped(v):
    """Indices 0 = i0 < i1 < ... with a record between each pair whose verdict differs from both."""
    keep, i, n = [0], 0, len(v)
    while True:
        nxt = next((j for j in range(i + 2, n)
                    if any(v[g] != v[i] and v[g] != v[j] for g in range(i + 1, j))), None)
        if nxt is None:
            return keep
        keep.append(nxt)
        i = nxt


@pytest.mark.parametrize("kernel,kind", SIDES, ids=SIDE_IDS)
def test_offsets_order_is_irrelevant(gpu, kernel, kind):
    s = _side(kernel, kind)
    arena, offs, exp, table = _layout(kernel, kind, 4)
    n = len(offs)
    rng = np.random.default_rng(5)
    # reversed: no lane's successor lies behind it
    order = offs[::-1]
    assert all(t[3] <= 1 for t in _tiles(s, arena, order))
    _run(s, arena, order, G.lookup(arena, order, table))
    # blocks of 64 in order, the blocks shuffled: runs end where a block does
    blocks = [offs[i:i + 64] for i in range(0, n, 64)]
    order = np.concatenate([blocks[i] for i in rng.permutation(len(blocks))])
    tiles = _tiles(s, arena, order)
    assert sum(1 for t in tiles if 0 < t[3] < t[2]) >= 10 and any(t[3] >= 32 for t in tiles)
    _run(s, arena, order, G.lookup(arena, order, table))
    # every 7th entry swapped with its successor: the run breaks mid-tile
    order = offs.copy()
    for i in range(6, n - 1, 7):
        order[i], order[i + 1] = order[i + 1], order[i]
    tiles = _tiles(s, arena, order)
    assert max(t[3] for t in tiles) <= 7 and sum(1 for t in tiles if 0 < t[3] < t[2]) >= 10
    _run(s, arena, order, G.lookup(arena, order, table))
    # each offset three times in a row: a staged lane whose successor is itself
    order = np.repeat(offs[:1365], 3)
    assert sum(1 for t in _tiles(s, arena, order) if t[3] >= 6) >= 10
    _run(s, arena, order, G.lookup(arena, order, table))
    # a subset with gaps: whole valid records lie between a lane's record and its successor
    keep = _gapped(exp.tolist())
    assert len(keep) > n // 4
    order = offs[keep]
    assert sum(1 for t in _tiles(s, arena, order) if t[3] >= 8) >= 10
    _run(s, arena, order, exp[keep])


@pytest.mark.parametrize("kernel,kind", SIDES, ids=SIDE_IDS)
def test_bad_offsets_inside_tiles(gpu, kernel, kind):
    """4096 small records, every tile whole in the clean case; then one bad
    offset in the first tile of a wave (so no earlier cut tile moves it), at
    lane 0 / 1 / 31 / 32 / 33 / 62 / 63, of four kinds, and the first and last
    record of the batch bad."""
    s = _side(kernel, kind)
    small = (s.stage // 64) & ~15
    arena, offs = G.build_arena(s.records([small] * 4096, 3))
    exp = s.oracle(arena, offs)
    assert set(G.INTENDED) <= set(exp.tolist())
    clean = _tiles(s, arena, offs)
    assert len(clean) == 64 and all(t[2:5] == (64, 64, 64) and t[6] == 0 for t in clean)
    _run(s, arena, offs, exp)
    nb = arena.nbytes
    kinds = [lambda o: o + 2, lambda o: nb, lambda o: nb + 4096, lambda o: 2 ** 40]
    lanes = (0, 1, 31, 32, 33, 62, 63)
    bad, want = offs.copy(), exp.copy()
    for j, lane in enumerate(lanes):
        for q, f in enumerate(kinds):
            i = 128 * (4 * j + q + 1) + lane
            bad[i], want[i] = f(int(offs[i])), ERR
    for i, f in ((128 * 30 + 5, kinds[0]), (128 * 29 + 104, kinds[1]), (0, kinds[3]), (4095, kinds[2])):
        bad[i], want[i] = f(int(offs[i])), ERR
    tiles = _tiles(s, arena, bad)
    # (the lane before an entry past the arena is not staged either: its successor is out of range)
    assert {0, 1, 30, 31, 32, 33, 61, 62, 63} <= {t[3] for t in tiles}, sorted({t[3] for t in tiles})
    assert (want == ERR).sum() == 32
    _run(s, arena, bad, want)


def _http_embed(outer_size, key, inner):
    """An HTTP record of outer_size bytes whose pad value holds the record
    `inner` at a 4-byte boundary; returns (record, offset of inner in it)."""
    rec = bytearray(G.http_record(outer_size, key))
    at = (G.http_front_index(rec) + 3 + 2 + 1 + 1 + 3) & ~3  # past method, path, host and the pad's name
    assert at + len(inner) < outer_size - 2
    rec[at:at + len(inner)] = inner
    return bytes(rec), at


def _http_longer(rec):
    """rec with rec_len and its last value's length 4 bytes longer than the record."""
    out = bytearray(rec)
    nh = out[11]
    size, = struct.unpack_from("<I", out)
    struct.pack_into("<I", out, 0, size + 4)
    name_len, value_len = struct.unpack_from("<HH", out, 20 + 4 * (nh - 1))
    struct.pack_into("<HH", out, 20 + 4 * (nh - 1), name_len, value_len + 4)
    return bytes(out)


def _kafka_longer(rec):
    out = bytearray(rec)
    struct.pack_into(">i", out, 0, len(rec))  # msize + 4
    return bytes(out)


@pytest.mark.parametrize("kernel,kind", SIDES, ids=SIDE_IDS)
def test_overlapping_records(gpu, kernel, kind):
    """offs[i + 1] inside record i (a whole valid record embedded in its pad):
    the staged lane must refuse a record longer than the distance to its
    successor and read HBM; a record that claims 4 bytes more than it has is
    valid where arena follows and a parse error as the arena's last."""
    s = _side(kernel, kind)
    sizes = [64, 256, 64, 512, 64, 64, 1024, 64] * 150
    recs = s.records(sizes, 4)
    embedded = {}
    for i in range(1, len(recs), 8):  # the 256-byte records
        inner = s.records([64], 1000 + i)[0]
        if kernel == "http":
            recs[i], at = _http_embed(256, 7 * i, inner)
        else:
            at = 20  # inside the ClientID
            recs[i] = recs[i][:at] + inner + recs[i][at + len(inner):]
        embedded[i] = at
    longer = _http_longer if kernel == "http" else _kafka_longer
    for i in range(4, len(recs), 8):
        recs[i] = longer(recs[i])
    recs[-1] = longer(recs[-1])
    arena, offs = G.build_arena(recs)
    order = []
    for i, o in enumerate(offs.tolist()):
        order.append(o)
        if i in embedded:
            order.append(o + embedded[i])
    order = np.array(order, dtype=np.uint64)
    exp = s.oracle(arena, order)
    pos = {o: j for j, o in enumerate(order.tolist())}
    inner_pos = [pos[int(offs[i]) + at] for i, at in embedded.items()]
    assert (exp[inner_pos] != ERR).all() and len(set(exp[inner_pos].tolist())) >= 3
    assert (exp[[pos[int(offs[i])] for i in embedded]] != ERR).all()
    assert (exp[[pos[int(offs[i])] for i in range(4, len(recs) - 8, 8)]] != ERR).all() and exp[-1] == ERR
    tiles = _tiles(s, arena, order)
    assert sum(1 for t in tiles if t[3] >= 16) >= 4  # the overlapping entries sit inside staged runs
    _run(s, arena, order, exp)


@pytest.mark.parametrize("kernel,kind", SIDES, ids=SIDE_IDS)
def test_batch_sizes_and_wave_shares(gpu, kernel, kind):
    s = _side(kernel, kind)
    arena, offs, exp, _ = _dense(kernel, kind)
    for n, shares in BATCH_SIZES.items():
        tiles = G.plan_tiles(offs[:n], arena.nbytes, s.stage, s.kernel)
        waves = 16 if n <= 2048 else 32
        took = [sum(t[4] for t in tiles if t[0] == w) for w in range(waves)]
        assert set(took) == shares and sum(took) == n, (n, set(took))
        _run(s, arena, offs[:n], exp[:n])


@pytest.mark.parametrize("kernel", ["http", "kafka"])
def test_trailing_slack_and_exact_end(gpu, kernel):
    s = _side(kernel, "default")
    arena, offs, exp, _ = _layout(kernel, "default", 8)
    end = int(offs[-1]) + (int(offs[-1]) - int(offs[-2]))
    assert end == arena.nbytes
    for slack in (0, 4, 12, 64):
        a = np.concatenate([arena, np.full(slack, 0xA5, dtype=np.uint8)])
        last = _tiles(s, a, offs)[-1]
        assert last[2] == last[3] and last[5] < s.stage  # the last run is staged up to arena_bytes
        _run(s, a, offs, exp)


def test_eval_device_same_geometry(gpu):
    """l7m_eval_device on an arena of exactly round_up(arena_bytes, 16) bytes
    (the contract of include/l7match.h): the host path's verdicts and
    counters, nothing written past [0, n) and [0, n_counters)."""
    import torch
    dev = torch.device("cuda:0")
    for kernel, kind in SIDES:
        s = _side(kernel, kind)
        lead = next(x for x in (12, 8, 4) if _layout(kernel, kind, x)[0].nbytes % 16)
        arena, offs, exp, _ = _layout(kernel, kind, lead)
        n, nc = len(offs), s.rs.n_counters
        assert arena.nbytes % 16 != 0
        host = np.full(-(-arena.nbytes // 16) * 16, 0xA5, dtype=np.uint8)
        host[:arena.nbytes] = arena
        da = torch.from_numpy(host).to(dev)
        assert da.data_ptr() % 16 == 0 and da.numel() == host.nbytes
        do = torch.from_numpy(offs.astype(np.int64)).to(dev)
        dv = torch.full((n + 64,), -77, dtype=torch.int32, device=dev)
        dh = torch.full((nc + 64,), 1000, dtype=torch.int64, device=dev)
        s.rs.eval_device(da, arena.nbytes, do, n, dv, dh, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        v, h = dv.cpu().numpy(), dh.cpu().numpy()
        assert (v[n:] == -77).all() and (h[nc:] == 1000).all()
        hh = np.zeros(nc, dtype=np.uint64)
        assert v[:n].tolist() == s.rs.eval(arena, offs, hh).tolist() == exp.tolist()
        assert (h[:nc] - 1000).tolist() == hh.tolist()


# ---- HTTP: the slow pass's LDS record slot ---------------------------------------------------
def test_slow_pass_slot_boundary(gpu):
    """Records of 200..260 bytes that the back-reference rule decides:
    http_slow_kernel copies those <= kSlowRec - 32 bytes into its LDS slot and
    reads the larger ones from HBM."""
    s = _side("http", "slow")
    deny = [k for k in range(200) if G.outcome(k) >= 4]
    allow = [k for k in range(200) if G.outcome(k) < 4]
    recs, hit = [], []
    for j, size in enumerate(range(200, 264, 4)):
        assert (size <= G.SLOW_REC - 32) == (size <= 224)
        for q in range(6):
            key = deny[(6 * j + q) % len(deny)] if q != 2 else allow[j]  # (q 2: a core rule decides first)
            path = G.SLOW_PATH_MISS if q == 4 else G.SLOW_PATH_HIT
            recs.append(G.http_record(size, key, q & 1, path))
            hit.append(q not in (2, 4))
    arena, offs = G.build_arena(recs, lead=4)
    exp = s.oracle(arena, offs)
    hit = np.array(hit)
    assert (exp[hit] == G.SLOW_RULE).all() and (exp[~hit] != G.SLOW_RULE).all()
    assert {int(o) % 16 for o in offs[hit]} == {0, 4, 8, 12}
    _run(s, arena, offs, exp)
    order = offs[::-1]  # the first pass reads them from HBM too
    _run(s, arena, order, exp[::-1])


# ---- Kafka: source identities follow their records --------------------------------------------
def test_kafka_identities_follow_reordering(gpu):
    rules = G.kafka_rules()
    entries = [(rules[:2], False), (rules[2:4], False), (rules[4:], True)]
    idents = {100: [0], 200: [1], 300: [0, 1]}
    rs = L.RuleSet.compile_kafka_map(entries, idents)
    orc = KafkaOracle.from_map(entries, idents)
    s = _side("kafka", "default")
    arena, offs, _, _ = _layout("kafka", "default", 4)
    n = len(offs)
    ids = np.array([(0, 100, 200, 300, 999)[G.outcome(3 * i + 1) % 5] for i in range(n)], dtype=np.uint32)
    rng = np.random.default_rng(6)
    blocks = [np.arange(i, min(i + 64, n)) for i in range(0, n, 64)]
    shuffled = np.concatenate([blocks[i] for i in rng.permutation(len(blocks))])
    for name, perm in (("in order", np.arange(n)), ("reversed", np.arange(n)[::-1]), ("blocks", shuffled)):
        o, d = offs[perm], ids[perm]
        exp = orc.eval(arena, o, threads=8, identities=d)
        assert len(set(exp.tolist())) >= 4
        assert any(t[3] > 1 for t in G.plan_tiles(o, arena.nbytes, s.stage, "kafka")) == (name != "reversed")
        h = np.zeros(rs.n_counters, dtype=np.uint64)
        got = rs.eval(arena, o, h, identities=d)
        assert got.tolist() == exp.tolist()
        assert int(h[0]) == int((exp == -1).sum()) and int(h.sum()) == n
        assert h[2:2 + rs.n_rules].tolist() == np.bincount(exp[exp >= 0], minlength=rs.n_rules).tolist()
    same = orc.eval(arena, offs, threads=8, identities=ids)
    assert (same != orc.eval(arena, offs, threads=8, identities=np.zeros(n, np.uint32))).any()
