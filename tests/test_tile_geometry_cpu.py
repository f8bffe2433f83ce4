"""The inputs of tests/test_tile_geometry_gpu.py reach the planner branches
they are named after (tile_geometry.plan_tiles, a model of plan() in
l7m_http_impl.h / l7m_kafka.hip), the model's constants are the sources', and
the record generators put the deciding bytes at both ends.  No GPU."""
import os
import re

import numpy as np
import pytest

import tile_geometry as G
from cilium_amd import l7match as L
from oracle import HttpOracle, KafkaOracle
from program_interp import HDR_FIELDS, HttpProgram

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cilium_amd", "csrc")
LEADS = (0, 4, 8, 12)


def _source_constant(fname, pattern):
    with open(os.path.join(CSRC, fname)) as f:
        m = re.search(pattern, f.read(), re.M)
    assert m, f"{fname}: {pattern} not found: the geometry moved, update tests/tile_geometry.py"
    return int(m.group(1))


@pytest.mark.parametrize("fname,pattern,model", [
    ("program.h", r"^#define L7M_HTTP_WAVES (\d+)", G.HTTP_WAVES),
    ("program.h", r"^#define L7M_HTTP_MAX_STAGE (\d+)", G.HTTP_MAX_STAGE),
    ("program.h", r"^#define L7M_HTTP_WG_PER_CU (\d+)", G.WG_PER_CU),
    ("program.h", r"constexpr uint32_t kHttpMinStage = (\d+);", G.HTTP_MIN_STAGE),
    ("program.h", r"constexpr uint32_t kHttpRegDfas = (\d+);", G.HTTP_REG_DFAS),
    ("program.h", r"constexpr uint32_t kMaxLdsCounters = (\d+);", G.MAX_LDS_COUNTERS),
    ("program.h", r"constexpr uint32_t kLdsBytes = (\d+)u \* 1024u;", G.LDS_BYTES // 1024),
    ("program.h", r"constexpr uint32_t kKafkaKinds = (\d+);", G.K_KINDS),
    ("l7m_http_impl.h", r"constexpr uint32_t kMinStagedTake = (\d+);", G.MIN_STAGED_TAKE),
    ("l7m_http_impl.h", r"constexpr uint32_t kSlowRec = (\d+);", G.SLOW_REC),
    ("l7m_kafka.hip", r"constexpr uint32_t kKWaves = (\d+);", G.K_WAVES),
    ("l7m_kafka.hip", r"constexpr uint32_t kKMaxStage = (\d+);", G.K_MAX_STAGE),
    ("l7m_kafka.hip", r"constexpr uint32_t kKLdsBytes = (\d+) \* 1024;", G.LDS_BYTES // 1024),
    ("l7m_kafka.hip", r"constexpr uint32_t kKMaxLdsCounters = (\d+);", G.K_MAX_LDS_COUNTERS),
    ("l7m_kafka.hip", r"constexpr uint32_t kTopicQ = (\d+);", G.K_TOPIC_Q),
    ("l7m_kafka.hip", r"constexpr uint32_t kMaxCliLdsBytes = (\d+);", G.K_MAX_CLI_LDS_BYTES),
])
def test_geometry_constants_match_the_sources(fname, pattern, model):
    got = _source_constant(fname, pattern)
    assert got == model, f"{fname} has {got}, tests/tile_geometry.py has {model}: update the model"


def test_header_word_indices():
    for name, i in G._HTTP_HDR.items():
        assert HDR_FIELDS.index(name) == i


# ---- the planner model on hand-made offsets --------------------------------------
def test_model_on_hand_made_offsets():
    # 64 x 128 B from offset 0: one full tile whose window ends exactly at the stage
    offs = [128 * i for i in range(64)]
    assert G.plan_tiles(offs, 8192, 8192, "http") == [(w, 4 * w, 4, 4, 4, 512, 0) for w in range(16)]
    offs = [128 * i for i in range(2048)]
    t = G.plan_tiles(offs, 128 * 2048, 8192, "http")
    assert len(t) == 32 and all(x[2:] == (64, 64, 64, 8192, 0) for x in t)
    # the same sizes 4 bytes later: the last record leaves the window
    t = G.plan_tiles([o + 4 for o in offs], 128 * 2048 + 4, 8192, "http")
    assert t[0] == (0, 0, 64, 63, 63, 4 + 63 * 128, 4) and t[1][:5] == (0, 63, 64, 63, 63)
    # reversed: a tile stages at most its first record; HTTP still takes all m, Kafka one
    rev = offs[::-1]
    t = G.plan_tiles(rev, 128 * 2048, 8192, "http")
    assert len(t) == 32 and all(x[3] <= 1 and x[4] == 64 for x in t)
    t = G.plan_tiles(rev, 128 * 2048, 6144, "kafka")
    assert len(t) == 2048 and all(x[4] == 1 for x in t)
    # a bad offset at lane 31 cuts the run below kMinStagedTake (HTTP takes 64), at lane 32 not
    for lane, take in ((31, 64), (32, 32)):
        bad = list(offs)
        bad[lane] += 2
        assert G.plan_tiles(bad, 128 * 2048, 8192, "http")[0][3:5] == (lane, take)
    # two workgroups from 2049 records on
    assert {x[0] for x in G.plan_tiles(offs, 128 * 2048, 8192, "http")} == set(range(16))
    assert {x[0] for x in G.plan_tiles(offs + [128 * 2048], 128 * 2049, 8192, "http")} == set(range(32))


# ---- the stages of the GPU tests' rule sets ------------------------------------------
def _http_stages():
    out = {}
    for kind in G.HTTP_KINDS:
        rules, kw, _ = G.http_rules(kind)
        out[kind] = G.http_stage_bytes(L.RuleSet.compile_http(rules, **kw).program())
    return out


def _kafka_stages():
    many = G.kafka_rules() + [L.PortRuleKafka(APIKey="fetch", Topic=f"unused-{i}") for i in range(G.KAFKA_MANY)]
    return {"default": G.kafka_stage_bytes(L.RuleSet.compile_kafka(G.kafka_rules()).program()),
            "many": G.kafka_stage_bytes(L.RuleSet.compile_kafka(many).program())}


def test_stages_of_the_gpu_rule_sets():
    hs = _http_stages()
    assert all(G.HTTP_MIN_STAGE <= s <= G.HTTP_MAX_STAGE and s % 16 == 0 for s in hs.values()), hs
    assert hs["default"] == G.HTTP_MAX_STAGE and hs["columns"] < G.HTTP_MAX_STAGE, hs
    P = HttpProgram(L.RuleSet.compile_http(G.http_rules("columns")[0]).program())
    assert P.h["n_dfas"] > G.HTTP_REG_DFAS and G.http_stage_bytes(P) == hs["columns"]
    assert HttpProgram(L.RuleSet.compile_http(G.http_rules("default")[0]).program()).h["n_dfas"] <= 4
    ks = _kafka_stages()
    assert ks["default"] == G.K_MAX_STAGE and 1024 <= ks["many"] < G.K_MAX_STAGE and ks["many"] % 16 == 0, ks


@pytest.mark.parametrize("kernel", ["http", "kafka"])
def test_layouts_cover_every_tile_class(kernel):
    """Per stage, the union over the four leads of the layouts the GPU tests
    run holds >= 2 tiles of every class; the first tile ends exactly at the
    stage at lead 0 and loses one record at lead 4; the last staged run ends
    at arena_bytes."""
    if kernel == "http":
        stages = {2048, 4096, 6144, 8192} | set(_http_stages().values())
        classes = G.HTTP_CLASSES
    else:
        stages = {2048, 4096, 6144} | set(_kafka_stages().values())
        classes = G.KAFKA_CLASSES
    report = {}
    for stage in sorted(stages):
        sizes = G.segment_sizes(stage, kernel)
        total, first = G.Counter(), {}
        for lead in LEADS:
            offs = np.cumsum([lead] + sizes[:-1])
            nbytes = lead + sum(sizes)
            tiles = G.plan_tiles(offs, nbytes, stage, kernel)
            assert sum(t[4] for t in tiles) == len(sizes)
            total += G.classify(tiles, stage, kernel)
            first[lead] = tiles[0]
            wave, cur, m, k, take, _, _ = tiles[-1]
            assert k == m == take and cur + take == len(sizes), (stage, lead, tiles[-1])
            assert int(offs[-1]) + sizes[-1] == nbytes
        report[stage] = {c: total[c] for c in classes}
        assert first[0][2:] == (64, 64, 64, stage, 0), (stage, first[0])
        assert first[4][2:] == (64, 63, 63, 4 + 63 * sizes[0], 4), (stage, first[4])
    short = {s: {c: v for c, v in r.items() if v < 2} for s, r in report.items()}
    assert not any(short.values()), f"classes with < 2 tiles per stage: {short}; all counts: {report}"


def test_layout_offsets_are_the_segment_sizes():
    """layout() packs segment_sizes() back to back: what the coverage test
    plans is what the GPU tests launch."""
    for kernel, stage in (("http", 2048), ("kafka", 2048)):
        sizes = G.segment_sizes(stage, kernel)
        for lead in (0, 12):
            arena, offs = G.layout(stage, kernel, lead=lead)
            assert offs.tolist() == np.cumsum([lead] + sizes[:-1]).tolist()
            assert arena.nbytes == lead + sum(sizes) and arena.ctypes.data % 16 == 0
    assert G.layout(2048, "http", kind="slow")[1].tolist() == G.layout(2048, "http")[1].tolist()


# ---- generator contracts -----------------------------------------------------------------
def _flip(rec, index):
    out = bytearray(rec)
    out[index] ^= 1
    return bytes(out)


def _contract(records, keys, oracle, front_index):
    """Exact intended verdicts; the last byte and the first deciding byte each change them."""
    for variant, want_equal in (("as built", True), ("last byte", False), ("front byte", False)):
        recs = records
        if variant == "last byte":
            recs = [_flip(r, len(r) - 1) for r in records]
        elif variant == "front byte":
            recs = [_flip(r, front_index(r)) for r in records]
        arena, offs = G.build_arena(recs)
        got = oracle.eval(arena, offs, threads=8)
        exp = np.array([G.intended(k) for k in keys], dtype=np.int32)
        if want_equal:
            assert got.tolist() == exp.tolist()
        else:
            assert (got != exp).all(), (variant, [int(i) for i in np.nonzero(got == exp)[0][:10]])
            assert (got >= L.VERDICT_DENY).all()  # (still well-formed records)


def test_outcomes_are_aperiodic():
    seq = [G.outcome(i) for i in range(4096)]
    assert set(seq) == set(range(6)) and len(set(G.INTENDED)) == 5
    for shift in list(range(1, 130)) + [2048]:
        same = sum(a == b for a, b in zip(seq, seq[shift:]))
        assert same < 0.3 * (len(seq) - shift), shift  # (1/6 expected for independent draws)


@pytest.mark.parametrize("flavour", [0, 1])
def test_http_record_contract(flavour):
    sizes = list(range(G.HTTP_MIN, 1400, 4)) + [2048, 8176, 8192, 8196, 16384, G.HTTP_MAX]
    recs = [G.http_record(s, 11 * s + 1, flavour) for s in sizes]
    assert [len(r) for r in recs] == sizes
    _contract(recs, [11 * s + 1 for s in sizes], HttpOracle(G.http_rules("default")[0]), G.http_front_index)
    lit_len = {len(v) for s in sizes for n, v in G.http_record_fields(s, 3, 1)[3] if n == b"lit"}
    assert len(G.LIT) in lit_len and max(lit_len) > 8 * len(G.LIT)  # equal length: only the last byte differs


def test_http_record_sizes_with_longer_paths():
    for path in (G.SLOW_PATH_HIT, G.SLOW_PATH_MISS):
        for size in range(36, 300, 4):
            assert len(G.http_record(size, size, size & 1, path)) == size


def test_kafka_record_contract():
    sizes = list(range(G.KAFKA_MIN, 1400, 4)) + [2048, 6128, 6144, 6148, 24576, G.KAFKA_MAX - 3]
    recs = [G.kafka_record(s, 13 * s + 2) for s in sizes]
    assert [len(r) for r in recs] == sizes
    _contract(recs, [13 * s + 2 for s in sizes], KafkaOracle(G.kafka_rules()), lambda r: G.KAFKA_FRONT_INDEX)


def test_compiled_program_equals_oracle_on_a_layout():
    """A second reference: program_interp's walk of the compiled program on a
    (2048-byte stage) layout, every third record of it."""
    rules = G.http_rules("default")[0]
    arena, offs = G.layout(2048, "http", seed=1, lead=4)
    offs = offs[::3]
    exp = HttpOracle(rules).eval(arena, offs, threads=8)
    assert set(G.INTENDED) <= set(exp.tolist())
    got = HttpProgram(L.RuleSet.compile_http(rules).program()).eval(arena, offs)
    assert got.tolist() == exp.tolist()
