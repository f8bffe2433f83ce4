"""GPU cases for the kernel instantiations the launchers select by
l7m_dispatch.h dispatch_values (launch_http, l7m_http_feat.hip, launch_kafka,
launch_kafka_resident) that the other GPU test files leave out, and Kafka's
in full: a small rule set that selects the cell, 130 records (two tiles and a partial
one), verdicts and every hit counter bit-exact against the oracle."""
import numpy as np
import pytest

import kafka_wire as K
import tile_geometry as G
from cilium_amd import l7match as L
from oracle import HttpOracle, KafkaOracle

pytestmark = pytest.mark.gpu
RE2 = L.DIALECT_RE2_SEARCH


# ---- HTTP ------------------------------------------------------------------
@pytest.mark.parametrize("n_fields", [1, 4, 8])
@pytest.mark.parametrize("counters", ["none", "global"])
def test_http_hit_modes_by_end_code_storage(gpu, n_fields, counters):
    """launch_http's first-pass instantiations without hit counters and with
    wave-aggregated global ones (kMaxLdsCounters - 1 further rules: counters =
    rules + 2 no longer fit the LDS array), each with end codes in 4 registers,
    8 registers and LDS columns; the LDS-counter instantiations run in
    tests/test_http_gpu.py test_end_code_storage_and_header_jobs.  130 records (two tiles and a
    partial one): verdicts and every counter equal the oracle's."""
    rng = np.random.default_rng(7100 + n_fields)
    names = [f"x-h{j}" for j in range(n_fields)]
    rules = [L.PortRuleHTTP(Path=f"/p{i % 7}/.*", Method=["GET", "POST", ""][i % 3],
                            Headers=[f"{names[i % n_fields]}: v{i % 4}"]) for i in range(24)]
    if counters == "global":
        rules += [L.PortRuleHTTP(Method="NEVER")] * (G.MAX_LDS_COUNTERS - 1)
    reqs = [L.HTTPRequest(["GET", "POST", "PUT"][int(rng.integers(0, 3))],
                          f"/p{int(rng.integers(0, 9))}/{int(rng.integers(0, 100))}", "h",
                          [(names[int(rng.integers(0, n_fields))], f"v{int(rng.integers(0, 5))}")
                           for _ in range(int(rng.integers(0, 4)))]) for _ in range(130)]
    arena, offs = L.pack_http(reqs)
    rs = L.RuleSet.compile_http(rules)
    assert (rs.info.n_dfas <= 4) == (n_fields == 1) and (rs.info.n_dfas > G.HTTP_REG_DFAS) == (n_fields == 8)
    assert (rs.n_rules + 2 > G.MAX_LDS_COUNTERS) == (counters == "global")
    h = None if counters == "none" else np.zeros(rs.n_counters, dtype=np.uint64)
    got = rs.eval(arena, offs, h)
    exp = HttpOracle(rules).eval(arena, offs, threads=8)
    assert got.tolist() == exp.tolist()
    assert (exp >= 0).any() and (exp == -1).any()
    if h is not None:
        assert int(h[0]) == int((exp == -1).sum()) and int(h[1]) == int((exp <= -2).sum())
        assert h[2:2 + rs.n_rules].tolist() == np.bincount(exp[exp >= 0], minlength=rs.n_rules).tolist()
        assert int(h.sum()) == len(exp)


def test_http_search_global_hit_counters(gpu):
    """The search instantiation with wave-aggregated global counters (more
    than kMaxLdsCounters - 2 rules; without counters: tests/test_re2_gpu.py, LDS
    counters: tests/test_tile_geometry_gpu.py).  130 records (two tiles and a
    partial one): verdicts and every counter equal the oracle's."""
    rng = np.random.default_rng(41)
    rules = [L.PortRuleHTTP(Path="bcb", Method="^FET$"), L.PortRuleHTTP(Path="^/p", Method="GET", Headers=["k: a"]),
             L.PortRuleHTTP(Host="\\.local$")] + [L.PortRuleHTTP(Method="^NEVER$")] * (G.MAX_LDS_COUNTERS - 1)
    reqs = [L.HTTPRequest(str(rng.choice(["GET", "FET", "PUT"])), str(rng.choice(["/p", "/abcbz", "/q/bcb", "/x"])),
                          str(rng.choice(["a.local", "example.com"])), [("k", "a")] if rng.random() < 0.5 else [])
            for _ in range(130)]
    arena, offs = L.pack_http(reqs)
    rs = L.RuleSet.compile_http(rules, dialect=RE2)
    assert rs.n_rules + 2 > G.MAX_LDS_COUNTERS
    h = np.zeros(rs.n_counters, dtype=np.uint64)
    got = rs.eval(arena, offs, h)
    exp = HttpOracle(rules, dialect=RE2).eval(arena, offs, threads=8)
    assert got.tolist() == exp.tolist()
    assert {0, 1, 2, -1} <= set(exp.tolist())
    assert int(h[0]) == int((exp == -1).sum()) and int(h[1]) == int((exp <= -2).sum())
    assert h[2:2 + rs.n_rules].tolist() == np.bincount(exp[exp >= 0], minlength=rs.n_rules).tolist()
    assert int(h.sum()) == len(exp)


# ---- Kafka -----------------------------------------------------------------
_CELL_TOPICS = ["t%d" % i for i in range(6)]
_CELL_CLIENTS = ["c%d" % i for i in range(3)]


def _cell_program(rng, clients, groups, n_unused=0):
    """(rule set, oracle, per-request identities) that select one instantiation:
    a client table in LDS or no ClientID rule x one L7DataMap entry for every
    source or identity groups; n_unused further rules only add counters.
    130 records: two tiles and a partial one."""
    rules = [L.PortRuleKafka(APIKey=["produce", "fetch", "metadata"][i % 3], Topic=_CELL_TOPICS[i % 6],
                             ClientID=_CELL_CLIENTS[i % 3] if clients and i % 2 else "") for i in range(12)]
    rules += [L.PortRuleKafka(APIKey="fetch", Topic="unused-%d" % i) for i in range(n_unused)]
    if not groups:
        return L.RuleSet.compile_kafka(rules), KafkaOracle(rules), None
    entries, ids = [(rules[0::3], False), (rules[1::3], False), (rules[2::3], True)], {100: [0], 200: [1], 300: [0, 1]}
    idv = np.array([100, 200, 300, 0, 999], np.uint32)[rng.integers(0, 5, 130)]
    return L.RuleSet.compile_kafka_map(entries, ids), KafkaOracle.from_map(entries, ids), idv


def _cell_records(rng):
    return K.random_requests(rng, 130, _CELL_TOPICS + ["zz"], _CELL_CLIENTS + ["cX"])


@pytest.mark.parametrize("groups", [False, True], ids=["all-rules", "groups"])
@pytest.mark.parametrize("clients", [False, True], ids=["no-clients", "clients-lds"])
@pytest.mark.parametrize("counters", ["none", "lds", "global"])
def test_kafka_first_pass_instantiations(gpu, counters, clients, groups):
    """launch_kafka's kafka_eval_kernel instantiations, one per case: hit
    counters none / in LDS / global (more than kKMaxLdsCounters - 2 rules) x
    _cell_program's client table x identity groups: verdicts and every
    counter equal the oracle's."""
    rng = np.random.default_rng(17)
    rs, orc, idv = _cell_program(rng, clients, groups, G.K_MAX_LDS_COUNTERS - 1 if counters == "global" else 0)
    arena, offs = L.pack_records(_cell_records(rng))
    w = rs.program()  # KafkaHeader: [1] n_rules, [10] n_clients, [14] n_id_slots
    assert (int(w[1]) + 2 > G.K_MAX_LDS_COUNTERS) == (counters == "global")
    assert (int(w[10]) != 0) == clients and int(w[10]) * G.K_CLIENT_SLOT_WORDS * 4 <= G.K_MAX_CLI_LDS_BYTES
    assert (int(w[14]) != 0) == groups
    h = None if counters == "none" else np.zeros(rs.n_counters, dtype=np.uint64)
    got = rs.eval(arena, offs, h, identities=idv)
    exp = orc.eval(arena, offs, threads=8, identities=idv)
    assert got.tolist() == exp.tolist()
    assert (exp >= 0).any() and (exp == -1).any()
    if h is not None:
        assert int(h[0]) == int((exp == -1).sum()) and int(h[1]) == int((exp <= -2).sum())
        assert h[2:2 + rs.n_rules].tolist() == np.bincount(exp[exp >= 0], minlength=rs.n_rules).tolist()
        assert int(h.sum()) == len(exp)


@pytest.mark.parametrize("groups", [False, True], ids=["all-rules", "groups"])
@pytest.mark.parametrize("clients", [False, True], ids=["no-clients", "clients-lds"])
def test_kafka_resident_instantiations(gpu, clients, groups):
    """launch_kafka_resident's four kafka_resident_kernel instantiations (kind
    & 3: client table in LDS, identity groups): one caller sends
    _cell_records one at a time through a batcher; every verdict equals the
    oracle's and the resident workgroup decided batches."""
    rng = np.random.default_rng(23)
    rs, orc, idv = _cell_program(rng, clients, groups)
    recs = _cell_records(rng)
    arena, offs = L.pack_records(recs)
    exp = orc.eval(arena, offs, identities=idv)
    assert (exp >= 0).any() and (exp == -1).any()
    b = L.Batcher(rs, max_delay_us=50, eager=True)
    try:
        got = [b.eval(r) if idv is None else b.eval(r, int(idv[i])) for i, r in enumerate(recs)]
        assert got == exp.tolist()
        assert b.profile()["resident_batches"] > 0
    finally:
        b.close()
