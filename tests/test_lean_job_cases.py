"""CPU-side conditions of the lean kernel's job and verification cases
(tests/lean_job_cases.py): the verdict classes every family claims occur under
the oracle, the rule sets are lean, and the programs
have the shapes the GPU test relies on."""
import numpy as np
import pytest

import lean_job_cases as C
from cilium_amd import l7match as L
from program_interp import HttpProgram

KNONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def exp():
    return C.expectations()  # (asserts the classes of lean_job_cases.CLASSES per family)


def test_every_claimed_verdict_class_occurs(exp):
    (arena, offs, where), verdicts = exp
    assert set(verdicts) == set(C.FAMILY_RULES) and sum(len(ix) for ix in where.values()) == len(offs)
    for fam, v in verdicts.items():
        assert (v >= 0).any() and (v == L.VERDICT_DENY).any(), fam
    assert (verdicts["directory"] == L.VERDICT_PARSE_ERROR).sum() >= 1


def test_the_field_counts():
    """32 and 33 fields, both lean: field 32's bit is in the second word of the
    mask of present fields and of the presence-list mask."""
    for n in (32, 33):
        rs = L.RuleSet.compile_http(C.fields_rules(n))
        P = HttpProgram(rs.program())
        assert P.h["n_fields"] == n and rs.http_lean
        assert (P.h["pres_fields_hi"] != 0) == (n == 33)


@pytest.mark.parametrize("fam,field", [("dead_m", 0), ("dead_p", 1), ("dead_a", 2)])
def test_the_dead_automata_are_dead_from_the_start(fam, field):
    P = HttpProgram(L.RuleSet.compile_http(C.FAMILY_RULES[fam]()).program())
    d = [x for x in P.dfas if x["field"] == field]
    assert len(d) == 1 and d[0]["start_base"] == 0


def cand_entries(P, field):
    """(records, matchers of the first record) of every non-empty candidate
    entry of the field's automaton (program.h CandEntry: len, off, rid, header)."""
    d = [x for x in P.dfas if x["field"] == field][0]
    mem, at = (P.img, d["lds_ct"]) if d["lds_ct"] != KNONE else (P.w, d["ct_off"])
    out = []
    for idx in range(1, d["nsets"] + d["npats"] + 1):
        e = mem[at + 16 * idx: at + 16 * idx + 4]
        if e[0]:
            out.append((e[0], e[3] & 0xff))
    return d, out


def test_the_candidate_shapes():
    """The path automaton of the candidate family has entries of one record
    with 1-4 matchers (the keyed one included: checked inline), with 5 and 6
    (more than fit the entry: scanned from the pool) and lists of 2 and 3
    records; its end codes are of both kinds (sets and latched patterns), and
    three automata have candidates, so verification visits more than one."""
    P = HttpProgram(L.RuleSet.compile_http(C.cands_rules()).program())
    assert bin(P.h["cand_dfas_lo"]).count("1") == 3 and P.h["pres_fields_lo"] == 0
    d, ent = cand_entries(P, 1)
    assert d["nsets"] >= 2 and d["npats"] >= 10
    assert {m for n, m in ent if n == 1} >= {1, 2, 3, 4, 5, 6}
    assert {n for n, m in ent} >= {1, 2, 3}
    # presence lists; remote sets and the zero list (the rule with a remote set and no matcher)
    P = HttpProgram(L.RuleSet.compile_http(C.presence_rules()).program())
    assert P.h["pres_fields_lo"] != 0
    P = HttpProgram(L.RuleSet.compile_http(C.remote_rules()).program())
    assert P.h["any_remotes"] == 0 and P.h["zero_len"] == 1
    # two referenced name lengths beside x-val's in the directory family
    P = HttpProgram(L.RuleSet.compile_http(C.directory_rules()).program())
    assert P.h["name_len_lo"] == (1 << 5 | 1 << 6 | 1 << 8)


def test_the_scalars_of_jobs_0_to_2_hold_their_fields():
    """l7m_http_impl.h LeanJob packs lim (17 bits) with t0 (14), and lds_latch
    (17) with nsets (8) and the DFA index (2): the bounds hold for every lean
    program of the cases and for the benchmark's."""
    from cilium_amd import workloads as W
    sets = [mk() for fam, mk in C.FAMILY_RULES.items() if fam not in C.GENERIC] + [W.rules(2)]
    for rules in sets:
        rs = L.RuleSet.compile_http(rules)
        assert rs.http_lean
        P = HttpProgram(rs.program())
        assert P.h["n_dfas"] <= 4
        for d in P.dfas[:P.h["n_dfas"]]:
            assert d["lds_table"] < 1 << 14 and 4 * (d["lds_table"] + d["region"]) < 1 << 17
            assert d["lds_latch"] < 1 << 17 and d["nsets"] < 1 << 8


def test_the_batch_covers_the_cuts(exp):
    (arena, offs, where), _ = exp
    assert len(offs) >= max(C.CUTS)
    sub_arena, sub_offs = C.cut(arena, offs, 55)
    assert len(sub_offs) == 55 and sub_arena.nbytes == int(offs[55])
    assert np.all(np.diff(offs.astype(np.int64)) > 0)
