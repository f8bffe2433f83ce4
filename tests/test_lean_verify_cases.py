"""CPU checks of tests/lean_verify_cases.py and of what the compiler writes for
the lean HTTP kernel's verification: every CandEntry::pad bit equals the
membership of the matcher's pattern in that set, the header flag
kHttpInlineMasks follows the set counts, and every lean program has at most one
header field with an automaton (it follows from l7m_dispatch.h
http_program_lean's four value automata, three of them owned by method, path
and authority; asserted here over the case modules' programs and config 2)."""
import numpy as np
import pytest

import lean_job_cases as J
import lean_tail_cases as T
import lean_verify_cases as C
from cilium_amd import l7match as L
from cilium_amd import workloads as W
from program_interp import HttpProgram

KNONE = 0xFFFFFFFF
INLINE_MASKS = 2  # program.h kHttpInlineMasks (HttpHeader::single_entry bit 1)


@pytest.fixture(scope="module")
def programs():
    return {fam: HttpProgram(L.RuleSet.compile_http(mk()).program()) for fam, mk in C.FAMILY_RULES.items()}


def set_members(P, d, s):
    """Local pattern ids of set s of automaton d, from the program's set lists."""
    so = P.h["off_sets"] + 2 * (P.dfas[d]["set_base"] + s)
    po, pl = P.w[so], P.w[so + 1]
    return set(P.w[P.h["off_pool"] + po: P.h["off_pool"] + po + pl])


def entries(P):
    """(automaton, index, the entry's 16 words) of every candidate entry, the program's copy."""
    for k in range(P.h["n_dfas"]):
        d = P.dfas[k]
        for idx in range(d["nsets"] + d["npats"]):
            e = list(P.w[d["ct_off"] + 16 * idx: d["ct_off"] + 16 * idx + 16])
            if d["lds_ct"] != KNONE:
                assert e == list(P.img[d["lds_ct"] + 16 * idx: d["lds_ct"] + 16 * idx + 16]), (k, idx)
            yield k, idx, e


def check_pads(P):
    """Asserts every pad word; returns (inline code matchers seen, whether their automata all have <= 32 sets)."""
    seen, exact = 0, True
    for k, idx, e in entries(P):
        nm = e[3] & 0xFF if e[0] else 0
        for q in range(4):
            pad = e[12 + q]
            if not e[0] or nm > 4 or q >= nm or (e[4 + 2 * q] >> 8) & 1:
                assert pad == 0, (k, idx, q)  # no record, a scanned record, no matcher, a presence matcher
                continue
            d, pat = e[4 + 2 * q] >> 9, e[5 + 2 * q]
            ns = P.dfas[d]["nsets"]
            want = sum(1 << s for s in range(min(ns, 32)) if pat in set_members(P, d, s))
            assert pad == want, (k, idx, q, hex(pad), hex(want))
            assert not pad & 1  # set 0 is the empty set: code 0 never passes
            seen += 1
            exact &= ns <= 32
    return seen, exact


def test_conditions_hold():
    (arena, offs, where), exp = C.expectations()
    assert set(exp) == set(C.FAMILY_RULES) and len(offs) >= 16 * 65
    a, o = C.error_batch(130)
    assert len(o) == 130


@pytest.mark.parametrize("fam", list(C.FAMILY_RULES))
def test_pad_bits_are_set_membership(programs, fam):
    P = programs[fam]
    seen, exact = check_pads(P)
    assert seen > 0 or fam in ("nohdr", "vlen", "among"), fam
    assert bool(P.h["single_entry"] & INLINE_MASKS) == exact == C.INLINE_MASKS[fam], fam
    assert P.h["single_entry"] & 1


def test_config2_pads_and_flag():
    P = HttpProgram(L.RuleSet.compile_http(W.rules(2)).program())
    seen, exact = check_pads(P)
    assert seen > 0 and exact and P.h["single_entry"] & INLINE_MASKS


@pytest.mark.parametrize("fam", list(C.METHOD_SETS))
def test_method_automaton_has_the_sets_it_claims(programs, fam):
    P = programs[fam]
    method = P.dfas[P.fields[0][0]]
    assert method["nsets"] == C.METHOD_SETS[fam]
    # ... and an inline code matcher targets it
    assert any(e[0] and (e[3] & 0xFF) <= 4 and not (e[4] >> 8) & 1 and e[4] >> 9 == P.fields[0][0]
               for _, _, e in entries(P))


def test_inline_family_has_every_entry_shape(programs):
    P = programs["inline"]
    shapes = {(e[0], e[3] & 0xFF) for _, _, e in entries(P) if e[0]}
    for nm in (1, 2, 3, 4, 5):
        assert (1, nm) in shapes, shapes
    assert any(n == 2 for n, _ in shapes)


def test_value_automata_counts(programs):
    for fam, n in C.N_DFAS.items():
        assert programs[fam].h["n_dfas"] == n, fam


def lean_programs():
    for mod in (J, T, C):
        for fam, mk in mod.FAMILY_RULES.items():
            rs = L.RuleSet.compile_http(mk())
            if rs.http_lean:
                yield f"{mod.__name__}.{fam}", HttpProgram(rs.program())
    rs = L.RuleSet.compile_http(W.rules(2))
    assert rs.http_lean
    yield "config2", HttpProgram(rs.program())


def test_lean_programs_have_one_header_automaton_at_the_most():
    n = 0
    for name, P in lean_programs():
        nd = [f[1] for f in P.fields[3:]]
        assert all(x <= 1 for x in nd) and sum(nd) <= 1, (name, nd)
        assert all(f[1] == 0 or f[0] < P.h["n_dfas"] for f in P.fields[3:]), name
        n += 1
    assert n >= 15
