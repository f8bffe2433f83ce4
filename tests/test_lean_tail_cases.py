"""CPU-side conditions of the lean kernel's tail and directory cases
(tests/lean_tail_cases.py): every family has its share of allowed and denied
cases under the oracle, every rule set is of the lean class, and the records
have the shapes the GPU test relies on."""
import struct

import numpy as np
import pytest

import lean_tail_cases as C
from cilium_amd import l7match as L


@pytest.fixture(scope="module")
def exp():
    return C.expectations()  # (asserts a quarter allowed and a quarter denied per family)


def test_every_family_allows_and_denies(exp):
    (arena, offs, where), verdicts, last = exp
    assert set(where) == set(C.FAMILY_RULES) and sum(len(ix) for ix in where.values()) == len(offs) <= 4096
    # the bad records of the directory family are parse errors, two per host length
    assert (verdicts["directory"][where["directory"]] == L.VERDICT_PARSE_ERROR).sum() == 8
    # the last record in the "cut" form is rejected, in the "whole" form decided by its last field
    for full, arena_bytes, loffs, v, staged, form in last:
        assert full.nbytes == (arena_bytes + 15) & ~15 and (full[arena_bytes:] == ord("c")).all()
        assert (v[-1] == L.VERDICT_PARSE_ERROR) == (form == "cut")


def test_every_rule_set_is_lean():
    for fam, mk in C.FAMILY_RULES.items():
        assert L.RuleSet.compile_http(mk()).http_lean, fam


def test_the_tail_records_cover_every_alignment():
    """Path, authority and header value of the tail family start at every
    offset of a word, the method at offset 0 (by the record format)."""
    seen = {f: set() for f in C.FIELDS}
    for f in C.FIELDS:
        for shift in range(4):
            r = C.with_field(f, C.BASE[f][:5], shift)
            w2, w3, w4 = struct.unpack_from("<3I", r, 8)
            nhdr, mlen, plen, alen = w2 >> 24, w3 & 0xffff, w3 >> 16, w4 & 0xffff
            pos = 20 + 4 * nhdr
            if f != "method":
                pos += mlen
            if f in ("host", "value"):
                pos += plen
            if f == "value":
                ents = struct.unpack_from("<%dI" % nhdr, r, 20)
                pos += alen + sum((e & 0xffff) + (e >> 16) for e in ents[:-1]) + (ents[-1] & 0xffff)
            assert r[pos:pos + 5] == C.BASE[f][:5]
            seen[f].add(pos & 3)
    assert seen["method"] == {0} and all(seen[f] == {0, 1, 2, 3} for f in ("path", "host", "value"))


def test_the_large_record_puts_the_header_past_65535():
    big = [u[0] for u in C.directory_units() if len(u[0]) > 70000]
    assert len(big) == 4
    for r in big:
        assert r.index(b"x-val") > 65535
