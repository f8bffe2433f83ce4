"""The HTTP compiler is a function of its input: compiling a rule set twice
gives the same program words (no uninitialised padding, no address-ordered
container in any phase of http_phases.cc).  tools/program_digest.py checks the
same over a large corpus and against another build of the library."""
import numpy as np
import pytest

import policy_cases
import tile_geometry
from cilium_amd import l7match as L


def _words(compile_fn, make):
    return [compile_fn(*make()).program() for _ in range(2)]


@pytest.mark.parametrize("kind", tile_geometry.HTTP_KINDS)
def test_rules_compile_to_the_same_words_twice(kind):
    def make():
        rules, kw, _ = tile_geometry.http_rules(kind)
        return rules, kw

    a, b = _words(lambda rules, kw: L.RuleSet.compile_http(rules, **kw), make)
    assert a.size > 0 and np.array_equal(a, b)


def test_policy_map_compiles_to_the_same_words_twice():
    a, b = _words(L.RuleSet.compile_http_policies, lambda: (policy_cases.random_policies(1),))
    assert a.size > 0 and np.array_equal(a, b)
