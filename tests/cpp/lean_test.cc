// lean_test.cc -- stand-alone host test of l7m_dispatch.h http_program_lean
// (tests/test_lean_cpu.py builds it with g++ under ASan/UBSan): one synthetic
// header / descriptor set that passes every clause of the predicate, and one
// per clause that differs from it in that clause alone and must fail.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../cilium_amd/csrc/l7m_dispatch.h"

using namespace l7m;

static int g_fail = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                               \
    }                                                         \
  } while (0)

struct Prog {
  HttpHeader h;
  std::vector<DfaDesc> dd;    // n_dfas value automata (+ the name automaton)
  std::vector<FieldDesc> fd;  // n_fields
  bool lean() const { return http_program_lean(h, dd.data(), fd.data()); }
};

// A config-2-shaped program: method, path, authority with one LDS-walked
// automaton each, one header field with a fourth, names by the LDS table.
static Prog good() {
  Prog p;
  std::memset(&p.h, 0, sizeof p.h);
  p.h.magic = kMagicHttp;
  p.h.n_rules = 10;
  p.h.n_fields = 4;
  p.h.n_dfas = 4;
  p.h.always_rule = kNone;
  p.h.allow_no_l7 = 0;
  p.h.has_name_dfa = 1;
  p.h.lds_name_tab = 4096;
  p.h.name_tab_mask = 7;
  p.h.single_entry = 1;
  p.h.n_policies = 1;
  p.h.lds_ent_tab = kNone;
  p.h.search = 0;
  p.h.lds_dcap = kNone;
  p.h.off_slow = kNone;
  p.h.n_slow = 0;
  p.dd.resize(5);
  for (size_t k = 0; k < p.dd.size(); ++k) {
    DfaDesc& d = p.dd[k];
    std::memset(&d, 0xff, sizeof d);  // every offset kNone
    d.kind = kDfaPacked;
    d.lds_table = 256 + 1024 * static_cast<uint32_t>(k);
    d.lds_es = kLdsEsInEntry;
    d.lds_latch = 100;
    d.start_base = 1;
    d.region = 300;
    d.nsets = 3;
    d.field = static_cast<uint32_t>(k);
  }
  // the name automaton (dd[n_dfas]) is outside the predicate: give it every disqualifying value
  p.dd[4].lds_table = kNone;
  p.dd[4].lds_es = kNone;
  p.dd[4].lit_tab = 7;
  p.dd[4].lds_skip = 9;
  p.fd.resize(4);
  for (size_t f = 0; f < p.fd.size(); ++f) {
    std::memset(&p.fd[f], 0, sizeof p.fd[f]);
    p.fd[f].dfa_first = static_cast<uint32_t>(f);
    p.fd[f].ndfa = 1;
    p.fd[f].gram_tab = p.fd[f].alit_tab = kNone;
  }
  return p;
}

static void fails(const char* what, const std::function<void(Prog&)>& edit) {
  Prog p = good();
  edit(p);
  if (p.lean()) {
    std::printf("FAIL clause \"%s\" does not make the predicate false\n", what);
    ++g_fail;
  }
}

int main() {
  CHECK(good().lean());
  {  // also lean: no referenced header at all (no name automaton, no name table), fewer automata
    Prog p = good();
    p.h.has_name_dfa = 0;
    p.h.lds_name_tab = kNone;
    p.h.n_fields = 3;
    p.h.n_dfas = 3;
    CHECK(p.lean());
  }
  fails("single_entry", [](Prog& p) { p.h.single_entry = 0; });
  fails("allow_no_l7", [](Prog& p) { p.h.allow_no_l7 = 1; });
  fails("search", [](Prog& p) { p.h.search = 1; });
  fails("forced capture", [](Prog& p) { p.h.lds_dcap = 512; });
  fails("slow-path rules", [](Prog& p) { p.h.n_slow = 1; });
  fails("n_dfas <= 4", [](Prog& p) {
    p.h.n_dfas = 5;
    p.dd.insert(p.dd.begin() + 4, p.dd[3]);  // a fifth lean-shaped value automaton
  });
  for (uint32_t k = 0; k < 4; ++k) {
    fails("literal table", [k](Prog& p) { p.dd[k].lit_tab = 64; });
    fails("dense automaton", [k](Prog& p) { p.dd[k].kind = kDfaDense; });
    fails("search automaton", [k](Prog& p) { p.dd[k].kind = kDfaSearch; });
    fails("table not in LDS", [k](Prog& p) { p.dd[k].lds_table = kNone; });
    fails("end codes in a table", [k](Prog& p) { p.dd[k].lds_es = 2 * 300; });
    fails("end codes in the program", [k](Prog& p) { p.dd[k].lds_es = kNone; });
    fails("skip descriptors", [k](Prog& p) { p.dd[k].lds_skip = 128; });
  }
  fails("names by the name automaton", [](Prog& p) { p.h.lds_name_tab = kNone; });
  fails("name-length masks without a name table", [](Prog& p) {
    p.h.has_name_dfa = 0;
    p.h.lds_name_tab = kNone;
    p.h.name_len_lo = 1u << 7;
  });
  fails("name-length masks (high word) without a name table", [](Prog& p) {
    p.h.has_name_dfa = 0;
    p.h.lds_name_tab = kNone;
    p.h.name_len_hi = 1u;
  });
  for (uint32_t f = 0; f < 3; ++f) {
    fails("pseudo-header field without an automaton", [f](Prog& p) { p.fd[f].ndfa = 0; });
    fails("pseudo-header field with two automata", [f](Prog& p) { p.fd[f].ndfa = 2; });
    fails("pseudo-header automaton out of range", [f](Prog& p) { p.fd[f].dfa_first = 4; });
  }
  fails("fewer than three fields", [](Prog& p) { p.h.n_fields = 2; });

  std::printf("failures=%d\n", g_fail);
  return g_fail ? 1 : 0;
}
