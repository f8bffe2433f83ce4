// http_phases.cc — translated HTTP rules -> the device program, in phases.
//
// compile_http_core (at the end) is the driver; each phase is one function
// that reads the structs of the phases before it by const& and fills its own:
//   1. match_rules          rules -> Matchers (fields, distinct patterns, rule matchers)
//   2. build_field_automata per field: parse, groups, filters -> FieldAutomata, dcaps
//   3. number_automata      header-name automaton, global numbering -> Numbering
//   4. key_rules            most selective matcher per rule -> RuleKeys
//   5. build_records        descriptors, sets, check records -> Tables
//   6. place_*              the LDS image, in budget order -> Image (and the lds_* of Tables)
//   7. convert_dense        packed -> dense automata walked from the program
//   8. lay_out              word offsets of everything -> Layout
//   9. emit_*               the copies into the program and its image
// The order of the placements in 6-8 is part of the output: every take moves
// the cursor that the later budget tests read.  DESIGN.md "Compiler (cold
// path)" has the table of what each phase reads and writes.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <regex>
#include <unordered_map>

#include "dfa_pack.h"
#include "http_phases.h"
#include "l7m_internal.h"
#include "program.h"
#include "regex_ecma.h"
#include "regex_vm.h"

namespace l7m {
namespace {

// A phase's outcome: L7M_OK, or the status and message the compile fails with.
struct Err {
  int status = L7M_OK;
  std::string msg;
  bool ok() const { return status == L7M_OK; }
};
Err fail(int st, const std::string& m) { return {st, m}; }

constexpr uint64_t round_up(uint64_t x, uint64_t granule) { return (x + granule - 1) & ~(granule - 1); }
constexpr uint64_t round4(uint64_t x) { return round_up(x, 4); }

// Word allocator of the LDS image (16-byte granules) and of the program.
struct WordAlloc {
  uint64_t at = 0;  // cursor, words
  uint32_t take(uint64_t words, uint64_t granule = 1) {
    const uint64_t o = at;
    at += round_up(words, granule);
    return static_cast<uint32_t>(o);
  }
  void align(uint64_t granule) { at = round_up(at, granule); }
};

// States of one look-ahead pattern's exact automaton before it is carried as
// a superset (the look-ahead dropped) and decided by the slow path.
constexpr size_t kLookMaxStates = 1u << 16;

struct FieldPattern {
  MatchKind kind;
  std::string value;
  bool operator<(const FieldPattern& o) const {
    if (kind != o.kind) return kind < o.kind;
    return value < o.value;
  }
};

// Search automaton of <= kSearchMaxPats RE2-dialect patterns (program.h
// kDfaSearch): the dense DFA of [\x00-\xff]*(p0|...|pk) with, per state, the
// patterns matching a substring that ends there (mid set, '$' unsatisfied)
// and at the end of the input (end set).
struct SearchDfa {
  uint32_t nstates = 0, ncls = 0, start = 0, start_mid = 0;
  uint8_t cmap[256] = {0};
  std::vector<uint32_t> table;    // nstates * ncls: next state | mid id << 24
  std::vector<uint32_t> endmask;  // per state
  std::vector<uint32_t> midmask;  // per mid id (0: no pattern)
};

re::Status build_search_dfa(const std::vector<const re::Ast*>& pats, SearchDfa* out) {
  if (pats.size() > kSearchMaxPats) return re::Status::TooBig;
  std::vector<re::Ast> a(pats.size());
  std::vector<const re::Ast*> ptrs;
  for (size_t i = 0; i < pats.size(); ++i) {
    a[i] = *pats[i];
    re::simplify_search(&a[i]);
    re::make_search_prefix(&a[i]);
    ptrs.push_back(&a[i]);
  }
  re::Dfa d;
  re::DfaLimits lim;
  lim.max_states = 1u << 17;
  lim.max_table_bytes = 32ull << 20;
  const re::Status st = re::build_dfa(ptrs, lim, &d, /*with_mid=*/true);
  if (st != re::Status::Ok) return st;
  if (static_cast<uint64_t>(d.nstates) * d.ncls >= (1u << 24)) return re::Status::TooBig;
  std::vector<uint32_t> set_mask(d.sets.size(), 0);
  for (size_t k = 0; k < d.sets.size(); ++k)
    for (uint32_t p : d.sets[k]) set_mask[k] |= 1u << p;
  // mid ids: distinct mid sets, 0 = the empty set
  std::vector<uint32_t> mid_id(d.sets.size(), kNone);
  out->midmask.assign(1, 0u);
  mid_id[0] = 0;
  for (int q = 0; q < d.nstates; ++q) {
    const uint32_t sid = d.midset[q];
    if (mid_id[sid] != kNone) continue;
    if (out->midmask.size() >= kSearchMaxMid) return re::Status::TooBig;
    mid_id[sid] = static_cast<uint32_t>(out->midmask.size());
    out->midmask.push_back(set_mask[sid]);
  }
  out->nstates = static_cast<uint32_t>(d.nstates);
  out->ncls = static_cast<uint32_t>(d.ncls);
  out->start = static_cast<uint32_t>(d.start);
  out->start_mid = set_mask[d.midset[d.start]];
  std::memcpy(out->cmap, d.cmap, 256);
  out->table.resize(static_cast<size_t>(d.nstates) * d.ncls);
  for (size_t i = 0; i < out->table.size(); ++i) {
    const uint32_t nx = d.next[i];
    out->table[i] = nx | mid_id[d.midset[nx]] << 24;
  }
  out->endmask.resize(d.nstates);
  for (int q = 0; q < d.nstates; ++q) out->endmask[q] = set_mask[d.endset[q]];
  return re::Status::Ok;
}

struct Group {
  std::vector<uint32_t> pats;  // field pattern indices (local id = position)
  PackedDfa pk;                // kDfaPacked groups
  bool search = false;         // kDfaSearch group (sd)
  SearchDfa sd;
  bool alit = false;           // kDfaAlit group (no automaton: the field's alit scan)
};

// Literal-anchored RE2 patterns of one field (program.h FieldDesc::alit_*).
struct AlitField {
  bool on = false;
  uint32_t first_group = 0;            // field group index of the first kDfaAlit group
  std::vector<uint32_t> tab;           // buckets x {gram, pattern + 1, gram, pattern + 1}
  std::vector<uint32_t> pats;          // field pattern ids in alit order (AlitRec order)
  std::vector<std::string> lit;        // per alit pattern: L
  std::vector<uint32_t> k;             // per alit pattern: offset of its table gram in L
  std::vector<uint32_t> resid;         // per alit pattern: residual id, kNone = empty
  PackedDfa resid_pk;                  // automaton of the distinct residuals
  uint32_t n_resid = 0;
};

// Choose the alit patterns of a field: every RE2 pattern L R whose L's
// grams fit the table (rarest gram first); the rest stay search patterns.
void plan_alit(const std::vector<re::Ast>& asts, const std::vector<uint32_t>& sidx, AlitField* out,
               std::vector<uint32_t>* rest) {
  std::vector<uint32_t> cand;
  std::vector<std::string> lits;
  std::vector<re::Ast> res;
  for (uint32_t p : sidx) {
    re::Ast sa = asts[p];
    re::simplify_search(&sa);
    std::string L;
    re::Ast R;
    if (re::split_literal_prefix(sa, &L, &R)) {
      cand.push_back(p);
      lits.push_back(std::move(L));
      res.push_back(std::move(R));
    } else {
      rest->push_back(p);
    }
  }
  if (cand.size() < kAlitMinPatterns) {
    rest->insert(rest->end(), cand.begin(), cand.end());
    std::sort(rest->begin(), rest->end());
    return;
  }
  std::map<uint32_t, uint32_t> freq;
  for (const auto& L : lits)
    for (size_t i = 0; i + 4 <= L.size(); ++i) {
      uint32_t g;
      std::memcpy(&g, L.data() + i, 4);
      ++freq[g];
    }
  uint32_t buckets = 64;
  while (buckets < 2 * cand.size()) buckets <<= 1;  // quarter-full: every pattern finds a bucket
  if (16ull * buckets > kAlitMaxLdsBytes) buckets = kAlitMaxLdsBytes / 16;
  out->tab.assign(4ull * buckets, 0u);
  std::map<std::string, uint32_t> rid;
  std::vector<re::Ast> rasts;
  for (size_t c = 0; c < cand.size(); ++c) {
    const std::string& L = lits[c];
    int best_i = -1, best_e = -1;
    uint32_t best_f = kNone, best_g = 0;
    for (size_t i = 0; i + 4 <= L.size(); ++i) {
      uint32_t g;
      std::memcpy(&g, L.data() + i, 4);
      const uint32_t* b = &out->tab[4ull * (gram_bucket(g) & (buckets - 1))];
      const int e = !b[1] ? 0 : !b[3] ? 1 : -1;
      if (e < 0) continue;
      if (freq[g] < best_f) {
        best_f = freq[g];
        best_i = static_cast<int>(i);
        best_e = e;
        best_g = g;
      }
    }
    if (best_i < 0) {  // every bucket of its grams is full: a search pattern
      rest->push_back(cand[c]);
      continue;
    }
    const uint32_t id = static_cast<uint32_t>(out->pats.size());
    uint32_t* b = &out->tab[4ull * (gram_bucket(best_g) & (buckets - 1))];
    b[2 * best_e] = best_g;
    b[2 * best_e + 1] = id + 1;
    out->pats.push_back(cand[c]);
    out->lit.push_back(L);
    out->k.push_back(static_cast<uint32_t>(best_i));
    if (re::residual_is_empty(res[c])) {
      out->resid.push_back(kNone);
    } else {
      auto it = rid.emplace(re::ast_key(res[c]), static_cast<uint32_t>(rasts.size()));
      if (it.second) rasts.push_back(std::move(res[c]));
      out->resid.push_back(it.first->second);
    }
  }
  std::sort(rest->begin(), rest->end());
  if (out->pats.size() < kAlitMinPatterns) {
    rest->insert(rest->end(), out->pats.begin(), out->pats.end());
    std::sort(rest->begin(), rest->end());
    *out = AlitField();
    return;
  }
  out->n_resid = static_cast<uint32_t>(rasts.size());
  if (!rasts.empty()) {
    std::vector<const re::Ast*> rp;
    for (const auto& a : rasts) rp.push_back(&a);
    if (build_field_dfa(rp, FieldDfaLimits(), &out->resid_pk) != re::Status::Ok || out->resid_pk.n_slots > 12000) {
      rest->insert(rest->end(), out->pats.begin(), out->pats.end());  // residual automaton too large: search groups
      std::sort(rest->begin(), rest->end());
      *out = AlitField();
      return;
    }
  }
  out->on = true;
}

// Search groups of one field's RE2-dialect patterns: chunks of
// kSearchMaxPats, halved while an automaton exceeds the limits.
int build_search_groups(const std::vector<const re::Ast*>& asts, std::vector<uint32_t> idx,
                        std::vector<Group>* out, std::string* err) {
  if (idx.size() > kSearchMaxPats) {
    for (size_t o = 0; o < idx.size(); o += kSearchMaxPats) {
      std::vector<uint32_t> part(idx.begin() + o, idx.begin() + std::min(idx.size(), o + kSearchMaxPats));
      const int rc = build_search_groups(asts, std::move(part), out, err);
      if (rc != L7M_OK) return rc;
    }
    return L7M_OK;
  }
  std::vector<const re::Ast*> sub;
  for (uint32_t i : idx) sub.push_back(asts[i]);
  Group g;
  g.search = true;
  const re::Status st = build_search_dfa(sub, &g.sd);
  if (st == re::Status::Ok) {
    g.pats = std::move(idx);
    out->push_back(std::move(g));
    return L7M_OK;
  }
  if (st != re::Status::TooBig) {
    *err = "search DFA construction failed";
    return L7M_EUNSUPPORTED;
  }
  if (idx.size() == 1) {
    *err = "a single search pattern exceeds the DFA state limit";
    return L7M_ETOOBIG;
  }
  const size_t h = idx.size() / 2;
  std::vector<uint32_t> a(idx.begin(), idx.begin() + h), b(idx.begin() + h, idx.end());
  const int rc = build_search_groups(asts, std::move(a), out, err);
  if (rc != L7M_OK) return rc;
  return build_search_groups(asts, std::move(b), out, err);
}

// RE2-dialect gram filter of one field (program.h FieldDesc::gram_tab): a
// 2-entry-bucket table 4-byte gram -> mask of search groups (bit j % 32 of
// the field's search group j).  Each pattern with a required literal is
// entered under ONE of its literal's grams -- the rarest among the field's
// patterns whose bucket has room --, so a value that contains none of a
// group's chosen grams cannot match any of the group's patterns and the
// group's automaton is not walked.
struct GramFilter {
  bool on = false;
  uint32_t search_first = 0;  // field group index of the first search group
  uint32_t always = 0;        // groups walked for every value
  uint32_t n_search = 0;      // search groups of the field
  std::vector<uint32_t> tab;  // buckets x {gram, mask, gram, mask}
};

void build_gram_filter(const std::vector<Group>& groups, uint32_t first, uint32_t first_lit,
                       const std::vector<std::vector<uint32_t>>& grams, GramFilter* out) {
  const uint32_t ns = static_cast<uint32_t>(groups.size()) - first;
  out->search_first = first;
  if (ns < kGramMinGroups || ns > kGramMaxGroups || first_lit == groups.size()) return;
  std::map<uint32_t, uint32_t> freq;
  uint32_t n_lit = 0;
  for (uint32_t j = first_lit; j < groups.size(); ++j)
    for (uint32_t p : groups[j].pats) {
      for (uint32_t g : grams[p]) ++freq[g];
      ++n_lit;
    }
  uint32_t buckets = 64;
  while (buckets < n_lit) buckets <<= 1;
  if (buckets > 65536) return;
  out->tab.assign(4ull * buckets, 0u);
  for (uint32_t j = first; j < first_lit; ++j) out->always |= 1u << ((j - first) & 31u);
  for (uint32_t j = first_lit; j < groups.size(); ++j) {
    const uint32_t bit = 1u << ((j - first) & 31u);
    for (uint32_t p : groups[j].pats) {
      uint32_t best = kNone, best_freq = kNone;
      int best_slot = -1;
      for (uint32_t g : grams[p]) {
        uint32_t* b = &out->tab[4ull * (gram_bucket(g) & (buckets - 1))];
        int slot = -1;
        for (int e = 0; e < 2 && slot < 0; ++e)
          if (b[2 * e + 1] && b[2 * e] == g) slot = e;  // already entered: shares the entry
        for (int e = 0; e < 2 && slot < 0; ++e)
          if (!b[2 * e + 1]) slot = e;
        if (slot < 0) continue;
        const uint32_t fq = freq[g];
        if (fq < best_freq) {
          best = g;
          best_freq = fq;
          best_slot = slot;
        }
      }
      if (best_slot < 0) {  // every bucket of its grams is full: walk the group always
        out->always |= bit;
        continue;
      }
      uint32_t* b = &out->tab[4ull * (gram_bucket(best) & (buckets - 1))];
      b[2 * best_slot] = best;
      b[2 * best_slot + 1] |= bit;
    }
  }
  out->on = true;
}

// Build the field automata of one field's patterns: normally ONE automaton
// (dfa_pack.h, linear in the rules for prefix-diverging sets); a set whose
// product exceeds the limits (e.g. unanchored RE2-search patterns, which never
// latch) is split in halves.
int build_groups(const std::vector<const re::Ast*>& asts, std::vector<uint32_t> idx,
                 const FieldDfaLimits& lim, std::vector<Group>* out, std::string* err) {
  std::vector<const re::Ast*> sub;
  for (uint32_t i : idx) sub.push_back(asts[i]);
  Group g;
  re::Status st = build_field_dfa(sub, lim, &g.pk);
  if (st == re::Status::Ok) {
    g.pats = std::move(idx);
    out->push_back(std::move(g));
    return L7M_OK;
  }
  if (st != re::Status::TooBig) {
    *err = "DFA construction failed";
    return L7M_EUNSUPPORTED;
  }
  if (idx.size() == 1) {
    *err = "a single pattern exceeds the DFA state/table limit";
    return L7M_ETOOBIG;
  }
  size_t h = idx.size() / 2;
  std::vector<uint32_t> a(idx.begin(), idx.begin() + h), b(idx.begin() + h, idx.end());
  int rc = build_groups(asts, std::move(a), lim, out, err);
  if (rc != L7M_OK) return rc;
  return build_groups(asts, std::move(b), lim, out, err);
}

constexpr size_t kLitMinBytes = 16;  // shorter literal values are walked byte by byte

// ---- phase 1: rule matchers ------------------------------------------
struct RM {
  uint32_t field;
  MatchKind kind;
  uint32_t fpat;  // field pattern index (kNone for Present)
};

struct Matchers {
  std::vector<std::string> field_names = {":method", ":path", ":authority"};  // then referenced headers, lower-case
  std::vector<std::vector<FieldPattern>> fpats =    // [field]: its distinct Regex / Value patterns
      std::vector<std::vector<FieldPattern>>(3);
  std::vector<std::vector<RM>> rule_m;              // [rule]: matchers in getHTTPRule order
  uint32_t nf() const { return static_cast<uint32_t>(field_names.size()); }
};

// translate_http_rule per rule; a field per referenced name, a pattern index
// per distinct (kind, value) of a field.
Err match_rules(const l7m_http_rule* rules, size_t n, Matchers* out) {
  std::vector<std::string>& field_names = out->field_names;
  std::vector<std::vector<FieldPattern>>& fpats = out->fpats;
  std::unordered_map<std::string, uint32_t> field_of = {
      {":method", kFieldMethod}, {":path", kFieldPath}, {":authority", kFieldAuthority}};
  std::vector<std::map<FieldPattern, uint32_t>> fpat_idx(3);
  out->rule_m.resize(n);
  std::vector<HeaderMatcher> hm;
  for (size_t i = 0; i < n; ++i) {
    std::string err;
    int rc = translate_http_rule(rules[i], &hm, &err);
    if (rc != L7M_OK) return fail(rc, "rule " + std::to_string(i) + ": " + err);
    if (hm.size() > kCrMaxMatchers)
      return fail(L7M_ETOOBIG, "rule " + std::to_string(i) + ": more than 255 header matchers");
    for (const auto& m : hm) {
      std::string lname = lower_ascii(m.name);  // Envoy LowerCaseString
      auto it = field_of.find(lname);
      uint32_t f;
      if (it == field_of.end()) {
        f = static_cast<uint32_t>(field_names.size());
        if (f >= kMaxFields)
          return fail(L7M_ETOOBIG, "more than 64 distinct header fields referenced");
        field_of.emplace(lname, f);
        field_names.push_back(lname);
        fpat_idx.emplace_back();
        fpats.emplace_back();
      } else {
        f = it->second;
      }
      MatchKind k = envoy_kind(m);
      RM r{f, k, kNone};
      if (k != MatchKind::Present) {
        FieldPattern fp{k, m.value};
        auto pit = fpat_idx[f].find(fp);
        if (pit == fpat_idx[f].end()) {
          pit = fpat_idx[f].emplace(fp, static_cast<uint32_t>(fpats[f].size())).first;
          fpats[f].push_back(fp);
        }
        r.fpat = pit->second;
      }
      out->rule_m[i].push_back(r);
    }
  }
  return {};
}

// ---- phase 2: the automata of one field ------------------------------
// A back-reference whose capture is forced (regex_ecma.h DcapForm): decided
// in the first pass.  The list is shared by the fields; it grows in field and
// pattern order and stops at kMaxDcap.
struct DcapOut {
  uint32_t field;
  re::DcapForm form;
  PackedDfa rpk;  // R's full-match automaton (unless form.r_empty)
};

struct FieldAutomata {
  std::vector<Group> groups;
  // slow-path programs (regex_vm.h) of the patterns whose automata are
  // supersets (back-references, oversized look-ahead): [pattern]
  std::vector<std::vector<uint32_t>> slow_vm;
  std::vector<uint32_t> dcap_of;                      // [pattern] -> dcap id, kNone otherwise
  std::vector<std::pair<uint32_t, uint32_t>> fp_loc;  // [pattern] -> (group, local id)
  GramFilter gram;  // RE2 dialect: which search groups a value may need
  AlitField alit;   // RE2 dialect: the literal-anchored patterns
};

// One pattern of field f in its dialect -> the Ast its automaton is built
// from, and, where that automaton is a superset, a forced capture or a
// slow-path program.
Err parse_pattern(const FieldPattern& fp, uint32_t f, const std::string& field_name, bool re2, re::Ast* ast,
                  std::vector<uint32_t>* slow_vm, uint32_t* dcap_of, std::vector<DcapOut>* dcaps) {
  if (fp.kind == MatchKind::Regex && re2) {
    // Go regexp.MustCompile(p).MatchString(v): RE2 syntax, unanchored.
    std::string perr;
    re::Status st = re::parse_re2(fp.value, ast, &perr);
    if (st == re::Status::Syntax)
      return fail(L7M_EINVAL_REGEX, "invalid regex '" + fp.value + "' on " + field_name + ": " + perr +
                                        " (regexp.Compile would fail)");
    if (st != re::Status::Ok)
      return fail(L7M_EUNSUPPORTED, "regex '" + fp.value + "': " + perr + " is outside the RE2 byte subset");
    return {};
  }
  if (fp.kind != MatchKind::Regex) {
    *ast = re::literal_ast(fp.value);
    return {};
  }
  try {
    std::regex probe(fp.value, std::regex::ECMAScript | std::regex::optimize);
    (void)probe;
  } catch (const std::regex_error& e) {
    return fail(L7M_EINVAL_REGEX, "invalid regex '" + fp.value + "' on " + field_name +
                                      ": " + e.what() + " (Envoy would NACK the policy)");
  }
  std::string perr;
  re::Ast full;
  re::Status st = re::parse_ecma(fp.value, &full, &perr);
  if (st == re::Status::TooBig)
    return fail(L7M_ETOOBIG, "regex '" + fp.value + "': " + perr);
  if (st != re::Status::Ok)
    return fail(L7M_EUNSUPPORTED, "regex '" + fp.value + "': " + perr + " (parser disagrees with std::regex)");
  bool exact = true;
  *ast = re::lower_for_dfa(full, &exact);
  if (exact && re::has_node(*ast, re::Node::Look)) {
    // look-ahead is determinised exactly (regex_ecma.cc build_ctx)
    // unless its automaton exceeds kLookMaxStates: then the DFA carries
    // the pattern without it (a superset) and the slow path decides
    re::Dfa probe;
    re::DfaLimits ll;
    ll.max_states = kLookMaxStates;
    if (re::build_dfa({ast}, ll, &probe) != re::Status::Ok) {
      *ast = re::drop_lookahead(*ast);
      exact = false;
    }
  }
  re::DcapForm form;
  if (!exact && dcaps->size() < kMaxDcap && re::analyze_dcap(full, &form)) {
    // a forced capture: the superset automaton plus byte compares in
    // the first pass decide it exactly (no slow path)
    DcapOut dc;
    dc.field = f;
    dc.form = std::move(form);
    if (!dc.form.r_empty) {
      std::vector<const re::Ast*> rp{&dc.form.r};
      if (build_field_dfa(rp, FieldDfaLimits(), &dc.rpk) != re::Status::Ok) dc.field = kNone;
    }
    if (dc.field != kNone) {
      *dcap_of = static_cast<uint32_t>(dcaps->size());
      dcaps->push_back(std::move(dc));
      exact = true;
    }
  }
  if (!exact) {
    // the automaton accepts a superset; rules using this pattern are
    // decided by the slow path (libstdc++'s executor restated)
    std::string verr;
    if (!vm_compile(full, slow_vm, &verr))
      return fail(L7M_ETOOBIG, "regex '" + fp.value + "': " + verr);
  }
  return {};
}

// RE2 dialect: the search groups of the regex patterns `sidx` that the alit
// scan left over, and the gram filter over them.
Err build_search_side(const std::vector<re::Ast>& asts, const std::vector<const re::Ast*>& ptrs,
                      const std::vector<uint32_t>& sidx, const std::string& field_name, FieldAutomata* out) {
  // patterns without a 4-byte required literal ("always" walked) are
  // grouped apart from the others, so the gram filter can skip whole groups
  std::vector<std::vector<uint32_t>> grams(asts.size());
  std::vector<uint32_t> s_always, s_lit;
  for (uint32_t p : sidx) {
    for (const std::string& lit : re::required_literals(asts[p]))
      for (size_t i = 0; i + 4 <= lit.size(); ++i) {
        uint32_t g;
        std::memcpy(&g, lit.data() + i, 4);
        grams[p].push_back(g);
      }
    std::sort(grams[p].begin(), grams[p].end());
    grams[p].erase(std::unique(grams[p].begin(), grams[p].end()), grams[p].end());
    (grams[p].empty() ? s_always : s_lit).push_back(p);
  }
  std::string err;
  const uint32_t first = static_cast<uint32_t>(out->groups.size());
  out->gram.search_first = first;
  if (sidx.empty()) {
    // every regex of the field is literal-anchored
  } else if (sidx.size() <= kSearchMaxPats && !out->alit.on) {  // one group: walked anyway, no filter
    int rc = build_search_groups(ptrs, sidx, &out->groups, &err);
    if (rc != L7M_OK) return fail(rc, field_name + ": " + err);
  } else {
    if (!s_always.empty()) {
      int rc = build_search_groups(ptrs, s_always, &out->groups, &err);
      if (rc != L7M_OK) return fail(rc, field_name + ": " + err);
    }
    const uint32_t first_lit = static_cast<uint32_t>(out->groups.size());
    if (!s_lit.empty()) {
      int rc = build_search_groups(ptrs, s_lit, &out->groups, &err);
      if (rc != L7M_OK) return fail(rc, field_name + ": " + err);
    }
    build_gram_filter(out->groups, first, first_lit, grams, &out->gram);
  }
  out->gram.n_search = static_cast<uint32_t>(out->groups.size()) - first;
  return {};
}

// Field f's patterns -> its groups in order: packed full-match groups, search
// groups, then kDfaAlit groups.  no_alit: keep literal-anchored patterns in
// search groups.
Err build_field_automata(uint32_t f, const std::string& field_name, const std::vector<FieldPattern>& fpats, bool re2,
                         const FieldDfaLimits& lim, bool no_alit, FieldAutomata* out, std::vector<DcapOut>* dcaps) {
  std::vector<re::Ast> asts(fpats.size());
  std::vector<const re::Ast*> ptrs;
  out->slow_vm.resize(fpats.size());
  out->dcap_of.assign(fpats.size(), kNone);
  for (size_t p = 0; p < fpats.size(); ++p) {
    const Err e = parse_pattern(fpats[p], f, field_name, re2, &asts[p], &out->slow_vm[p], &out->dcap_of[p], dcaps);
    if (!e.ok()) return e;
    ptrs.push_back(&asts[p]);
  }
  // RE2 dialect: regex patterns become search automata (program.h
  // kDfaSearch); literal header values stay full-match packed automata
  std::vector<uint32_t> idx, sidx;
  for (uint32_t p = 0; p < fpats.size(); ++p)
    (re2 && fpats[p].kind == MatchKind::Regex ? sidx : idx).push_back(p);
  if (!idx.empty()) {
    std::string err;
    int rc = build_groups(ptrs, idx, lim, &out->groups, &err);
    if (rc != L7M_OK) return fail(rc, field_name + ": " + err);
  }
  if (!sidx.empty()) {
    // literal-anchored patterns (L R) leave the search groups: an alit scan
    // decides them (gram probe, literal compare, shared residual automaton)
    std::vector<uint32_t> rest;
    if (no_alit) rest = sidx;
    else plan_alit(asts, sidx, &out->alit, &rest);
    const Err e = build_search_side(asts, ptrs, rest, field_name, out);
    if (!e.ok()) return e;
  }
  AlitField& alit = out->alit;
  if (alit.on) {  // kDfaAlit groups of <= kSearchMaxPats patterns, after the search groups
    alit.first_group = static_cast<uint32_t>(out->groups.size());
    for (size_t o = 0; o < alit.pats.size(); o += kSearchMaxPats) {
      Group g;
      g.alit = true;
      g.pats.assign(alit.pats.begin() + o, alit.pats.begin() + std::min(alit.pats.size(), o + kSearchMaxPats));
      out->groups.push_back(std::move(g));
    }
  }
  out->fp_loc.assign(fpats.size(), {0, 0});
  for (uint32_t g = 0; g < out->groups.size(); ++g)
    for (uint32_t l = 0; l < out->groups[g].pats.size(); ++l)
      out->fp_loc[out->groups[g].pats[l]] = {g, l};
  return {};
}

// ---- phase 3: header-name automaton, global automaton numbering ------
struct Numbering {
  bool has_name = false;
  PackedDfa name_dfa;               // over every regular field name (exact, lower-case)
  std::vector<uint32_t> dfa_first;  // [field]: fields in order, groups in order
  uint32_t ndfa = 0;                // value automata (groups) of all fields
};

Err number_automata(const Matchers& m, const std::vector<FieldAutomata>& fa, Numbering* out) {
  const uint32_t nf = m.nf();
  out->has_name = nf > 3;
  if (out->has_name) {
    std::vector<re::Ast> asts;
    for (uint32_t f = 3; f < nf; ++f) asts.push_back(re::literal_ast(m.field_names[f]));
    std::vector<const re::Ast*> ptrs;
    for (auto& a : asts) ptrs.push_back(&a);
    if (build_field_dfa(ptrs, FieldDfaLimits(), &out->name_dfa) != re::Status::Ok)
      return fail(L7M_ETOOBIG, "header-name DFA too large");
  }
  out->dfa_first.assign(nf, 0);
  for (uint32_t f = 0; f < nf; ++f) {
    out->dfa_first[f] = out->ndfa;
    out->ndfa += static_cast<uint32_t>(fa[f].groups.size());
  }
  return {};
}

// ---- phase 4: rule keys ----------------------------------------------
struct RuleKeys {
  std::vector<std::vector<std::vector<uint32_t>>> keyed;  // [dfa][local pattern]: rules keyed on it
  std::vector<std::vector<uint32_t>> pres_keyed;          // [field]: rules keyed on its presence
  uint32_t always_rule = kNone;
  std::vector<uint32_t> zero_list;  // no matchers, remote-restricted
  std::vector<std::vector<uint32_t>> remotes;  // [rule]: sorted, unique
  bool any_remotes = true;
  // rules with slow-path matchers: (field, pattern) pairs, in matcher order
  std::vector<uint8_t> slow_rule;
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> slow_list;
  uint32_t n_slow = 0;
};

uint32_t field_rank(uint32_t f) {
  if (f == kFieldPath) return 0;
  if (f == kFieldAuthority) return 1;
  if (f == kFieldMethod) return 3;
  return 2;
}

// Every rule is keyed on its most selective matcher: a pattern before a
// presence, then the pattern fewest rules share, then the field's rank.
Err key_rules(const l7m_http_rule* rules, size_t n, const PolicyPlan& plan, const Matchers& m,
              const std::vector<FieldAutomata>& fa, const Numbering& num, RuleKeys* out) {
  const uint32_t nf = m.nf();
  std::vector<std::vector<uint32_t>> share(nf);
  for (uint32_t f = 0; f < nf; ++f) share[f].assign(m.fpats[f].size(), 0);
  for (size_t i = 0; i < n; ++i) {
    std::vector<std::pair<uint32_t, uint32_t>> seen;
    for (const auto& rm : m.rule_m[i])
      if (rm.fpat != kNone) {
        auto key = std::make_pair(rm.field, rm.fpat);
        if (std::find(seen.begin(), seen.end(), key) == seen.end()) {
          seen.push_back(key);
          share[rm.field][rm.fpat]++;
        }
      }
  }
  out->keyed.resize(num.ndfa);
  for (uint32_t f = 0; f < nf; ++f)
    for (uint32_t g = 0; g < fa[f].groups.size(); ++g)
      out->keyed[num.dfa_first[f] + g].resize(fa[f].groups[g].pats.size());
  out->pres_keyed.resize(nf);
  out->remotes.resize(n);
  for (size_t i = 0; i < n; ++i) {
    if (rules[i].n_remote_ids) {
      if (!rules[i].remote_ids) return fail(L7M_EINVAL, "remote_ids == NULL with n_remote_ids > 0");
      auto& r = out->remotes[i];
      r.assign(rules[i].remote_ids, rules[i].remote_ids + rules[i].n_remote_ids);
      std::sort(r.begin(), r.end());
      r.erase(std::unique(r.begin(), r.end()), r.end());
      out->any_remotes = false;
    }
  }
  auto score = [&share](const RM& rm) {
    uint64_t pres = rm.kind == MatchKind::Present ? 1 : 0;
    uint64_t sh = rm.fpat == kNone ? 0xffffffffu : share[rm.field][rm.fpat];
    return (pres << 60) | (sh << 8) | field_rank(rm.field);
  };
  for (size_t i = 0; i < n; ++i) {
    if (m.rule_m[i].empty()) {
      // matcher-less rules: the smallest unrestricted one decides outright in a
      // one-entry map; otherwise they are checked like any other candidate
      // (remote set, port entry)
      if (plan.single && out->remotes[i].empty()) {
        if (out->always_rule == kNone) out->always_rule = static_cast<uint32_t>(i);
      } else {
        out->zero_list.push_back(static_cast<uint32_t>(i));
      }
      continue;
    }
    const RM* best = nullptr;
    for (const auto& rm : m.rule_m[i])
      if (!best || score(rm) < score(*best)) best = &rm;
    if (best->kind == MatchKind::Present) {
      out->pres_keyed[best->field].push_back(static_cast<uint32_t>(i));
    } else {
      auto loc = fa[best->field].fp_loc[best->fpat];
      out->keyed[num.dfa_first[best->field] + loc.first][loc.second].push_back(static_cast<uint32_t>(i));
    }
  }
  out->slow_rule.assign(n, 0);
  out->slow_list.resize(n);
  for (size_t i = 0; i < n; ++i) {
    for (const auto& rm : m.rule_m[i])
      if (rm.fpat != kNone && !fa[rm.field].slow_vm[rm.fpat].empty()) out->slow_list[i].push_back({rm.field, rm.fpat});
    if (!out->slow_list[i].empty()) {
      out->slow_rule[i] = 1;
      ++out->n_slow;
    }
  }
  return {};
}

// What phases 1-4 make of the rules; read-only from phase 5 on.
struct Front {
  size_t n = 0;  // rules
  bool re2 = false;
  Matchers m;
  std::vector<FieldAutomata> fa;  // [field]
  std::vector<DcapOut> dcaps;
  Numbering num;
  RuleKeys keys;
};

// ---- phase 5: descriptors and check records --------------------------
struct DfaOut {
  const PackedDfa* d;
  uint32_t field;
  uint32_t npats;
  const Group* grp;  // nullptr for the name DFA
};

// The u32 pool (set pattern lists, remote ids, slow-path pairs) and the check
// records (program.h): one per (list, rule).
struct Records {
  std::vector<uint32_t> pool, cr;
  Span push_list(const std::vector<uint32_t>& v) {
    Span s{static_cast<uint32_t>(pool.size()), static_cast<uint32_t>(v.size())};
    pool.insert(pool.end(), v.begin(), v.end());
    return s;
  }
  Span push_records(const std::vector<uint32_t>& rids, const Front& fr, const PolicyPlan& plan) {
    Span s{static_cast<uint32_t>(cr.size()), static_cast<uint32_t>(rids.size())};
    for (uint32_t rid : rids) {
      const auto& rule_m = fr.m.rule_m[rid];
      cr.push_back(rid);
      cr.push_back(static_cast<uint32_t>(rule_m.size()) | plan.rule_entry[rid] << kCrEntryShift |
                   (fr.keys.remotes[rid].empty() ? 0u : kCrRemote) | (fr.keys.slow_rule[rid] ? kCrSlow : 0u));
      for (const auto& m : rule_m) {
        uint32_t dfa = 0, pat = 0, dcap = kNone;
        if (m.fpat != kNone) {
          auto loc = fr.fa[m.field].fp_loc[m.fpat];
          dfa = fr.num.dfa_first[m.field] + loc.first;
          pat = loc.second;
          dcap = fr.fa[m.field].dcap_of[m.fpat];
        }
        const uint32_t kind = m.kind == MatchKind::Present ? 1u : 0u;
        cr.push_back(m.field | (kind << 8) | (dfa << 9));
        if (dcap != kNone) pat |= (dcap + 1) << kDcapShift;
        cr.push_back(pat);
      }
    }
    return s;
  }
};

// The program's tables before they have addresses.  Phases 6-9 fill in the
// lds_* / *_off members of dd and fd; everything else is fixed by phase 5
// (dense, n_dense and the dense automata's share of total_states by phase 7).
struct Tables {
  // value groups (index = global DFA number), the name automaton, the
  // literal-anchored fields' residual automata, the forced captures' R automata
  std::vector<DfaOut> all;
  std::vector<uint32_t> resid_dfa;  // [field] -> index in all, or kNone
  std::vector<uint32_t> dcap_rdfa;  // [dcap] -> index in all, or kNone
  std::vector<DfaDesc> dd;          // [all]
  std::vector<FieldDesc> fd;        // [field]
  std::vector<Span> sets;
  std::vector<std::vector<Span>> ct;         // per DFA: [nsets + npats]
  std::vector<std::vector<uint64_t>> masks;  // per DFA with npats <= 64
  std::vector<uint32_t> name_field;
  std::vector<Span> rremote;  // [rule]
  Span zero_span{0, 0};
  Records rec;
  uint64_t total_states = 0;
  std::vector<DenseDfa> dense;  // [all]: of the kDfaDense ones
  uint32_t n_dense = 0;
  uint32_t ndt() const { return static_cast<uint32_t>(all.size()); }
};

DfaDesc init_dfa_desc(const DfaOut& o, uint32_t set_base) {
  const PackedDfa& d = *o.d;
  DfaDesc dd;
  std::memset(&dd, 0, sizeof(DfaDesc));
  dd.start_base = d.start_base;
  dd.region = d.region;
  dd.start_latch = d.start_latch;
  dd.n_slots = d.n_slots;
  dd.nsets = static_cast<uint32_t>(d.sets.size());
  dd.npats = o.npats;
  dd.set_base = set_base;
  dd.field = o.field;
  dd.nstates = d.nstates;
  dd.lds_table = dd.lds_es = dd.lds_latch = dd.lds_ct = dd.lds_mask = kNone;
  dd.lds_ctmask = kNone;
  dd.lit_tab = kNone;
  dd.lds_skip = kNone;
  dd.skip_lim = 0;
  dd.kind = kDfaPacked;
  dd.lds_search = dd.lds_mid = kNone;
  if (o.grp && o.grp->alit) {  // no automaton: codes from the field's alit scan
    dd.kind = kDfaAlit;
    dd.start_base = 0;
    dd.region = 0;
    dd.n_slots = 0;
    dd.nstates = 0;
  }
  if (o.grp && o.grp->search) {
    const SearchDfa& sd = o.grp->sd;
    dd.kind = kDfaSearch;
    dd.start_base = sd.start;
    dd.start_es8 = sd.start_mid;
    dd.region = 0;
    dd.n_slots = sd.nstates * sd.ncls;
    dd.nstates = sd.nstates;
    dd.acc_ncls = sd.ncls;
  }
  return dd;
}

// (presence: the field's check records; the tables are placed in the LDS image later)
FieldDesc init_field_desc(const Front& fr, uint32_t f, Span presence, uint32_t resid_dfa) {
  FieldDesc fd;
  std::memset(&fd, 0, sizeof(FieldDesc));
  fd.dfa_first = fr.num.dfa_first[f];
  fd.ndfa = static_cast<uint32_t>(fr.fa[f].groups.size());
  fd.presence = presence;
  fd.gram_tab = kNone;
  fd.always = ~0u;
  fd.search_first = fr.fa[f].gram.search_first;
  fd.n_search = fr.fa[f].gram.n_search;
  fd.alit_tab = fd.alit_pats = kNone;
  for (size_t k = 0; k < fr.dcaps.size(); ++k)
    if (fr.dcaps[k].field == f) fd.dcap_mask |= 1u << k;
  fd.resid_dfa = resid_dfa;
  return fd;
}

Err build_records(const Front& fr, const PolicyPlan& plan, Tables* t) {
  const uint32_t nf = fr.m.nf(), ndfa = fr.num.ndfa;
  if (ndfa >= (1u << 23)) return fail(L7M_ETOOBIG, "too many DFA groups");
  std::vector<DfaOut>& all = t->all;
  for (uint32_t f = 0; f < nf; ++f)
    for (auto& g : fr.fa[f].groups) all.push_back({&g.pk, f, static_cast<uint32_t>(g.pats.size()), &g});
  if (fr.num.has_name) all.push_back({&fr.num.name_dfa, kNone, nf - 3, nullptr});
  t->resid_dfa.assign(nf, kNone);
  for (uint32_t f = 0; f < nf; ++f)
    if (fr.fa[f].alit.on && fr.fa[f].alit.n_resid) {
      t->resid_dfa[f] = static_cast<uint32_t>(all.size());
      all.push_back({&fr.fa[f].alit.resid_pk, f, fr.fa[f].alit.n_resid, nullptr});
    }
  t->dcap_rdfa.assign(fr.dcaps.size(), kNone);
  for (size_t k = 0; k < fr.dcaps.size(); ++k)
    if (!fr.dcaps[k].form.r_empty) {
      t->dcap_rdfa[k] = static_cast<uint32_t>(all.size());
      all.push_back({&fr.dcaps[k].rpk, fr.dcaps[k].field, 1, nullptr});
    }
  const uint32_t ndt = t->ndt();

  t->dd.resize(ndt);
  t->ct.resize(ndt);
  t->masks.resize(ndt);
  for (uint32_t k = 0; k < ndt; ++k) {
    const PackedDfa& d = *all[k].d;
    t->dd[k] = init_dfa_desc(all[k], static_cast<uint32_t>(t->sets.size()));
    t->total_states += t->dd[k].nstates;
    for (size_t s = 0; s < d.sets.size(); ++s) {
      t->sets.push_back(t->rec.push_list(d.sets[s]));
      if (k < ndfa) {
        std::vector<uint32_t> c;
        for (uint32_t p : d.sets[s]) {
          const auto& kl = fr.keys.keyed[k][p];
          c.insert(c.end(), kl.begin(), kl.end());
        }
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        t->ct[k].push_back(t->rec.push_records(c, fr, plan));
      }
      if (all[k].npats <= 64) {
        uint64_t m = 0;
        for (uint32_t p : d.sets[s]) m |= 1ull << p;
        t->masks[k].push_back(m);
      }
    }
    if (k < ndfa)
      for (const auto& rids : fr.keys.keyed[k]) t->ct[k].push_back(t->rec.push_records(rids, fr, plan));
  }
  if (fr.num.has_name)
    for (const auto& s : fr.num.name_dfa.sets) t->name_field.push_back(s.empty() ? kNone : 3 + s[0]);
  for (uint32_t f = 0; f < nf; ++f)
    t->fd.push_back(init_field_desc(fr, f, t->rec.push_records(fr.keys.pres_keyed[f], fr, plan), t->resid_dfa[f]));
  for (size_t i = 0; i < fr.n; ++i) t->rremote.push_back(t->rec.push_list(fr.keys.remotes[i]));
  t->zero_span = t->rec.push_records(fr.keys.zero_list, fr, plan);
  t->rec.cr.insert(t->rec.cr.end(), 8, 0u);  // the kernel fetches 8 words per record
  return {};
}

// ---- phase 6: LDS image placement ------------------------------------
// Descriptors always; then, hottest DFA first (header names, path,
// authority, method, header values), slot table + u16 end codes/latches; then
// candidate tables and set masks, within the budget.  Every take moves the
// cursor the later budget tests read: the order below is part of the output.
struct Image {
  WordAlloc cur;        // image words, 16-byte granules
  uint64_t budget = 0;  // image words the table placements may fill
  uint32_t lds_dfas = 0, lds_fields = 0, lds_name_field = 0;
  uint32_t lds_dcap = kNone;  // forced-capture specs, then per spec its literals P1, L2
  std::vector<uint32_t> dcap_p1, dcap_l2;
  uint32_t lds_name_tab = kNone, name_slots = 0;  // header-name hash table
  std::vector<uint32_t> name_off;                 // [field - 3]: its name's bytes
  uint32_t ent_slots = 2, lds_ent_tab = kNone;    // port-entry table
  std::vector<uint32_t> ent_tab;
  std::vector<uint64_t> alit_words;  // [field]: AlitRecs (header + literal granules)
  uint64_t at() const { return cur.at; }
  uint32_t take(uint64_t words) { return cur.take(words, 4); }
  bool fits(uint64_t words) const { return cur.at + round4(words) <= budget; }
};

// The always-resident part and what the kernel's other LDS users leave: the
// per-lane end-code columns (more than kHttpRegDfas value DFAs: 4 bytes x
// kHttpBlock lanes each), the hit counters (when they fit kMaxLdsCounters)
// and a record stage of at least kHttpMinStage bytes per wave
// (l7m_kernels.hip http_lds_bytes).  What is left bounds the table image;
// rule sets whose fixed part does not fit are rejected here, when the policy
// loads, not on every batch.
Err place_fixed(const Front& fr, const l7m_opts& opts, const Tables& t, Image* im) {
  const uint32_t nf = fr.m.nf(), ndfa = fr.num.ndfa;
  const size_t n = fr.n;
  bool any_search = false;
  for (uint32_t f = 0; f < nf; ++f)
    for (const auto& g : fr.fa[f].groups) any_search |= g.search;
  // (search programs keep their end codes in a global scratch, l7m_kernels.hip)
  const uint64_t codes_bytes = ndfa > kHttpRegDfas && !any_search ? 4ull * kHttpBlock * ndfa : 0;
  const uint64_t ctr_bytes = n + 2 <= kMaxLdsCounters ? 4ull * round4(n + 2) : 0;
  const uint64_t stage_bytes = static_cast<uint64_t>(kHttpWaves) * (kHttpMinStage + 16);
  im->take(256);  // image words [0, 256): the zero dead row of every LDS slot table (program.h kLdsRowShift)
  im->lds_dfas = im->take(static_cast<uint64_t>(t.ndt()) * sizeof(DfaDesc) / 4);
  im->lds_fields = im->take(static_cast<uint64_t>(nf) * sizeof(FieldDesc) / 4);
  im->lds_name_field = im->take(t.name_field.size());
  // forced-capture specs and their literals (read by every walk of their field)
  im->dcap_p1.resize(fr.dcaps.size());
  im->dcap_l2.resize(fr.dcaps.size());
  if (!fr.dcaps.empty()) {
    im->lds_dcap = im->take(16ull * fr.dcaps.size());
    for (size_t k = 0; k < fr.dcaps.size(); ++k) {
      im->dcap_p1[k] = im->take((fr.dcaps[k].form.p1.size() + 3) / 4);
      im->dcap_l2[k] = im->take((fr.dcaps[k].form.l2.size() + 3) / 4);
    }
  }
  const uint64_t other = codes_bytes + ctr_bytes + stage_bytes, fixed = 4 * im->at() + other;
  if (fixed > kHttpLdsBytes)
    return fail(L7M_ETOOBIG, std::to_string(ndfa) + " value DFA groups over " + std::to_string(nf) +
                                 " fields need " + std::to_string(fixed) + " bytes of fixed LDS (descriptors, "
                                 "end-code columns, counters, record stage) > " + std::to_string(kHttpLdsBytes));
  uint64_t budget_bytes = opts.lds_budget_bytes ? opts.lds_budget_bytes : kDefaultLdsBudget;
  budget_bytes = std::min<uint64_t>(budget_bytes, other < kHttpLdsBytes ? kHttpLdsBytes - other : 0);
  im->budget = budget_bytes / 4;
  return {};
}

// The tables a walk reads once per value byte: the header-name table, the
// literal-anchored fields' bucket tables, the gram filters, the search
// automata's mid masks and the residual automata.
Err place_scan_tables(const Front& fr, Tables* t, Image* im, uint32_t* alit_over) {
  const uint32_t nf = fr.m.nf();
  // header-name table (always resident when it fits)
  if (fr.num.has_name) {
    im->name_slots = 2;
    while (im->name_slots < 2 * (nf - 3)) im->name_slots <<= 1;
    uint64_t words = 4ull * im->name_slots;
    for (uint32_t f = 3; f < nf; ++f) words += round4((fr.m.field_names[f].size() + 3) / 4);
    if (4 * words <= kMaxNameTabBytes && im->at() + words <= im->budget) {
      im->lds_name_tab = im->take(4ull * im->name_slots);
      for (uint32_t f = 3; f < nf; ++f) im->name_off.push_back(im->take((fr.m.field_names[f].size() + 3) / 4));
    }
  }
  // RE2-dialect literal-anchored patterns: the bucket table (read once per
  // value byte; their groups have no automaton, so it must be resident)
  for (uint32_t f = 0; f < nf; ++f) {
    const AlitField& alit = fr.fa[f].alit;
    if (!alit.on) continue;
    if (im->at() + kAlitBloomWords + alit.tab.size() > im->budget) {
      // not resident: the caller compiles again with this field's patterns
      // as plain search groups (a policy that compiled before the alit scan
      // existed still compiles)
      *alit_over = f;
      return fail(L7M_ETOOBIG, fr.m.field_names[f] + ": the literal-anchored pattern table needs " +
                                   std::to_string(4 * alit.tab.size()) + " bytes of LDS");
    }
    // prefilter bits, then the table
    t->fd[f].alit_tab = im->take(kAlitBloomWords + alit.tab.size()) + kAlitBloomWords;
    t->fd[f].alit_mask = static_cast<uint32_t>(alit.tab.size() / 4 - 1);
  }
  // RE2-dialect gram filters (read once per value byte): right after the name table
  for (uint32_t f = 0; f < nf; ++f) {
    const GramFilter& gram = fr.fa[f].gram;
    if (!gram.on || im->at() + gram.tab.size() > im->budget) continue;
    t->fd[f].gram_tab = im->take(gram.tab.size());
    t->fd[f].gram_mask = static_cast<uint32_t>(gram.tab.size() / 4 - 1);
    t->fd[f].always = gram.always;
  }
  // search automata's mid masks (one read per value byte, <= 256 words each):
  // in LDS, so a search step costs one L2 request (the table entry), not two
  for (uint32_t k = 0; k < t->ndt(); ++k) {
    if (!t->all[k].grp || !t->all[k].grp->search) continue;
    const uint64_t mw = t->all[k].grp->sd.midmask.size();
    if (im->fits(mw)) t->dd[k].lds_mid = im->take(mw);
  }
  // ... the residual automata they walk (slot table + end codes, pattern masks)
  for (uint32_t f = 0; f < nf; ++f) {
    const uint32_t k = t->resid_dfa[f];
    if (k == kNone || t->fd[f].alit_tab == kNone) continue;
    const PackedDfa& d = *t->all[k].d;
    const uint64_t half_latch = (d.latch.size() + 1) / 2;
    const bool es8 = d.sets.size() < kEs8Latched && t->all[k].npats < kEs16Latched;
    if (es8 && im->at() + d.n_slots <= kLdsTableWords &&
        im->at() + round4(d.n_slots) + round4(half_latch) <= im->budget) {
      t->dd[k].lds_table = im->take(d.n_slots);
      t->dd[k].lds_es = kLdsEsInEntry;
      t->dd[k].lds_latch = 2 * im->take(half_latch);
    }
    if (!t->masks[k].empty() && im->fits(2 * t->masks[k].size())) t->dd[k].lds_mask = im->take(2 * t->masks[k].size());
  }
  return {};
}

int hotness(uint32_t field) {
  if (field == kNone) return 0;
  if (field == kFieldPath) return 1;
  if (field == kFieldAuthority) return 2;
  if (field == kFieldMethod) return 3;
  return 4;
}

// The slot table of packed automaton k with, while the budget lasts, its end
// codes in the entries (es8), in a u16 table (es16), or left in the program.
void place_slot_table(uint32_t k, Tables* t, Image* im) {
  const PackedDfa& d = *t->all[k].d;
  DfaDesc& dd = t->dd[k];
  const uint64_t half_es = (d.n_slots + 1) / 2, half_latch = (d.latch.size() + 1) / 2;
  const uint64_t need = round4(d.n_slots) + round4(half_es) + round4(half_latch);
  const bool es16 = d.sets.size() < kEs16Latched && t->all[k].npats < kEs16Latched;
  const bool es8 = d.sets.size() < kEs8Latched && t->all[k].npats < kEs16Latched;
  if (im->at() + d.n_slots > kLdsTableWords) return;  // rows are 16-bit byte addresses (program.h)
  const uint64_t need8 = round4(d.n_slots) + round4(half_latch);
  if (es8 && im->at() + need8 <= im->budget) {  // end codes ride in the slot entries
    dd.lds_table = im->take(d.n_slots);
    dd.lds_es = kLdsEsInEntry;
    dd.lds_latch = 2 * im->take(half_latch);
  } else if (es16 && im->at() + need <= im->budget) {
    dd.lds_table = im->take(d.n_slots);
    dd.lds_es = 2 * im->take(half_es);
    dd.lds_latch = 2 * im->take(half_latch);
  } else if (im->fits(d.n_slots)) {
    // the slot table (read once per byte) alone; end codes / latches (read
    // once per walk) stay in the program
    dd.lds_table = im->take(d.n_slots);
  }
}

// The port-entry table, the candidate bitmasks, then per automaton in
// hotness order the slot tables, the pattern masks, the candidate tables,
// and last the literal-anchored patterns' records.
void place_automata(const Front& fr, const PolicyPlan& plan, Tables* t, Image* im) {
  const uint32_t nf = fr.m.nf(), ndfa = fr.num.ndfa, ndt = t->ndt();
  // (policy, direction, port) -> port entry table (open addressing on
  // ent_hash, program.h); in LDS when small
  uint32_t& ent_slots = im->ent_slots;
  while (ent_slots < 2 * plan.keys.size()) ent_slots <<= 1;
  im->ent_tab.assign(2ull * ent_slots, 0);
  for (const auto& kv : plan.keys) {
    uint32_t at = ent_hash(kv.first) & (ent_slots - 1);
    while (im->ent_tab[2 * at]) at = (at + 1) & (ent_slots - 1);
    im->ent_tab[2 * at] = kv.first + 1;
    im->ent_tab[2 * at + 1] = kv.second | (plan.entry_have_http[kv.second] ? kEntHaveHttp : 0u);
  }
  if (!plan.single && 2ull * ent_slots <= kMaxLdsEntWords && im->at() + 2ull * ent_slots <= im->budget)
    im->lds_ent_tab = im->take(2ull * ent_slots);
  // candidate-presence bitmasks: one bit per end code; small ones in LDS
  for (uint32_t k = 0; k < ndfa; ++k) {
    const uint64_t words = (t->ct[k].size() + 31) / 32;
    if (words <= kMaxLdsCtmaskWords && im->at() + words <= im->budget) t->dd[k].lds_ctmask = im->take(words);
  }
  std::vector<uint32_t> order(ndt);
  for (uint32_t k = 0; k < ndt; ++k) order[k] = k;
  std::stable_sort(order.begin(), order.end(),
                   [t](uint32_t a, uint32_t b) { return hotness(t->all[a].field) < hotness(t->all[b].field); });
  for (uint32_t k : order) {
    DfaDesc& dd = t->dd[k];
    if (dd.kind == kDfaAlit || dd.lds_table != kNone) continue;  // no automaton / placed above
    if (dd.kind != kDfaSearch) {
      place_slot_table(k, t, im);
      continue;
    }
    // walked from the program; the 256-byte class map in LDS when it fits
    if (im->at() + 64 <= im->budget) dd.lds_table = im->take(64);
    // small automata (a method's, a few hosts'): the dense table and its mid
    // masks too, so their steps read LDS instead of L2
    const uint64_t tw = t->all[k].grp->sd.table.size();
    if (dd.lds_table != kNone && dd.lds_mid != kNone && tw <= kLdsSearchMaxWords && im->at() + tw <= im->budget)
      dd.lds_search = im->take(tw);
  }
  // Candidate tables are read once per request (after the walks), so they
  // only go to LDS while the image stays small: record staging space is worth
  // more (measured on MI355X, config 2: 5.0 ms with them in HBM vs 5.5 ms).
  const uint64_t ct_budget = std::min<uint64_t>(im->budget, kLdsCtBudget / 4);
  for (uint32_t k : order) {
    if (!t->masks[k].empty() && t->dd[k].lds_mask == kNone && im->fits(2 * t->masks[k].size()))
      t->dd[k].lds_mask = im->take(2 * t->masks[k].size());
  }
  for (uint32_t k : order) {
    const uint64_t words = 16 * t->ct[k].size();
    if (k < ndfa && im->at() + round4(words) <= ct_budget) t->dd[k].lds_ct = im->take(words);
  }
  // literal-anchored patterns' descriptors and literals, last: in LDS when they fit
  // (else program memory)
  im->alit_words.assign(nf, 0);
  for (uint32_t f = 0; f < nf; ++f)
    for (const auto& L : fr.fa[f].alit.lit) im->alit_words[f] += 4ull * alit_rec_granules(L.size());
  for (uint32_t f = 0; f < nf; ++f) {
    if (t->fd[f].alit_tab == kNone) continue;
    const uint64_t words = im->alit_words[f];
    // (read once per candidate: within the table budget only -- config 2's
    // 1000 path records in LDS shrink the record stage, 32.8 vs 26 ms)
    if (im->at() + words > im->budget) continue;
    t->fd[f].alit_lds = 1;
    t->fd[f].alit_pats = im->take(words);
  }
}

// ---- phase 7: dense conversion ---------------------------------------
// Dense class-compressed form (program.h kDfaDense, l7m_opts.flags) of the
// packed automata that stay in the program: the fields' value automata and
// the forced-capture patterns' R automata, never the header-name automaton.
// L7M_OPT_DENSE_DFA converts a group whose u16 table is smaller than its
// slot table (prefix tries are smaller packed), ..._ALWAYS every group that
// fits u16 state ids.  The class map's copy goes to LDS while the budget
// lasts, as for search automata.
void convert_dense(const Front& fr, const l7m_opts& opts, Tables* t, Image* im) {
  const uint32_t ndt = t->ndt();
  t->dense.resize(ndt);
  uint32_t dflags = opts.flags;
  if (const char* e = std::getenv("L7M_DENSE_DFA")) dflags |= static_cast<uint32_t>(std::atoi(e)) & 3u;
  std::vector<char> cand(ndt, 0);
  for (uint32_t k = 0; k < fr.num.ndfa; ++k) cand[k] = 1;
  for (uint32_t k : t->dcap_rdfa)
    if (k != kNone) cand[k] = 1;
  for (uint32_t k = 0; k < ndt && !fr.re2 && (dflags & (L7M_OPT_DENSE_DFA | L7M_OPT_DENSE_DFA_ALWAYS)); ++k) {
    DfaDesc& dd = t->dd[k];
    if (!cand[k] || dd.kind != kDfaPacked || dd.lds_table != kNone) continue;
    const PackedDfa& d = *t->all[k].d;
    DenseDfa dn;
    if (!build_dense(d, &dn)) continue;
    if (!(dflags & L7M_OPT_DENSE_DFA_ALWAYS) && 2ull * dn.table.size() >= 4ull * d.n_slots) continue;
    t->dense[k] = std::move(dn);
    const DenseDfa& D = t->dense[k];
    t->total_states -= dd.nstates;
    dd.kind = kDfaDense;
    dd.start_base = D.start_state;
    dd.region = D.region;
    dd.nstates = D.nstates;
    dd.n_slots = D.nstates * D.ncls;
    dd.acc_ncls = D.ncls;
    dd.lds_cmap = im->at() + 64 <= im->budget ? im->take(64) : kNone;
    t->total_states += dd.nstates;
    ++t->n_dense;
  }
}

// ---- phase 8: program layout -----------------------------------------
struct Layout {
  HttpHeader h;
  WordAlloc w;  // program words
  std::vector<std::vector<uint32_t>> slow_off;   // [field][pattern]: its slow-path program, or kNone
  std::vector<Span> slow_span;                   // [rule]: its (field, program offset) pairs in the pool
  std::vector<std::vector<uint32_t>> lit_words;  // [dfa]: DfaDesc::lit_tab's pairs
};

// The header but for the offsets lay_out assigns.
HttpHeader header_fields(const Front& fr, const PolicyPlan& plan, const Tables& t, const Image& im) {
  const uint32_t nf = fr.m.nf(), ndfa = fr.num.ndfa;
  HttpHeader h;
  std::memset(&h, 0, sizeof h);
  h.magic = kMagicHttp;
  h.n_rules = static_cast<uint32_t>(fr.n);
  h.n_fields = nf;
  h.n_dfas = ndfa;
  h.always_rule = fr.keys.always_rule;
  h.allow_no_l7 = fr.n == 0 ? 1u : 0u;
  h.has_name_dfa = fr.num.has_name ? 1u : 0u;
  h.any_remotes = fr.keys.any_remotes ? 1u : 0u;
  h.zero_list = t.zero_span;
  h.single_entry = plan.single ? 1u : 0u;
  uint64_t m = 0;
  for (uint32_t f = 3; f < nf; ++f) m |= 1ull << std::min<size_t>(fr.m.field_names[f].size(), 63);
  h.name_len_lo = static_cast<uint32_t>(m);
  h.name_len_hi = static_cast<uint32_t>(m >> 32);
  // DFAs / fields the verification must visit (uniform skips in the kernel)
  uint64_t cm = 0, pm = 0;
  for (uint32_t k = 0; k < ndfa && k < 64; ++k)
    for (const Span& sp : t.ct[k])
      if (sp.len) {
        cm |= 1ull << k;
        break;
      }
  for (uint32_t f = 0; f < nf; ++f)
    if (t.fd[f].presence.len) pm |= 1ull << f;
  h.cand_dfas_lo = static_cast<uint32_t>(cm);
  h.cand_dfas_hi = static_cast<uint32_t>(cm >> 32);
  h.pres_fields_lo = static_cast<uint32_t>(pm);
  h.pres_fields_hi = static_cast<uint32_t>(pm >> 32);
  h.n_policies = plan.n_policies;
  h.n_slow = fr.keys.n_slow;
  for (uint32_t k = 0; k < ndfa; ++k) h.search |= t.dd[k].kind == kDfaSearch || t.dd[k].kind == kDfaAlit ? 1u : 0u;
  h.ent_mask = im.ent_slots - 1;
  h.lds_dcap = im.lds_dcap;
  h.lds_image_words = static_cast<uint32_t>(im.at());
  h.lds_dfas = im.lds_dfas;
  h.lds_fields = im.lds_fields;
  h.lds_name_field = im.lds_name_field;
  h.lds_name_tab = im.lds_name_tab;
  h.lds_ent_tab = im.lds_ent_tab;
  h.name_tab_mask = im.lds_name_tab != kNone ? im.name_slots - 1 : 0;
  return h;
}

// Literal values of HBM-walked DFAs (program.h DfaDesc::lit_tab): once such
// a walk is latched on a literal pattern, the kernel compares the rest of
// the field with the literal directly (independent loads) instead of one
// dependent table read per byte.
void lay_out_literals(const Front& fr, Tables* t, Layout* lo) {
  lo->lit_words.resize(t->ndt());
  for (uint32_t k = 0; k < fr.num.ndfa; ++k) {
    DfaDesc& dd = t->dd[k];
    if (dd.lds_table != kNone || !t->all[k].grp || dd.kind == kDfaDense) continue;  // (dense: every byte is walked)
    const Group& g = *t->all[k].grp;
    const std::vector<FieldPattern>& fpats = fr.m.fpats[t->all[k].field];
    bool any = false;
    for (uint32_t l = 0; l < g.pats.size(); ++l) {
      const FieldPattern& fp = fpats[g.pats[l]];
      any |= fp.kind == MatchKind::Value && fp.value.size() >= kLitMinBytes;
    }
    if (!any) continue;
    dd.lit_tab = lo->w.take(2ull * g.pats.size());
    std::vector<uint32_t>& lw = lo->lit_words[k];
    lw.assign(2ull * g.pats.size(), kNone);
    for (uint32_t l = 0; l < g.pats.size(); ++l) {
      const FieldPattern& fp = fpats[g.pats[l]];
      if (fp.kind != MatchKind::Value || fp.value.size() < kLitMinBytes) continue;
      lw[2 * l] = lo->w.take((fp.value.size() + 3) / 4);
      lw[2 * l + 1] = static_cast<uint32_t>(fp.value.size());
    }
  }
}

// Word offsets, in program order: header, descriptors, sets, remotes, slow
// path, entry table, pool, check records, per automaton its tables and
// candidate entries, literal tables, alit records, the LDS image.
Err lay_out(const Front& fr, const Image& im, Tables* t, Layout* lo) {
  const uint32_t nf = fr.m.nf(), ndt = t->ndt();
  const size_t n = fr.n;
  HttpHeader& h = lo->h;
  WordAlloc& w = lo->w;
  w.at = sizeof(HttpHeader) / 4;
  h.off_dfas = w.take(static_cast<uint64_t>(ndt) * sizeof(DfaDesc) / 4);
  h.off_fields = w.take(static_cast<uint64_t>(nf) * sizeof(FieldDesc) / 4);
  h.off_name_field = w.take(t->name_field.size());
  h.off_sets = w.take(t->sets.size() * 2);
  h.off_remotes = w.take(static_cast<uint64_t>(n) * 2);
  // slow path: Span[n_rules] into the pool of (field, program offset) pairs,
  // then the programs
  h.off_slow = kNone;
  lo->slow_off.resize(nf);
  lo->slow_span.assign(n, Span{0, 0});
  if (fr.keys.n_slow) {
    h.off_slow = w.take(2ull * n);
    for (uint32_t f = 0; f < nf; ++f) {
      lo->slow_off[f].assign(fr.m.fpats[f].size(), kNone);
      for (size_t pi = 0; pi < fr.m.fpats[f].size(); ++pi)
        if (!fr.fa[f].slow_vm[pi].empty()) lo->slow_off[f][pi] = w.take(fr.fa[f].slow_vm[pi].size());
    }
    for (size_t i = 0; i < n; ++i) {
      if (fr.keys.slow_list[i].empty()) continue;
      std::vector<uint32_t> pr;
      for (const auto& fp : fr.keys.slow_list[i]) {
        pr.push_back(fp.first);
        pr.push_back(lo->slow_off[fp.first][fp.second]);
      }
      lo->slow_span[i] = t->rec.push_list(pr);
      lo->slow_span[i].len /= 2;  // pairs
    }
  }
  h.ent_tab_off = w.take(2ull * im.ent_slots);
  h.off_pool = w.take(t->rec.pool.size());
  h.off_cr = w.take(t->rec.cr.size());
  for (uint32_t k = 0; k < ndt; ++k) {
    DfaDesc& dd = t->dd[k];
    if (dd.kind == kDfaSearch) {
      dd.table_off = w.take(dd.n_slots);
      dd.es_off = w.take(dd.nstates);  // end masks
      dd.latch_off = w.take(0);
      dd.acc_cmap_off = w.take(256 / 4);
      dd.acc_mid_off = w.take(kSearchMaxMid);
    } else if (dd.kind == kDfaAlit) {
      dd.table_off = dd.es_off = dd.latch_off = w.take(0);
    } else if (dd.kind == kDfaDense) {
      dd.table_off = w.take((t->dense[k].table.size() + 1) / 2);  // u16 entries
      dd.es_off = w.take(t->dense[k].es.size());
      dd.latch_off = w.take(t->dense[k].latch.size());
      dd.acc_cmap_off = w.take(256 / 4);
    } else {
      dd.table_off = w.take(t->all[k].d->n_slots);
      dd.es_off = w.take(t->all[k].d->n_slots);
      dd.latch_off = w.take(t->all[k].d->latch.size());
    }
    w.align(16);  // candidate entries on 64-byte boundaries
    dd.ct_off = w.take(16 * t->ct[k].size());
    dd.ctmask_off = w.take((t->ct[k].size() + 31) / 32);
  }
  lay_out_literals(fr, t, lo);
  // literal-anchored patterns' AlitRecs (program memory, 16-byte aligned)
  // when the LDS image has no room for them
  for (uint32_t f = 0; f < nf; ++f) {
    if (t->fd[f].alit_tab == kNone || t->fd[f].alit_lds) continue;
    w.align(4);
    t->fd[f].alit_pats = w.take(im.alit_words[f]);
  }
  w.align(64);  // 256-byte aligned image
  h.lds_image_off = w.take(im.at());
  if (w.at >= (1ull << 32)) return fail(L7M_ETOOBIG, "program exceeds 16 GiB");
  h.total_words = static_cast<uint32_t>(w.at);
  return {};
}

// ---- phase 9: emit ---------------------------------------------------
// Automaton k's tables and candidate entries into the program P and its
// image I.  False when an inlined matcher's automaton has more than 32 sets
// (program.h kHttpInlineMasks does not hold).
bool emit_automaton(uint32_t k, const Front& fr, const Layout& lo, Tables* t, uint32_t* P, uint32_t* I) {
  const PackedDfa& d = *t->all[k].d;
  DfaDesc& dd = t->dd[k];
  const std::vector<uint32_t>& cr = t->rec.cr;
  uint16_t* I16 = reinterpret_cast<uint16_t*>(I);
  bool inline_masks = true;
  if (dd.kind == kDfaSearch) {
    const SearchDfa& sd = t->all[k].grp->sd;
    std::memcpy(P + dd.table_off, sd.table.data(), sd.table.size() * 4ull);
    std::memcpy(P + dd.es_off, sd.endmask.data(), sd.endmask.size() * 4ull);
    std::memcpy(P + dd.acc_cmap_off, sd.cmap, 256);
    if (dd.lds_table != kNone) std::memcpy(I + dd.lds_table, sd.cmap, 256);
    if (dd.lds_search != kNone) std::memcpy(I + dd.lds_search, sd.table.data(), sd.table.size() * 4ull);
    if (dd.lds_mid != kNone) std::memcpy(I + dd.lds_mid, sd.midmask.data(), sd.midmask.size() * 4ull);
    std::memcpy(P + dd.acc_mid_off, sd.midmask.data(), sd.midmask.size() * 4ull);
  } else if (dd.kind == kDfaDense) {
    const DenseDfa& D = t->dense[k];
    std::memcpy(P + dd.table_off, D.table.data(), D.table.size() * 2ull);
    std::memcpy(P + dd.es_off, D.es.data(), D.es.size() * 4ull);
    std::memcpy(P + dd.latch_off, D.latch.data(), D.latch.size() * 4ull);
    std::memcpy(P + dd.acc_cmap_off, D.cmap, 256);
    if (dd.lds_cmap != kNone) std::memcpy(I + dd.lds_cmap, D.cmap, 256);
  } else {
    std::memcpy(P + dd.table_off, d.table.data(), d.n_slots * 4ull);
    std::memcpy(P + dd.es_off, d.es.data(), d.n_slots * 4ull);
    std::memcpy(P + dd.latch_off, d.latch.data(), d.latch.size() * 4ull);
  }
  std::vector<CandEntry> ce(t->ct[k].size());
  std::memset(ce.data(), 0, ce.size() * sizeof(CandEntry));
  for (size_t i = 0; i < t->ct[k].size(); ++i) {
    const Span sp = t->ct[k][i];
    ce[i].len = sp.len;
    ce[i].off = sp.off;
    if (!sp.len) continue;
    const uint32_t nm = cr_matchers(cr[sp.off + 1]);
    const uint32_t words = 2 + 2 * std::min(nm, kCandInlineMatchers);
    std::memcpy(ce[i].rec, cr.data() + sp.off, words * 4);
    // An inlined first record: pad[q] decides inline code matcher q from
    // its automaton's set code without a mask table (bit s: set s holds the
    // matcher's pattern), exact when that automaton has <= 32 sets.
    for (uint32_t q = 0; nm <= kCandInlineMatchers && q < nm; ++q) {
      const uint32_t a = ce[i].rec[2 + 2 * q], pat = ce[i].rec[3 + 2 * q] & kPatMask;
      if ((a >> 8) & 1u) continue;  // a presence matcher
      const auto& msets = t->all[a >> 9].d->sets;
      if (msets.size() > 32) inline_masks = false;
      for (size_t s2 = 0; s2 < msets.size() && s2 < 32; ++s2)
        if (std::find(msets[s2].begin(), msets[s2].end(), pat) != msets[s2].end()) ce[i].pad[q] |= 1u << s2;
    }
    P[dd.ctmask_off + i / 32] |= 1u << (i % 32);
    if (dd.lds_ctmask != kNone) I[dd.lds_ctmask + i / 32] |= 1u << (i % 32);
  }
  if (!ce.empty()) std::memcpy(P + dd.ct_off, ce.data(), ce.size() * sizeof(CandEntry));
  if (dd.lit_tab != kNone) {
    const std::vector<uint32_t>& lw = lo.lit_words[k];
    std::memcpy(P + dd.lit_tab, lw.data(), lw.size() * 4);
    for (uint32_t l = 0; l < t->all[k].npats; ++l)
      if (lw[2 * l] != kNone) {
        const std::string& v = fr.m.fpats[t->all[k].field][t->all[k].grp->pats[l]].value;
        std::memcpy(P + lw[2 * l], v.data(), v.size());
      }
  }
  if (dd.lds_table != kNone) {
    // the LDS copy names rows by image byte address (program.h
    // kLdsRowShift), with the target state's end code when it fits 8 bits
    const uint32_t t0 = dd.lds_table;
    const bool in_entry = dd.lds_es == kLdsEsInEntry;
    auto es8 = [&d](uint32_t base) -> uint32_t { return d.es[base] == kLatchedAccept ? kEs8Latched : d.es[base]; };
    for (uint32_t s = 0; s < d.n_slots; ++s) {
      const uint32_t e = d.table[s], next = e >> 8;
      I[t0 + s] = next ? ((4 * (t0 + next)) << kLdsRowShift) | (in_entry ? es8(next) << 8 : 0u) | (e & 0xffu) : 0u;
    }
    if (in_entry && d.start_base) dd.start_es8 = es8(d.start_base);
    for (uint32_t s = 0; dd.lds_es != kNone && !in_entry && s < d.n_slots; ++s)
      I16[dd.lds_es + s] = d.es[s] == kLatchedAccept ? static_cast<uint16_t>(kEs16Latched)
                                                      : static_cast<uint16_t>(d.es[s]);
    for (size_t s = 0; dd.lds_latch != kNone && s < d.latch.size(); ++s)
      I16[dd.lds_latch + s] = d.latch[s] == kNone ? static_cast<uint16_t>(kEs16Latched)
                                                   : static_cast<uint16_t>(d.latch[s]);
  }
  if (dd.lds_ct != kNone) std::memcpy(I + dd.lds_ct, ce.data(), ce.size() * sizeof(CandEntry));
  if (dd.lds_mask != kNone) std::memcpy(I + dd.lds_mask, t->masks[k].data(), t->masks[k].size() * 8);
  return inline_masks;
}

// Field f's literal-anchored scan: the bucket table with its prefilter bits
// into the image, the AlitRecs into the image or the program.
void emit_alit(uint32_t f, const Front& fr, FieldDesc* fd, uint32_t* P, uint32_t* I) {
  const AlitField& A = fr.fa[f].alit;
  std::vector<uint32_t> gran(A.pats.size());  // pattern -> its AlitRec's granule
  uint32_t g = 0;
  for (size_t i = 0; i < A.pats.size(); ++i) {
    gran[i] = g;
    g += alit_rec_granules(A.lit[i].size());
  }
  fd->alit_granules = g;
  std::vector<uint32_t> tab = A.tab;  // {gram, pattern + 1} -> {gram, granule + 1}
  for (size_t e = 1; e < tab.size(); e += 2)
    if (tab[e]) tab[e] = gran[tab[e] - 1] + 1;
  std::memcpy(I + fd->alit_tab, tab.data(), tab.size() * 4ull);
  uint32_t* bloom = I + fd->alit_tab - kAlitBloomWords;
  for (size_t e = 0; kAlitBloomWords && e < tab.size(); e += 2)
    if (tab[e + 1]) {
      const uint32_t b = alit_bloom_bit(gram_bucket(tab[e]));
      bloom[b >> 5] |= 1u << (b & 31u);
    }
  uint32_t* base = (fd->alit_lds ? I : P) + fd->alit_pats;
  for (size_t i = 0; i < A.pats.size(); ++i) {
    const auto loc = fr.fa[f].fp_loc[A.pats[i]];  // (group, local id)
    AlitRec ar;
    ar.len_k = static_cast<uint32_t>(A.lit[i].size()) | A.k[i] << 16;
    ar.code = (fr.num.dfa_first[f] + loc.first) << 8 | loc.second;
    ar.resid = A.resid[i];
    ar.pad = 0;
    std::memcpy(base + 4 * gran[i], &ar, sizeof ar);
    std::memcpy(reinterpret_cast<uint8_t*>(base + 4 * gran[i] + 4), A.lit[i].data(), A.lit[i].size());
  }
}

void emit_dcaps(const Front& fr, const Tables& t, const Image& im, uint32_t* I) {
  for (size_t k = 0; k < fr.dcaps.size(); ++k) {
    const re::DcapForm& F = fr.dcaps[k].form;
    DcapSpec sp;
    std::memset(&sp, 0, sizeof sp);
    sp.lens = static_cast<uint32_t>(F.p1.size()) | static_cast<uint32_t>(F.l2.size()) << 16;
    sp.min = static_cast<uint32_t>(F.min);
    sp.max = F.max < 0 ? kNone : static_cast<uint32_t>(F.max);
    sp.rdfa = t.dcap_rdfa[k];
    for (int b = 0; b < 256; ++b)
      if (F.cls.test(b)) sp.cls[b >> 5] |= 1u << (b & 31);
    sp.p1 = im.dcap_p1[k];
    sp.l2 = im.dcap_l2[k];
    std::memcpy(I + im.lds_dcap + 16 * k, &sp, sizeof sp);
    std::memcpy(I + im.dcap_p1[k], F.p1.data(), F.p1.size());
    std::memcpy(I + im.dcap_l2[k], F.l2.data(), F.l2.size());
  }
}

// Every table into the program, the resident ones into its image too.  The
// descriptors go last: emit_automaton and emit_alit still write start_es8 and
// alit_granules, and the header's kHttpInlineMasks bit is known only after
// every candidate entry is filled.
std::vector<uint32_t> emit_program(const Front& fr, const Image& im, Layout* lo, Tables* t) {
  const uint32_t nf = fr.m.nf();
  HttpHeader& h = lo->h;
  std::vector<uint32_t> prog(lo->w.at, 0);
  uint32_t* P = prog.data();
  uint32_t* I = P + h.lds_image_off;
  bool inline_masks = true;  // CandEntry::pad decides every inline code matcher (program.h kHttpInlineMasks)
  for (uint32_t k = 0; k < t->ndt(); ++k) inline_masks &= emit_automaton(k, fr, *lo, t, P, I);
  // (a bit of single_entry, so single-entry programs alone carry it: the lean kernel's)
  if (inline_masks && h.single_entry) h.single_entry |= kHttpInlineMasks;
  std::memcpy(P, &h, sizeof h);
  std::memcpy(P + h.off_dfas, t->dd.data(), t->dd.size() * sizeof(DfaDesc));
  std::memcpy(I + im.lds_dfas, t->dd.data(), t->dd.size() * sizeof(DfaDesc));
  emit_dcaps(fr, *t, im, I);
  for (uint32_t f = 0; f < nf; ++f) {
    const GramFilter& gram = fr.fa[f].gram;
    if (t->fd[f].gram_tab != kNone) std::memcpy(I + t->fd[f].gram_tab, gram.tab.data(), gram.tab.size() * 4ull);
  }
  for (uint32_t f = 0; f < nf; ++f)
    if (t->fd[f].alit_tab != kNone) emit_alit(f, fr, &t->fd[f], P, I);
  std::memcpy(P + h.off_fields, t->fd.data(), t->fd.size() * sizeof(FieldDesc));
  std::memcpy(I + im.lds_fields, t->fd.data(), t->fd.size() * sizeof(FieldDesc));
  if (im.lds_name_tab != kNone) {
    for (uint32_t f = 3; f < nf; ++f) {
      const std::string& nm = fr.m.field_names[f];
      const uint32_t hk = name_hash(nm);
      uint32_t at = hk & (im.name_slots - 1);
      while (I[im.lds_name_tab + 4 * at] != 0) at = (at + 1) & (im.name_slots - 1);
      uint32_t* sl = I + im.lds_name_tab + 4 * at;
      sl[0] = hk;
      sl[1] = static_cast<uint32_t>(nm.size());
      sl[2] = f;
      sl[3] = im.name_off[f - 3];
      std::memcpy(I + im.name_off[f - 3], nm.data(), nm.size());
    }
  }
  std::memcpy(P + h.ent_tab_off, im.ent_tab.data(), im.ent_tab.size() * 4);
  if (im.lds_ent_tab != kNone) std::memcpy(I + im.lds_ent_tab, im.ent_tab.data(), im.ent_tab.size() * 4);
  if (!t->name_field.empty()) {
    std::memcpy(P + h.off_name_field, t->name_field.data(), t->name_field.size() * 4);
    std::memcpy(I + im.lds_name_field, t->name_field.data(), t->name_field.size() * 4);
  }
  std::memcpy(P + h.off_sets, t->sets.data(), t->sets.size() * sizeof(Span));
  if (fr.n) std::memcpy(P + h.off_remotes, t->rremote.data(), t->rremote.size() * sizeof(Span));
  if (!t->rec.pool.empty()) std::memcpy(P + h.off_pool, t->rec.pool.data(), t->rec.pool.size() * 4);
  if (!t->rec.cr.empty()) std::memcpy(P + h.off_cr, t->rec.cr.data(), t->rec.cr.size() * 4);
  if (fr.keys.n_slow) {
    for (uint32_t f = 0; f < nf; ++f)
      for (size_t pi = 0; pi < fr.m.fpats[f].size(); ++pi)
        if (lo->slow_off[f][pi] != kNone)
          std::memcpy(P + lo->slow_off[f][pi], fr.fa[f].slow_vm[pi].data(), fr.fa[f].slow_vm[pi].size() * 4);
    std::memcpy(P + h.off_slow, lo->slow_span.data(), lo->slow_span.size() * sizeof(Span));
  }
  return prog;
}

CompileResult failed(const Err& e) {
  CompileResult res;
  res.status = e.status;
  res.err = e.msg;
  return res;
}

}  // namespace

CompileResult compile_http_core(const l7m_http_rule* rules, size_t n, const PolicyPlan& plan, const l7m_opts& opts,
                                uint64_t no_alit, uint32_t* alit_over) {
  Front fr;
  fr.n = n;
  fr.re2 = opts.dialect == L7M_DIALECT_RE2_SEARCH;
  if (n > 0 && !rules) return failed(fail(L7M_EINVAL, "rules == NULL"));
  if (opts.dialect != L7M_DIALECT_ENVOY_ECMA_FULL && !fr.re2) return failed(fail(L7M_EINVAL, "unknown dialect"));
  if (n >= kNone / 2) return failed(fail(L7M_ETOOBIG, "too many rules"));

  Err e = match_rules(rules, n, &fr.m);
  if (!e.ok()) return failed(e);
  const uint32_t nf = fr.m.nf();
  FieldDfaLimits lim;
  if (opts.max_dfa_states) lim.max_multi_states = opts.max_dfa_states;
  if (opts.max_table_bytes) lim.max_slots = std::min<uint64_t>(lim.max_slots, opts.max_table_bytes / 4);
  fr.fa.resize(nf);
  for (uint32_t f = 0; f < nf; ++f) {
    if (fr.m.fpats[f].empty()) continue;
    e = build_field_automata(f, fr.m.field_names[f], fr.m.fpats[f], fr.re2, lim, f < 64 && (no_alit >> f & 1),
                             &fr.fa[f], &fr.dcaps);
    if (!e.ok()) return failed(e);
  }
  if (!(e = number_automata(fr.m, fr.fa, &fr.num)).ok()) return failed(e);
  if (!(e = key_rules(rules, n, plan, fr.m, fr.fa, fr.num, &fr.keys)).ok()) return failed(e);

  Tables t;
  Image im;
  Layout lo;
  if (!(e = build_records(fr, plan, &t)).ok()) return failed(e);
  if (!(e = place_fixed(fr, opts, t, &im)).ok()) return failed(e);
  if (!(e = place_scan_tables(fr, &t, &im, alit_over)).ok()) return failed(e);
  place_automata(fr, plan, &t, &im);
  convert_dense(fr, opts, &t, &im);
  lo.h = header_fields(fr, plan, t, im);
  if (!(e = lay_out(fr, im, &t, &lo)).ok()) return failed(e);

  CompileResult res;
  res.program = emit_program(fr, im, &lo, &t);
  res.info.proto = L7M_PROTO_HTTP;
  res.info.n_rules = static_cast<uint32_t>(n);
  res.info.n_fields = nf;
  res.info.n_dfas = t.ndt();
  res.info.total_dfa_states = t.total_states;
  res.info.program_bytes = lo.w.at * 4;
  res.info.n_counters = static_cast<uint32_t>(n) + 2;
  res.info.n_dense_dfas = t.n_dense;
  return res;
}

}  // namespace l7m

