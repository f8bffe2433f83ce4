// Differential fuzzer of the dense class-compressed automaton (dfa_pack.h
// DenseDfa, program.h kDfaDense): for random pattern sets -- literal prefixes,
// shared tails, `.*x.{k}` blow-ups, single-pattern sets (latched start) --
// build_field_dfa, then build_dense, and on random and pattern-derived
// subjects (the empty string, NUL and bytes >= 0x80 included) the dense walk's
// end code must equal the packed walk's.  The tables' invariants (state 0 an
// all-zero row, targets below nstates, multi-pattern states first) are checked
// too.  Built with -fsanitize=address,undefined.  Test infrastructure only.
//   fuzz_dense <seed> <n_sets> <subjects_per_set>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../cilium_amd/csrc/dfa_pack.h"
#include "../../cilium_amd/csrc/regex_ecma.h"

using namespace l7m;
static std::mt19937_64 rng;
static int rnd(int n) { return (int)(rng() % (uint64_t)n); }
template <class T, size_t N>
static const T& pick(const T (&a)[N]) { return a[rnd((int)N)]; }

static const char* kTails[] = {"", "/v[0-9]+/(users|orders|items)/[0-9]+", "/.*", "[a-c]*", "\\.ns\\.local",
                               "(/\\w+)*", "/[^/]+/x", "\\d{1,3}", "(x|yz)+", "/?"};
static const char* kFree[] = {".*", "[a-z]+", "\\w*", "/(a|b)*", "[^/]*", "(?!/admin).*", ".*\\bv1\\b.*", "[\\x80-\\xff]+",
                              "\\x00*a", ".*\\.(txt|json)"};

static std::string rand_lit(int n) {
  static const char al[] = "abcxyz/01-._";
  std::string s;
  for (int i = 0; i < n; ++i) s.push_back(al[rnd((int)sizeof(al) - 1)]);
  std::string out;  // escaped for the regex parser
  for (char c : s) {
    if (c == '.' || c == '/' || c == '-') out.push_back('\\');
    out.push_back(c);
  }
  return out;
}

static std::vector<std::string> pattern_set() {
  std::vector<std::string> pats;
  const int shape = rnd(5);
  const int n = shape == 4 ? 1 : 1 + rnd(shape == 1 ? 40 : 8);
  const std::string shared = pick(kTails);
  for (int i = 0; i < n; ++i) {
    switch (shape) {
      case 0:  // literal prefixes, mixed tails
        pats.push_back("\\/" + rand_lit(1 + rnd(6)) + pick(kTails));
        break;
      case 1:  // many prefixes, one shared tail (config 2's shape)
        pats.push_back("\\/svc" + std::to_string(i) + shared);
        break;
      case 2:  // .*x.{k}: 2^k states
        pats.push_back(std::string(".*") + "xab"[rnd(3)] + ".{" + std::to_string(rnd(7)) + "}");
        break;
      case 3:  // no literal prefix
        pats.push_back(std::string(pick(kFree)) + (rnd(2) ? rand_lit(rnd(3)) : ""));
        break;
      default:  // one pattern: the start state is latched
        pats.push_back(rnd(2) ? "\\/" + rand_lit(rnd(5)) + pick(kTails) : std::string(pick(kFree)));
    }
  }
  return pats;
}

static std::string unescape(const std::string& p) {
  std::string s;
  for (size_t i = 0; i < p.size(); ++i) {
    const char c = p[i];
    if (c == '\\' && i + 1 < p.size()) { s.push_back(p[++i] == 'd' ? '7' : p[i] == 'w' ? 'q' : p[i]); continue; }
    if (c == '(' || c == ')' || c == '|' || c == '[' || c == ']' || c == '{' || c == '}' || c == '?' || c == '^') continue;
    if (c == '*' || c == '+') { if (!s.empty() && rnd(2)) s.push_back(s.back()); continue; }
    s.push_back(c == '.' ? "ax/\x80"[rnd(4)] : c);
  }
  return s;
}

static std::string subject(const std::vector<std::string>& pats) {
  std::string s;
  switch (rnd(6)) {
    case 0: return s;  // empty
    case 1:            // random bytes over the whole range
      for (int i = rnd(24); i > 0; --i) s.push_back((char)rnd(256));
      return s;
    case 2:  // small alphabet with NUL and high bytes
      for (int i = rnd(20); i > 0; --i) s.push_back("ab/x1.\x00\x80\xff-"[rnd(10)]);
      return s;
    default: {  // derived from a pattern, then perturbed
      s = unescape(pats[rnd((int)pats.size())]);
      const int k = rnd(4);
      if (k == 0 && !s.empty()) s[rnd((int)s.size())] = (char)rnd(256);
      if (k == 1) s = s.substr(0, rnd((int)s.size() + 1));
      if (k == 2) s += "/v12/users/345";
      return s;
    }
  }
}

int main(int argc, char** argv) {
  rng.seed(argc > 1 ? strtoull(argv[1], 0, 10) : 1);
  const int nsets = argc > 2 ? atoi(argv[2]) : 300;
  const int nstr = argc > 3 ? atoi(argv[3]) : 300;
  long built = 0, checked = 0, matched = 0, latched_start = 0, multi = 0, mism = 0;
  for (int i = 0; i < nsets; ++i) {
    const std::vector<std::string> pats = pattern_set();
    std::vector<re::Ast> asts;
    bool ok = true;
    for (const auto& p : pats) {
      re::Ast full;
      std::string err;
      if (re::parse_ecma(p, &full, &err) != re::Status::Ok) { ok = false; break; }
      bool exact = true;
      asts.push_back(re::lower_for_dfa(full, &exact));
    }
    if (!ok) continue;
    std::vector<const re::Ast*> ptr;
    for (const auto& a : asts) ptr.push_back(&a);
    PackedDfa pk;
    FieldDfaLimits lim;
    if (build_field_dfa(ptr, lim, &pk) != re::Status::Ok) continue;
    DenseDfa dn;
    if (!build_dense(pk, &dn)) continue;
    ++built;
    latched_start += pk.start_latch != 0xffffffffu;
    multi += dn.region > 1;
    // table invariants
    bool inv = dn.nstates <= kDenseMaxStates && dn.ncls >= 1 && dn.ncls <= 256 && dn.region >= 1 &&
               dn.region <= dn.nstates && dn.start_state < dn.nstates &&
               dn.table.size() == (size_t)dn.nstates * dn.ncls && dn.es.size() == dn.nstates &&
               dn.latch.size() == (size_t)dn.region * dn.ncls && dn.es[0] == 0;
    for (uint32_t c = 0; inv && c < dn.ncls; ++c) inv = dn.table[c] == 0;
    for (size_t k = 0; inv && k < dn.table.size(); ++k) inv = dn.table[k] < dn.nstates;
    for (int b = 0; inv && b < 256; ++b) inv = dn.cmap[b] < dn.ncls;
    if (!inv) {
      ++mism;
      printf("INVARIANT set %d (%s ...)\n", i, pats[0].c_str());
      continue;
    }
    for (int j = 0; j < nstr; ++j) {
      const std::string s = subject(pats);
      const uint32_t a = packed_walk(pk, reinterpret_cast<const uint8_t*>(s.data()), s.size());
      const uint32_t b = dense_walk(dn, reinterpret_cast<const uint8_t*>(s.data()), s.size());
      ++checked;
      matched += a != 0;
      if (a != b) {
        ++mism;
        if (mism < 20) {
          printf("MISMATCH set %d pat0=%s packed=%08x dense=%08x in=", i, pats[0].c_str(), a, b);
          for (unsigned char c : s) printf("%02x", c);
          printf("\n");
        }
      }
    }
  }
  printf("built=%ld checked=%ld matched=%ld latched_start=%ld multi=%ld mismatches=%ld\n", built, checked, matched,
         latched_start, multi, mism);
  return mism || !built || !matched || !latched_start || !multi ? 1 : 0;
}
