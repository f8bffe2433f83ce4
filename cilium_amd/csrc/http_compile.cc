// http_compile.cc — compile []PortRuleHTTP into the HTTP device program.
//
// Pipeline (cold path, once per policy revision):
//   1. getHTTPRule (pkg/envoy/server.go:261-320): PortRuleHTTP -> HeaderMatcher
//      list, sorted by SortHeaderMatchers (pkg/envoy/sort.go:205-250).  Equal
//      (Name, Value) pairs involving a header matcher make Go dereference a nil
//      Regex and panic (sort.go:225-228); we return L7M_EINVAL_RULE instead.
//   2. Envoy HeaderData (envoy/cilium_network_policy.h:52-66 -> upstream
//      ConfigUtility::HeaderData): name lower-cased; empty value -> Present,
//      regex flag -> Regex (std::regex(value, optimize): throws -> NACK, here
//      L7M_EINVAL_REGEX), else exact Value.
//   3. Fields: ":method", ":path", ":authority", then every other header name
//      a rule references.  Per field, the distinct Regex/Value patterns are
//      determinised together into DFA groups (split when a group exceeds the
//      state/table limits); a header-name DFA maps request header names to
//      field ids.
//   4. First-match index: every rule is "keyed" on its most selective matcher.
//      For each (DFA, end set) the sorted list of rules keyed on a pattern of
//      that set is precomputed; at run time the kernel scans those lists in
//      rule order and verifies the rule's remaining matchers (AND), giving the
//      smallest matching rule index = HttpNetworkPolicyRule OR semantics
//      (envoy/cilium_network_policy.h:98-105) with a deterministic index.
//
// This unit is the front end: the translation (1), the flattening of a
// NetworkPolicyMap into rules and a port-entry plan, and the retry without a
// field's literal-anchored scan.  Steps 2-4 and the program's layout are the
// phases of http_phases.cc (compile_http_core, http_phases.h).
#include <algorithm>

#include "http_phases.h"
#include "l7m_internal.h"
#include "program.h"

namespace l7m {
namespace {

std::string cstr(const char* p) { return p ? std::string(p) : std::string(); }

// Go strings.SplitN(s, " ", 2)
std::vector<std::string> split2(const std::string& s) {
  size_t k = s.find(' ');
  if (k == std::string::npos) return {s};
  return {s.substr(0, k), s.substr(k + 1)};
}

// Go strings.TrimRight(s, ":")
std::string trim_right_colon(std::string s) {
  while (!s.empty() && s.back() == ':') s.pop_back();
  return s;
}

// HeaderMatcherLess (pkg/envoy/sort.go:209-233) without the nil dereference;
// the caller rejects the inputs where Go would panic.
bool matcher_less(const HeaderMatcher& a, const HeaderMatcher& b) {
  if (a.name != b.name) return a.name < b.name;
  if (a.value != b.value) return a.value < b.value;
  bool ar = a.has_regex && a.regex, br = b.has_regex && b.regex;
  return !ar && br;
}

}  // namespace

std::string lower_ascii(const std::string& s) {
  std::string r = s;
  for (auto& c : r)
    if (c >= 'A' && c <= 'Z') c = static_cast<char>(c - 'A' + 'a');
  return r;
}

MatchKind envoy_kind(const HeaderMatcher& m) {
  if (m.value.empty()) return MatchKind::Present;
  if (m.has_regex && m.regex) return MatchKind::Regex;
  return MatchKind::Value;
}

int translate_http_rule(const l7m_http_rule& r, std::vector<HeaderMatcher>* out, std::string* err) {
  out->clear();
  std::string path = cstr(r.path), method = cstr(r.method), host = cstr(r.host);
  if (!path.empty()) out->push_back({":path", path, true, true});
  if (!method.empty()) out->push_back({":method", method, true, true});
  if (!host.empty()) out->push_back({":authority", host, true, true});
  for (uint32_t j = 0; j < r.n_headers; ++j) {
    if (!r.headers) {
      *err = "headers == NULL with n_headers > 0";
      return L7M_EINVAL;
    }
    auto parts = split2(cstr(r.headers[j]));
    if (parts.size() == 2) out->push_back({trim_right_colon(parts[0]), parts[1], false, false});
    else out->push_back({parts[0], "", false, false});
  }
  // SortHeaderMatchers panics on equal (Name, Value) with a nil Regex.
  for (size_t a = 0; a < out->size(); ++a)
    for (size_t b = a + 1; b < out->size(); ++b) {
      const auto& x = (*out)[a];
      const auto& y = (*out)[b];
      if (x.name == y.name && x.value == y.value && !(x.has_regex && y.has_regex)) {
        *err = "duplicate header matcher '" + x.name + "' (getHTTPRule sort would panic, "
               "pkg/envoy/sort.go:225-228)";
        return L7M_EINVAL_RULE;
      }
    }
  std::stable_sort(out->begin(), out->end(), matcher_less);
  for (const auto& m : *out)
    if (m.name.empty()) {
      // Envoy's HeaderMatcher.name validation (min_bytes 1) rejects the policy.
      *err = "empty header name";
      return L7M_EINVAL_RULE;
    }
  return L7M_OK;
}

namespace {

// compile_http_core, and again without the literal-anchored scan of each
// field whose bucket table did not fit the LDS budget (at most once per field).
CompileResult compile_http_alit_fallback(const l7m_http_rule* rules, size_t n, const PolicyPlan& plan,
                                         const l7m_opts& opts) {
  uint64_t no_alit = 0;
  for (;;) {
    uint32_t over = kNone;
    CompileResult r = compile_http_core(rules, n, plan, opts, no_alit, &over);
    if (r.status != L7M_ETOOBIG || over == kNone || over >= 64 || (no_alit >> over & 1)) return r;
    no_alit |= 1ull << over;
  }
}

}  // namespace

CompileResult compile_http(const l7m_http_rule* rules, size_t n, const l7m_opts& opts) {
  // one policy whose every port and direction use `rules`
  PolicyPlan plan;
  plan.single = true;
  plan.n_policies = 1;
  plan.rule_entry.assign(n, 0);
  plan.entry_have_http = {static_cast<uint8_t>(n > 0 ? 1 : 0)};
  plan.names = {""};
  plan.origin.resize(n);
  for (size_t i = 0; i < n; ++i) plan.origin[i] = {0, 1, 0, 0, static_cast<int32_t>(i), 0};
  CompileResult r = compile_http_alit_fallback(rules, n, plan, opts);
  r.names = std::move(plan.names);
  r.origin = std::move(plan.origin);
  return r;
}

// NetworkPolicyMap construction (envoy/cilium_network_policy.h:40-208,
// .cc:42-108) flattened for the kernel: every HTTP rule (or matcher-less
// pseudo rule of a port rule without http_rules) gets an index in the order
// l7m_rule_origin documents and the port entry it belongs to; the
// (policy, direction, port) -> entry table drives the exact-port / port-0 /
// no-entry selection of PortNetworkPolicy::Matches (h:169-192).
CompileResult compile_http_policies(const l7m_network_policy* pols, size_t npol, const l7m_opts& opts) {
  CompileResult bad;
  auto fail = [&](int st, const std::string& m) {
    bad.status = st;
    bad.err = m;
    return bad;
  };
  if (npol > 0 && !pols) return fail(L7M_EINVAL, "policies == NULL");
  if (npol >= L7M_POLICY_UNKNOWN) return fail(L7M_ETOOBIG, "more than 65534 endpoint policies");
  PolicyPlan plan;
  plan.single = false;
  plan.n_policies = static_cast<uint32_t>(npol);
  std::vector<l7m_http_rule> flat;
  std::vector<std::vector<uint32_t>> flat_remotes;  // owned copies
  std::vector<std::string> seen_names;
  for (size_t pi = 0; pi < npol; ++pi) {
    const l7m_network_policy& P = pols[pi];
    const std::string name = P.name ? P.name : "";
    if (std::find(plan.names.begin(), plan.names.end(), name) != plan.names.end())
      return fail(L7M_EINVAL_RULE, "duplicate endpoint policy name '" + name + "'");
    plan.names.push_back(name);
    for (uint32_t dir = 0; dir < 2; ++dir) {
      const uint32_t ingress = dir == 0 ? 1u : 0u;  // ingress, then egress
      const l7m_port_policy* pp = ingress ? P.ingress : P.egress;
      const size_t npp = ingress ? P.n_ingress : P.n_egress;
      if (npp && !pp) return fail(L7M_EINVAL, "port policies == NULL");
      // port entries in input order, the port-0 entry last
      std::vector<size_t> order;
      std::vector<uint32_t> ports_seen;
      for (size_t k = 0; k < npp; ++k) {
        if (pp[k].port > 65535) return fail(L7M_EINVAL_RULE, "port > 65535");
        if (pp[k].protocol != L7M_L4_TCP) continue;  // "NOT installing non-TCP policy" (h:163-165)
        if (std::find(ports_seen.begin(), ports_seen.end(), pp[k].port) != ports_seen.end())
          return fail(L7M_EINVAL_RULE, "PortNetworkPolicy: Duplicate port number " + std::to_string(pp[k].port));
        ports_seen.push_back(pp[k].port);
        if (pp[k].port != 0) order.push_back(k);
      }
      for (size_t k = 0; k < npp; ++k)
        if (pp[k].port == 0 && pp[k].protocol == L7M_L4_TCP) order.push_back(k);
      for (size_t k : order) {
        const l7m_port_policy& E = pp[k];
        if (E.n_rules && !E.rules) return fail(L7M_EINVAL, "port rules == NULL");
        const uint32_t entry = static_cast<uint32_t>(plan.entry_have_http.size());
        if (entry >= kCrMaxEntries) return fail(L7M_ETOOBIG, "too many port entries");
        bool have_http = false;
        for (size_t r = 0; r < E.n_rules; ++r) {
          const l7m_port_rule& R = E.rules[r];
          if (R.n_remote_ids && !R.remote_ids) return fail(L7M_EINVAL, "remote_ids == NULL");
          std::vector<uint32_t> rem(R.remote_ids, R.remote_ids + R.n_remote_ids);
          if (R.has_http_rules) {
            have_http = true;
            if (R.n_http_rules == 0 || !R.http_rules)
              return fail(L7M_EINVAL_RULE, "http_rules present but empty (HttpNetworkPolicyRules min_items = 1)");
            for (size_t j = 0; j < R.n_http_rules; ++j) {
              if (R.http_rules[j].n_remote_ids)
                return fail(L7M_EINVAL, "remote ids belong to the port rule, not to its http rules");
              flat.push_back(R.http_rules[j]);
              flat_remotes.push_back(rem);
              plan.rule_entry.push_back(entry);
              plan.origin.push_back({static_cast<uint32_t>(pi), ingress, E.port, static_cast<uint32_t>(r),
                                     static_cast<int32_t>(j), 0});
            }
          } else {
            flat.push_back(l7m_http_rule{});  // no L7 predicate: any request
            flat_remotes.push_back(rem);
            plan.rule_entry.push_back(entry);
            plan.origin.push_back({static_cast<uint32_t>(pi), ingress, E.port, static_cast<uint32_t>(r), -1, 0});
          }
        }
        plan.entry_have_http.push_back(have_http ? 1 : 0);
        plan.keys.emplace_back(ent_key(static_cast<uint32_t>(pi), ingress, E.port), entry);
      }
    }
  }
  for (size_t i = 0; i < flat.size(); ++i) {
    flat[i].remote_ids = flat_remotes[i].data();
    flat[i].n_remote_ids = static_cast<uint32_t>(flat_remotes[i].size());
  }
  CompileResult r = compile_http_alit_fallback(flat.data(), flat.size(), plan, opts);
  r.names = std::move(plan.names);
  r.origin = std::move(plan.origin);
  return r;
}

}  // namespace l7m
