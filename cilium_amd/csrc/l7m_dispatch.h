// l7m_dispatch.h -- a runtime value from a fixed list as a template argument
// (host code only): the launchers pick a kernel instantiation with it.
#pragma once
#include <type_traits>
#include <utility>

#include "program.h"

namespace l7m {

// Whether an HTTP program belongs to the "lean" class, whose first pass runs
// the lean instantiation of http_eval_kernel (l7m_http_impl.h kFeatLean): a
// single-entry program, decided in one launch, whose <= 4 value automata are
// all walked from LDS with the end code in the table entry.  Every clause is a
// compile-time constant of that instantiation, so a program outside the class
// must never reach it.  dd: the program's DfaDesc[n_dfas + has_name_dfa],
// fd: its FieldDesc[n_fields].
inline bool http_program_lean(const HttpHeader& h, const DfaDesc* dd, const FieldDesc* fd) {
  if (!h.single_entry || h.allow_no_l7) return false;  // the port-entry table is never probed
  if (h.search) return false;                          // ECMAScript dialect only
  if (h.lds_dcap != kNone) return false;               // no forced captures
  if (h.n_slow != 0) return false;                     // no slow-path rules
  if (h.n_dfas > 4) return false;                      // end codes in four registers
  for (uint32_t k = 0; k < h.n_dfas; ++k) {
    if (dd[k].kind != kDfaPacked || dd[k].lit_tab != kNone) return false;  // no dense automata, no literal tables
    if (dd[k].lds_table == kNone || dd[k].lds_es != kLdsEsInEntry || dd[k].lds_skip != kNone) return false;
  }
  if (h.has_name_dfa && h.lds_name_tab == kNone) return false;  // header names by the LDS name table
  // ... which the lean kernel probes for every name length the masks admit: without a table, none
  if (h.lds_name_tab == kNone && (h.name_len_lo | h.name_len_hi) != 0) return false;
  if (h.n_fields < 3) return false;
  for (uint32_t f = 0; f < 3; ++f)  // method, path, authority: one automaton each
    if (fd[f].ndfa != 1 || fd[f].dfa_first >= h.n_dfas) return false;
  return true;
}

// f(std::integral_constant<T, V>{}) for the first V of Vs equal to v; its
// result, or `fallback` (f not called) when v is none of them.  Nests:
//   dispatch_values<int, 0, 1, 2>(mode, err, [&](auto M) {
//     return dispatch_values<bool, false, true>(flag, err, [&](auto B) {
//       return launch<decltype(M)::value, decltype(B)::value>(...);
//     });
//   });
template <class T, T... Vs, class R, class F>
R dispatch_values(T v, R fallback, F&& f) {
  R r = std::move(fallback);
  (void)((v == Vs ? (r = f(std::integral_constant<T, Vs>{}), true) : false) || ...);
  return r;
}

}  // namespace l7m
