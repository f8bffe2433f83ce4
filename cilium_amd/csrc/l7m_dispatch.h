// l7m_dispatch.h -- a runtime value from a fixed list as a template argument
// (host code only): the launchers pick a kernel instantiation with it.
#pragma once
#include <type_traits>
#include <utility>

namespace l7m {

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
