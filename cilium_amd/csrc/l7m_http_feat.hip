// l7m_http_feat.hip -- the ECMAScript first-pass (http_eval_kernel) and
// slow-pass (http_slow_kernel) instantiations of the feature sets kFeat =
// L7M_FEAT (l7m_http_impl.h kFeatLit / kFeatDcap) and L7M_FEAT | kFeatDense
// (the same set for programs with dense automata).  Compiled once per
// L7M_FEAT (Makefile: build/l7m_http_f<F>.o), so the instantiations build in
// parallel; l7m_kernels.hip launch_http picks the set a program needs.
#include "l7m_dispatch.h"
#include "l7m_http_impl.h"

#if !defined(L7M_FEAT) || !defined(L7M_FEAT_DENSE)
#error "L7M_FEAT (0..3) selects the feature set, L7M_FEAT_DENSE (= L7M_FEAT + 4) its dense twin"
#endif

namespace l7m {

static_assert(L7M_FEAT_DENSE == (L7M_FEAT | kFeatDense) && L7M_FEAT < kFeatDense, "feature set numbering");

// First pass of feature set F: hit mode x end-code registers R (4, 8, 0 = LDS
// columns).  Any other mode counts in global memory, any other R uses columns.
// lean: the program is of the lean class (l7m_dispatch.h http_program_lean),
// whose kernels exist for the plain feature set with R = 4 only; any other
// combination is an error, never another kernel.
template <int F>
hipError_t launch_http_main(const LaunchPlan& p, const BatchRef& b, int mode, int R, bool lean, uint32_t* slowq,
                            DoneSignal done) {
  mode = mode == kNoHits || mode == kLdsHits ? mode : kGlobalHits;
  R = R == 4 || R == 8 ? R : 0;
  if (lean) {
    if constexpr (F == 0) {
      if (R != 4) return hipErrorInvalidValue;
      return dispatch_values<int, kNoHits, kLdsHits, kGlobalHits>(mode, hipErrorInvalidValue, [&](auto M) {
        return launch_one<decltype(M)::value, 4, 0, kFeatLean>(p, b, nullptr, slowq, done);
      });
    } else {
      return hipErrorInvalidValue;
    }
  }
  return dispatch_values<int, kNoHits, kLdsHits, kGlobalHits>(mode, hipErrorInvalidValue, [&](auto M) {
    return dispatch_values<int, 4, 8, 0>(R, hipErrorInvalidValue, [&](auto RR) {
      return launch_one<decltype(M)::value, decltype(RR)::value, 0, F>(p, b, nullptr, slowq, done);
    });
  });
}

// Slow pass of feature set F: R x tier (any tier but 1 is the second).
template <int F>
hipError_t launch_http_slow(const LaunchPlan& p, const HttpHeader& h, const BatchRef& b, const HttpSlowPass& s, int R,
                            int tier) {
  R = R == 4 || R == 8 ? R : 0;
  tier = tier == 1 ? 1 : 2;
  return dispatch_values<int, 4, 8, 0>(R, hipErrorInvalidValue, [&](auto RR) {
    return dispatch_values<int, 1, 2>(tier, hipErrorInvalidValue, [&](auto T) {
      return launch_slow<decltype(RR)::value, F, decltype(T)::value>(p, h, b, s);
    });
  });
}

// The two launch entry points of this unit's two feature sets.  The order of
// these lines is the order the kernels are laid out in the unit's code object,
// which cilium_amd/codehash.py kernel_md5 depends on: keep it.
template hipError_t launch_http_main<L7M_FEAT>(const LaunchPlan&, const BatchRef&, int, int, bool, uint32_t*, DoneSignal);
template hipError_t launch_http_slow<L7M_FEAT>(const LaunchPlan&, const HttpHeader&, const BatchRef&,
                                               const HttpSlowPass&, int, int);
template hipError_t launch_http_main<L7M_FEAT_DENSE>(const LaunchPlan&, const BatchRef&, int, int, bool, uint32_t*,
                                                     DoneSignal);
template hipError_t launch_http_slow<L7M_FEAT_DENSE>(const LaunchPlan&, const HttpHeader&, const BatchRef&,
                                                     const HttpSlowPass&, int, int);

}  // namespace l7m
