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
#define L7M_CAT2(a, b) a##b
#define L7M_CAT(a, b) L7M_CAT2(a, b)

namespace l7m {

static_assert(L7M_FEAT_DENSE == (L7M_FEAT | kFeatDense) && L7M_FEAT < kFeatDense, "feature set numbering");

namespace {

// First pass of feature set F: hit mode x end-code registers R (4, 8, 0 = LDS
// columns).  Any other mode counts in global memory, any other R uses columns.
// lean: the program is of the lean class (l7m_dispatch.h http_program_lean),
// whose kernels exist for the plain feature set with R = 4 only; any other
// combination is an error, never another kernel.
template <int F>
hipError_t http_main(int mode, int R, bool lean, dim3 grid, size_t lds, hipStream_t stream, const uint32_t* dprog,
                     const uint8_t* arena, uint64_t arena_bytes, const uint64_t* offs, uint64_t n, int32_t* verdicts,
                     unsigned long long* hits, uint32_t stage, uint32_t* slowq, DoneSignal done) {
  mode = mode == kNoHits || mode == kLdsHits ? mode : kGlobalHits;
  R = R == 4 || R == 8 ? R : 0;
  if (lean) {
    if constexpr (F == 0) {
      if (R != 4) return hipErrorInvalidValue;
      return dispatch_values<int, kNoHits, kLdsHits, kGlobalHits>(mode, hipErrorInvalidValue, [&](auto M) {
        return launch_one<decltype(M)::value, 4, 0, kFeatLean>(grid, lds, stream, dprog, arena, arena_bytes, offs, n,
                                                                verdicts, hits, stage, nullptr, slowq, done);
      });
    } else {
      return hipErrorInvalidValue;
    }
  }
  return dispatch_values<int, kNoHits, kLdsHits, kGlobalHits>(mode, hipErrorInvalidValue, [&](auto M) {
    return dispatch_values<int, 4, 8, 0>(R, hipErrorInvalidValue, [&](auto RR) {
      return launch_one<decltype(M)::value, decltype(RR)::value, 0, F>(
          grid, lds, stream, dprog, arena, arena_bytes, offs, n, verdicts, hits, stage, nullptr, slowq, done);
    });
  });
}

// Slow pass of feature set F: R x tier (any tier but 1 is the second).
template <int F>
hipError_t http_slow(int R, int tier, const HttpHeader& h, uint32_t blocks, hipStream_t stream, const uint32_t* dprog,
                     const uint8_t* arena, uint64_t arena_bytes, const uint64_t* offs, uint64_t n, int32_t* verdicts,
                     unsigned long long* hits, const uint32_t* slowq, uint32_t* slowq2, uint32_t* vmscratch,
                     uint32_t* work) {
  R = R == 4 || R == 8 ? R : 0;
  tier = tier == 1 ? 1 : 2;
  return dispatch_values<int, 4, 8, 0>(R, hipErrorInvalidValue, [&](auto RR) {
    return dispatch_values<int, 1, 2>(tier, hipErrorInvalidValue, [&](auto T) {
      return launch_slow<decltype(RR)::value, F, decltype(T)::value>(h, blocks, stream, dprog, arena, arena_bytes, offs,
                                                                     n, verdicts, hits, slowq, slowq2, vmscratch, work);
    });
  });
}

}  // namespace

// The two launch entry points of feature set F.
#define L7M_FEAT_DEFS(F)                                                                                         \
  hipError_t L7M_CAT(launch_http_main_f, F)(int mode, int R, bool lean, dim3 grid, size_t lds, hipStream_t stream, \
                                            const uint32_t* dprog, const uint8_t* arena, uint64_t arena_bytes,  \
                                            const uint64_t* offs, uint64_t n, int32_t* verdicts,                \
                                            unsigned long long* hits, uint32_t stage, uint32_t* slowq,          \
                                            DoneSignal done) {                                                   \
    return http_main<F>(mode, R, lean, grid, lds, stream, dprog, arena, arena_bytes, offs, n, verdicts, hits,    \
                        stage, slowq, done);                                                                     \
  }                                                                                                              \
  hipError_t L7M_CAT(launch_http_slow_f, F)(int R, int tier, const HttpHeader& h, uint32_t blocks,              \
                                            hipStream_t stream, const uint32_t* dprog, const uint8_t* arena,    \
                                            uint64_t arena_bytes, const uint64_t* offs, uint64_t n,             \
                                            int32_t* verdicts, unsigned long long* hits, const uint32_t* slowq, \
                                            uint32_t* slowq2, uint32_t* vmscratch, uint32_t* work) {            \
    return http_slow<F>(R, tier, h, blocks, stream, dprog, arena, arena_bytes, offs, n, verdicts, hits, slowq,  \
                        slowq2, vmscratch, work);                                                                \
  }

L7M_FEAT_DEFS(L7M_FEAT)
L7M_FEAT_DEFS(L7M_FEAT_DENSE)

#undef L7M_FEAT_DEFS

}  // namespace l7m
