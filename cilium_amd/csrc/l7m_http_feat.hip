// l7m_http_feat.hip -- the ECMAScript first-pass (http_eval_kernel) and
// slow-pass (http_slow_kernel) instantiations of the feature sets kFeat =
// L7M_FEAT (l7m_http_impl.h kFeatLit / kFeatDcap) and L7M_FEAT | kFeatDense
// (the same set for programs with dense automata).  Compiled once per
// L7M_FEAT (Makefile: build/l7m_http_f<F>.o), so the instantiations build in
// parallel; l7m_kernels.hip launch_http picks the set a program needs.
#include "l7m_http_impl.h"

#if !defined(L7M_FEAT) || !defined(L7M_FEAT_DENSE)
#error "L7M_FEAT (0..3) selects the feature set, L7M_FEAT_DENSE (= L7M_FEAT + 4) its dense twin"
#endif
#define L7M_CAT2(a, b) a##b
#define L7M_CAT(a, b) L7M_CAT2(a, b)

namespace l7m {

static_assert(L7M_FEAT_DENSE == (L7M_FEAT | kFeatDense) && L7M_FEAT < kFeatDense, "feature set numbering");

#define L7M_ONE(M, RR, F)                                                                              \
  return launch_one<M, RR, 0, F>(grid, lds, stream, dprog, arena, arena_bytes, offs, n, verdicts, hits, \
                                 stage, nullptr, slowq, done, hslice)
#define L7M_MODES(RR, F)                            \
  {                                                 \
    if (mode == kNoHits) L7M_ONE(kNoHits, RR, F);   \
    if (mode == kLdsHits) L7M_ONE(kLdsHits, RR, F); \
    L7M_ONE(kGlobalHits, RR, F);                    \
  }
#define L7M_SLOW(RR, T, F)                                                                                \
  return launch_slow<RR, F, T>(h, blocks, stream, dprog, arena, arena_bytes, offs, n, verdicts, hits, slowq, \
                               slowq2, vmscratch, work)

// The two launch entry points of feature set F.
#define L7M_FEAT_DEFS(F)                                                                                         \
  hipError_t L7M_CAT(launch_http_main_f, F)(int mode, int R, dim3 grid, size_t lds, hipStream_t stream,         \
                                            const uint32_t* dprog, const uint8_t* arena, uint64_t arena_bytes,  \
                                            const uint64_t* offs, uint64_t n, int32_t* verdicts,                \
                                            unsigned long long* hits, uint32_t stage, uint32_t* slowq,          \
                                            DoneSignal done, uint32_t* hslice) {                                 \
    if (R == 4) L7M_MODES(4, F)                                                                                  \
    if (R == 8) L7M_MODES(8, F)                                                                                  \
    L7M_MODES(0, F)                                                                                              \
  }                                                                                                              \
  hipError_t L7M_CAT(launch_http_slow_f, F)(int R, int tier, const HttpHeader& h, uint32_t blocks,              \
                                            hipStream_t stream, const uint32_t* dprog, const uint8_t* arena,    \
                                            uint64_t arena_bytes, const uint64_t* offs, uint64_t n,             \
                                            int32_t* verdicts, unsigned long long* hits, const uint32_t* slowq, \
                                            uint32_t* slowq2, uint32_t* vmscratch, uint32_t* work) {            \
    if (tier == 1) {                                                                                             \
      if (R == 4) L7M_SLOW(4, 1, F);                                                                             \
      if (R == 8) L7M_SLOW(8, 1, F);                                                                             \
      L7M_SLOW(0, 1, F);                                                                                         \
    }                                                                                                            \
    if (R == 4) L7M_SLOW(4, 2, F);                                                                               \
    if (R == 8) L7M_SLOW(8, 2, F);                                                                               \
    L7M_SLOW(0, 2, F);                                                                                           \
  }

L7M_FEAT_DEFS(L7M_FEAT)
L7M_FEAT_DEFS(L7M_FEAT_DENSE)

#undef L7M_FEAT_DEFS
#undef L7M_SLOW
#undef L7M_MODES
#undef L7M_ONE

}  // namespace l7m
