// l7m_wave.h -- wave-level device helpers shared by the HTTP kernels
// (l7m_http_impl.h) and the Kafka kernels (l7m_kafka.hip).  No state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/l7match.h"

namespace l7m {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// A wave-uniform lane's 64-bit value: v_readlane (no LDS round trip, unlike
// the ds_bpermute of __shfl); `src` must be wave-uniform.
__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t src) {
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(v), src);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(v >> 32), src);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
  const uint32_t lo = __shfl(static_cast<uint32_t>(v), src);
  const uint32_t hi = __shfl(static_cast<uint32_t>(v >> 32), src);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Counter slot of a verdict: 0 deny, 1 the other negative verdicts, 2 + i
// allowed by rule i.
__device__ __forceinline__ uint32_t hit_slot(int32_t v) {
  return v >= 0 ? static_cast<uint32_t>(v) + 2u : (v == L7M_VERDICT_DENY ? 0u : 1u);
}

// Per-wave aggregated counter increment: one atomic per distinct slot.
// Must be called by every lane of the wave.
__device__ __forceinline__ void count_slot(unsigned long long* __restrict__ hits, uint32_t slot, bool active) {
  uint64_t todo = __ballot(active);
  const uint32_t lane = __lane_id();
  while (todo) {
    const uint32_t leader = __builtin_ctzll(todo);
    const uint32_t key = __shfl(slot, leader);
    const uint64_t same = __ballot(active && slot == key) & todo;
    if (lane == leader) atomicAdd(hits + key, static_cast<unsigned long long>(__popcll(same)));
    todo &= ~same;
  }
}

}  // namespace
}  // namespace l7m
