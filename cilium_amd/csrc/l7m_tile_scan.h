// l7m_tile_scan.h — the measure / scan / emit scaffold of the device tile
// pipelines (l7m_http_wire.hip, l7m_http_log.hip, l7m_kafka_side.hip,
// l7m_stream_frame.hip).  A workgroup owns a tile of kTileThreads items, one
// per lane.  Measure leaves a size per item and a sum per tile (tile_sum_out),
// tile_scan_kernel turns the sums into tile bases and the total, emit gets its
// offsets from tile_exclusive; tile_pipeline enqueues the three on a stream.
//
// Barriers.  tile_sum_out and tile_exclusive are collectives of the whole
// workgroup, so a kernel may return early (even uniformly) only after its
// last call.  Each contains at least one __syncthreads() after entry: LDS that
// every lane wrote before the call is visible after it.  Other lanes may still
// read `tmp` when a call returns: another __syncthreads() goes between a call
// and whatever next writes tmp, a second call included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "l7m_device.h"

namespace l7m {
namespace {

constexpr uint32_t kTileThreads = 256;  // items per tile = threads per workgroup
constexpr uint32_t kScanThreads = 1024;

// Bytes in global memory or LDS; word(i) where p + i is a multiple of four.
struct ByteSrc {
  const uint8_t* p;
  __device__ uint8_t at(uint64_t i) const { return p[i]; }
  __device__ uint32_t word(uint64_t i) const { return *reinterpret_cast<const uint32_t*>(p + i); }
};

// Item i of n is [offs[i], offs[i + 1]) clamped to [0, bytes], so that no
// offset array can lead a load outside the buffer; empty for i >= n.
struct ClampedRange {
  uint64_t lo, hi;
};

__device__ __forceinline__ ClampedRange clamped_range(const uint64_t* offs, uint64_t i, uint64_t n, uint64_t bytes) {
  ClampedRange r{0, 0};
  if (i < n) {
    const uint64_t a = offs[i], b = offs[i + 1];
    r.lo = a < bytes ? a : bytes;
    r.hi = b < bytes ? b : bytes;
    if (r.hi < r.lo) r.hi = r.lo;
  }
  return r;
}

// Inclusive sum over the workgroup (kTileThreads threads) in LDS.
__device__ __forceinline__ uint64_t block_inclusive(uint64_t v, uint64_t* tmp /* LDS, kTileThreads */) {
  tmp[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kTileThreads; d <<= 1) {
    const uint64_t add = threadIdx.x >= d ? tmp[threadIdx.x - d] : 0;
    __syncthreads();
    tmp[threadIdx.x] += add;
    __syncthreads();
  }
  return tmp[threadIdx.x];
}

// The measure pass's tail: tile_sums[this tile] = the sum of the lanes' sizes.
__device__ __forceinline__ void tile_sum_out(uint64_t size, uint64_t* tmp /* LDS */, uint64_t* tile_sums) {
  const uint64_t incl = block_inclusive(size, tmp);
  if (threadIdx.x == kTileThreads - 1) tile_sums[blockIdx.x] = incl;
}

// The emit pass's head: this lane's exclusive offset among all items.
// Contains at least one __syncthreads() after entry; tmp may be written again
// only after another barrier.
__device__ __forceinline__ uint64_t tile_exclusive(uint64_t size, uint64_t* tmp /* LDS */, const uint64_t* tile_base) {
  return tile_base[blockIdx.x] + block_inclusive(size, tmp) - size;
}

// tile_sums[0, tiles) -> exclusive sums in place, *total.  One workgroup: each
// thread sums a contiguous share, the shares are scanned in LDS.
__global__ __launch_bounds__(kScanThreads) void tile_scan_kernel(uint64_t* tile_sums, uint64_t tiles,
                                                                 uint64_t* total) {
  __shared__ uint64_t part[kScanThreads];
  const uint64_t per = (tiles + kScanThreads - 1) / kScanThreads;
  const uint64_t lo = per * threadIdx.x < tiles ? per * threadIdx.x : tiles;
  const uint64_t hi = lo + per < tiles ? lo + per : tiles;
  uint64_t s = 0;
  for (uint64_t t = lo; t < hi; ++t) s += tile_sums[t];
  part[threadIdx.x] = s;
  __syncthreads();
  for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
    const uint64_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  uint64_t run = part[threadIdx.x] - s;
  for (uint64_t t = lo; t < hi; ++t) {
    const uint64_t v = tile_sums[t];
    tile_sums[t] = run;
    run += v;
  }
  if (threadIdx.x == kScanThreads - 1) *total = part[threadIdx.x];
}

// Enqueues one pipeline over n > 0 items: measure, one scan per entry of
// `totals` (device words), emit.  One scratch allocation holds a column of
// tile sums per total, column k at tile_sums + k * tiles, and `extra` bytes
// behind them for what the pipeline keeps between its passes.  Both callables
// take (tiles, tile_sums, the extra bytes): `measure` enqueues the measure
// kernel on `tiles` workgroups, `emit` the emit kernel and whatever follows.
template <class Measure, class Emit>
hipError_t tile_pipeline(uint64_t n, std::initializer_list<uint64_t*> totals, size_t extra, hipStream_t stream,
                         Measure&& measure, Emit&& emit) {
  const uint64_t tiles = (n + kTileThreads - 1) / kTileThreads;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  void* scratch = nullptr;
  hipError_t e = scratch_alloc_async(&scratch, totals.size() * tiles * sizeof(uint64_t) + extra, stream);
  if (e != hipSuccess) return e;
  uint64_t* tile_sums = static_cast<uint64_t*>(scratch);
  void* rest = tile_sums + totals.size() * tiles;
  measure(static_cast<uint32_t>(tiles), tile_sums, rest);
  uint64_t* column = tile_sums;
  for (uint64_t* total : totals) {
    tile_scan_kernel<<<dim3(1), dim3(kScanThreads), 0, stream>>>(column, tiles, total);
    column += tiles;
  }
  emit(static_cast<uint32_t>(tiles), tile_sums, rest);
  e = hipGetLastError();
  const hipError_t f = hipFreeAsync(scratch, stream);
  return e != hipSuccess ? e : f;
}

}  // namespace
}  // namespace l7m
