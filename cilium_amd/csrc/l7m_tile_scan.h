// l7m_tile_scan.h — the scan between a measure pass and an emit pass, shared
// by the HTTP wire decoder (l7m_http_wire.hip) and the access-log encoder
// (l7m_http_log.hip): every workgroup owns a tile of kTileThreads items, one
// per lane; the measure pass leaves a size per item and a sum per tile, one
// workgroup turns the tile sums into tile bases, and the emit pass adds the
// sum inside the tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace l7m {
namespace {

constexpr uint32_t kTileThreads = 256;  // items per tile = threads per workgroup
constexpr uint32_t kScanThreads = 1024;

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

// tile_sums[0, tiles) -> exclusive sums in place, *total.  One workgroup: each
// thread sums a contiguous share, the shares are scanned in LDS.
__global__ __launch_bounds__(kScanThreads) void http_wire_scan_tiles(uint64_t* tile_sums, uint64_t tiles,
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

}  // namespace
}  // namespace l7m
