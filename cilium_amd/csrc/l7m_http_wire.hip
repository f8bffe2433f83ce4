// l7m_http_wire.hip — HTTP/1.x request heads -> request arena on the device
// (include/l7match.h l7m_http_wire_decode_device; grammar in l7m_http_wire.h,
// shared with the host decoder).
//
// Two passes over the wire bytes with a scan between them.  A workgroup owns
// a tile of kTileThreads consecutive heads, whose bytes are one contiguous
// range of the wire.  It stages as many of them as fit kWireStage bytes of LDS with
// aligned 16-byte loads (a chunk; an ordinary tile is one chunk) and parses
// them one head per lane from LDS.  A head that does not fit the stage on its
// own is walked from global memory by its lane.
//   measure: status and padded record size per head, the tile's size sum
//   scan:    exclusive sum of the tile sums, the total
//   emit:    record offsets (rec_offsets[0, n); no entry n) and, when the
//            total fits the arena, the records, one aligned dword per store
//
// Compiled as part of l7m_kernels.hip's translation unit (included at its
// end): the library keeps one gfx950 code object per entry of the Makefile's
// DEV_SRCS / FEAT_OBJS, which cilium_amd/codehash.py and its test count.
#include <hip/hip_runtime.h>

#include "l7m_device.h"
#include "l7m_http_wire.h"
#include "l7m_tile_scan.h"

namespace l7m {
namespace {

constexpr uint32_t kWireStage = 64u * 1024u;   // staged wire bytes per chunk (256 per head)
constexpr uint32_t kWireLds = kWireStage + kTileThreads * sizeof(uint64_t) + 16;  // stage, tile_lo, s_end

// Record bytes in order -> aligned dword stores (records are 4-byte aligned
// and a multiple of four bytes long).
struct DwordSink {
  uint32_t* dst;
  uint32_t acc = 0, k = 0;
  __device__ void put(uint8_t b) {
    acc |= static_cast<uint32_t>(b) << (8u * (k & 3u));
    if ((++k & 3u) == 0) {
      dst[(k >> 2) - 1] = acc;
      acc = 0;
    }
  }
};

// Stage wire addresses [gbase, gend) (gbase 16-byte aligned) into lds[0, ...):
// aligned 16-byte loads for the units inside the wire buffer, guarded bytes
// for a unit that straddles one of its ends.
__device__ __forceinline__ void stage_chunk(uint8_t* lds, const uint8_t* wire, uint64_t wire_bytes, uint64_t gbase,
                                            uint64_t gend) {
  const uint64_t w0 = reinterpret_cast<uint64_t>(wire), w1 = w0 + wire_bytes;
  const uint32_t units = static_cast<uint32_t>((gend - gbase + 15) >> 4);
  for (uint32_t u = threadIdx.x; u < units; u += kTileThreads) {
    const uint64_t g = gbase + 16ull * u;
    uint4 v;
    if (g >= w0 && g + 16 <= w1) {
      v = *reinterpret_cast<const uint4*>(g);
    } else {
      uint32_t w[4] = {0, 0, 0, 0};
      for (uint32_t b = 0; b < 16; ++b)
        if (g + b >= w0 && g + b < w1)
          w[b >> 2] |= static_cast<uint32_t>(*reinterpret_cast<const uint8_t*>(g + b)) << (8u * (b & 3u));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(lds + 16u * u) = v;
  }
}

// Walks the tile chunk by chunk: f(src, len) runs once per head, on its lane,
// with a ByteSrc into LDS for a staged head and into the wire for one larger
// than the stage.  The head of lane t is wire[r.lo, r.hi) (clamped_range).
// A staged head is read a byte at a time.  (Keeping an aligned 8-byte window
// of the stage in registers, one ds_read_b64 per eight bytes, measured slower:
// 11.9 ms against 8.7 ms on 8.2 M heads of config 2.  The parse is bound by
// its per-byte branches, not by the LDS loads.)
template <class F>
__device__ __forceinline__ void for_each_head(uint8_t* lds, const uint8_t* wire, uint64_t wire_bytes, ClampedRange r,
                                              uint32_t cnt, const uint64_t* tile_lo /* LDS, kTileThreads */,
                                              uint64_t* s_end /* LDS, one word */, F&& f) {
  const uint64_t w0 = reinterpret_cast<uint64_t>(wire);
  uint32_t a = 0;
  while (a < cnt) {  // uniform
    const uint64_t gbase = (w0 + tile_lo[a]) & ~15ull;
    const bool fits = threadIdx.x >= a && threadIdx.x < cnt && r.lo >= tile_lo[a] && w0 + r.hi - gbase <= kWireStage;
    // ascending offsets: the heads that fit are a run starting at a
    uint32_t k = static_cast<uint32_t>(__syncthreads_count(fits));
    if (k == 0) k = 1;  // head a alone is larger than the stage
    // the run's last head ends the staged range
    if (threadIdx.x == a) *s_end = gbase;  // nothing staged unless a head fits
    __syncthreads();
    if (fits && threadIdx.x == a + k - 1) *s_end = w0 + r.hi;
    __syncthreads();
    const uint64_t gend = *s_end;
    stage_chunk(lds, wire, wire_bytes, gbase, gend);
    __syncthreads();
    if (threadIdx.x >= a && threadIdx.x < a + k) {
      if (fits && w0 + r.hi <= gend)
        f(ByteSrc{lds + (w0 + r.lo - gbase)}, r.hi - r.lo);
      else
        f(ByteSrc{wire + r.lo}, r.hi - r.lo);
    }
    __syncthreads();
    a += k;
  }
}

__global__ __launch_bounds__(kTileThreads) void http_wire_measure(const uint8_t* wire, uint64_t wire_bytes,
                                                                  const uint64_t* head_offs, uint64_t n,
                                                                  uint64_t* sizes /* = rec_offsets */,
                                                                  int32_t* status, uint64_t* tile_sums) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wire_smem[];
  uint64_t* tile_lo = reinterpret_cast<uint64_t*>(wire_smem + kWireStage);
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint64_t left = n - static_cast<uint64_t>(blockIdx.x) * kTileThreads;
  const uint32_t cnt = left < kTileThreads ? static_cast<uint32_t>(left) : kTileThreads;
  const ClampedRange r = clamped_range(head_offs, i, n, wire_bytes);
  tile_lo[threadIdx.x] = r.lo;
  __syncthreads();
  uint64_t size = 0;
  uint64_t* s_end = tile_lo + kTileThreads;
  for_each_head(wire_smem, wire, wire_bytes, r, cnt, tile_lo, s_end, [&](const auto& src, uint64_t len) {
    WireInfo info;
    wire_scan(src, len, info);
    size = info.status < 0 ? L7M_HTTP_REC_FIXED : wire_padded(info.rec_len);
    status[i] = info.status;
    sizes[i] = size;
  });
  tile_sum_out(size, tile_lo, tile_sums);  // tile_lo is free after for_each_head's last barrier
}

__global__ __launch_bounds__(kTileThreads) void http_wire_emit(const uint8_t* wire, uint64_t wire_bytes,
                                                               const uint64_t* head_offs, uint64_t n,
                                                               const l7m_http_wire_meta* meta, uint8_t* arena,
                                                               uint64_t cap, uint64_t* rec_offsets,
                                                               const uint64_t* tile_base, const uint64_t* total) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wire_smem[];
  uint64_t* tile_lo = reinterpret_cast<uint64_t*>(wire_smem + kWireStage);
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint64_t left = n - static_cast<uint64_t>(blockIdx.x) * kTileThreads;
  const uint32_t cnt = left < kTileThreads ? static_cast<uint32_t>(left) : kTileThreads;
  const uint64_t size = i < n ? rec_offsets[i] : 0;  // the measure pass left the sizes here
  const uint64_t off = tile_exclusive(size, tile_lo, tile_base);
  if (i < n) rec_offsets[i] = off;
  if (*total > cap) return;  // uniform: the arena stays untouched
  __syncthreads();  // tile_lo was the sum's tmp
  const ClampedRange r = clamped_range(head_offs, i, n, wire_bytes);
  tile_lo[threadIdx.x] = r.lo;
  __syncthreads();
  uint64_t* s_end = tile_lo + kTileThreads;
  for_each_head(wire_smem, wire, wire_bytes, r, cnt, tile_lo, s_end, [&](const auto& src, uint64_t len) {
    WireInfo info;
    wire_scan(src, len, info);
    l7m_http_wire_meta m{0, 0, 0, 1, {0, 0, 0}};  // no metadata: zeros, ingress
    if (meta) m = meta[i];
    DwordSink k{reinterpret_cast<uint32_t*>(arena + off)};
    if (info.status < 0) wire_emit_failed(&m, k);
    else wire_emit(src, info, &m, k);
  });
}

}  // namespace

hipError_t launch_http_wire(const uint8_t* wire, uint64_t wire_bytes, const uint64_t* head_offs, uint64_t n,
                            const l7m_http_wire_meta* meta, uint8_t* arena, uint64_t cap, uint64_t* rec_offsets,
                            int32_t* status, uint64_t* total, hipStream_t stream) {
  if (n == 0) return hipMemsetAsync(total, 0, sizeof(uint64_t), stream);
  hipError_t e = set_lds_attr_once(reinterpret_cast<const void*>(&http_wire_measure), kWireLds);
  if (e == hipSuccess) e = set_lds_attr_once(reinterpret_cast<const void*>(&http_wire_emit), kWireLds);
  if (e != hipSuccess) return e;
  return tile_pipeline(
      n, {total}, 0, stream,
      [&](uint32_t tiles, uint64_t* tile_sums, void*) {
        http_wire_measure<<<dim3(tiles), dim3(kTileThreads), kWireLds, stream>>>(wire, wire_bytes, head_offs, n,
                                                                                 rec_offsets, status, tile_sums);
      },
      [&](uint32_t tiles, const uint64_t* tile_base, void*) {
        http_wire_emit<<<dim3(tiles), dim3(kTileThreads), kWireLds, stream>>>(
            wire, wire_bytes, head_offs, n, meta, arena, cap, rec_offsets, tile_base, total);
      });
}

}  // namespace l7m
