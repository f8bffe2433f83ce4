// l7m_http_log.hip — verdict side effects of an HTTP batch on the device
// (include/l7match.h l7m_http_access_log_device,
// l7m_proxy_stats_update_device; the entry and the record validation in
// l7m_http_log.h, shared with the host functions of l7m_side.cc).
//
// Access log: a measure / scan / emit pipeline on l7m_tile_scan.h's scaffold.
// A workgroup owns a tile of kTileThreads consecutive requests, one per lane.
//   measure: entry size per request from the record's fixed part and
//            directory, read from global memory; the tile's size sum
//   scan:    exclusive sum of the tile sums, the total
//   emit:    entry offsets (entry_offs[0, n], entry n the total) and, when
//            the total fits, the entries.  The
//            records of the lanes that have an entry are staged into LDS with
//            aligned 16-byte loads, a window of kLogStage arena bytes at a
//            time starting at the lowest record not yet served; a lane whose
//            record lies inside the window reads it from LDS, and the lane of
//            that lowest record reads global memory when the record is larger
//            than the window.  A tile whose records lie within kLogStage
//            bytes (packed records, what every packer and the wire decoder
//            produce, in any order) takes one window; other offsets take
//            more windows, never a different result.
// Entries are byte-packed, so neighbours share dwords: LogOutSink stores the
// dwords that lie wholly inside its entry as dwords and the ragged head and
// tail as bytes, and so never stores a byte another entry owns.
//
// Statistics: one counter per (direction, port, verdict class) in a
// stream-ordered scratch table; a workgroup aggregates kStatsSpan tiles in an
// LDS hash table and issues one global atomic per distinct counter it saw.
//
// Compiled as part of l7m_kernels.hip's translation unit (included at its
// end, after l7m_http_wire.hip).
#include <hip/hip_runtime.h>

#include "l7m_device.h"
#include "l7m_http_log.h"
#include "l7m_tile_scan.h"

namespace l7m {
namespace {

constexpr uint32_t kLogStage = 64u * 1024u;   // staged arena bytes per window (256 per request)

// The arena in global memory (16-byte aligned; record offsets are 4-aligned)
// is a ByteSrc.  Arena bytes [base, base + staged) in LDS, base a multiple of 16.
struct LogLdsSrc {
  const uint8_t* lds;
  uint64_t base;
  __device__ uint8_t at(uint64_t i) const { return lds[i - base]; }
  __device__ uint32_t word(uint64_t i) const { return *reinterpret_cast<const uint32_t*>(lds + (i - base)); }
};

// Entry bytes in order -> stores to [p, ...), p of any alignment.  A dword
// that the entry covers completely is stored as one; the bytes of a dword it
// shares with a neighbour (before its first or after its last byte) are
// stored one by one, so that only bytes of this entry are ever written.
struct LogOutSink {
  uint8_t* p;       // the next byte
  uint32_t acc;     // bytes gathered of the dword p lies in
  uint32_t first;   // index in that dword of the first byte gathered
  __device__ explicit LogOutSink(uint8_t* q)
      : p(q), acc(0), first(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(q)) & 3u) {}
  __device__ void put(uint8_t b) {
    const uint32_t k = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 3u;
    acc |= static_cast<uint32_t>(b) << (8u * k);
    ++p;
    if (k == 3u) flush(4u);
  }
  // bytes [first, end) of the dword that ends at or after p
  __device__ void flush(uint32_t end) {
    uint8_t* w = p - end;
    if (first == 0 && end == 4u) {
      *reinterpret_cast<uint32_t*>(w) = acc;
    } else {
      for (uint32_t b = first; b < end; ++b) w[b] = static_cast<uint8_t>(acc >> (8u * b));
    }
    acc = 0;
    first = 0;
  }
  __device__ void finish() {
    const uint32_t k = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)) & 3u;
    if (k) flush(k);
  }
};

__global__ __launch_bounds__(kTileThreads) void http_log_measure(const uint8_t* arena, uint64_t arena_bytes,
                                                                 const uint64_t* offs, uint64_t n,
                                                                 const int32_t* verdicts, const LogConstsFixed c,
                                                                 uint32_t select, uint64_t* sizes /* = entry_offs */,
                                                                 uint64_t* tile_sums) {
  __shared__ uint64_t tmp[kTileThreads];
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  uint64_t size = 0;
  if (i < n) {
    const int32_t vd = verdicts[i];
    const ByteSrc src{arena};
    LogView v;
    if (log_wanted(vd, select) && log_view(src, arena_bytes, offs[i], v)) size = log_measure(src, v, vd, c);
    sizes[i] = size;
  }
  tile_sum_out(size, tmp, tile_sums);
}

// Window control words in LDS.
struct LogCtl {
  unsigned long long lo;  // lowest record offset among the lanes that still have an entry to write
  uint32_t end;           // bytes to stage
  uint32_t pad;
};
constexpr unsigned long long kLogNone = ~0ull;
constexpr uint32_t kLogLds = kLogStage + kTileThreads * sizeof(uint64_t) + sizeof(LogCtl);  // stage, tmp, ctl

__global__ __launch_bounds__(kTileThreads) void http_log_emit(const uint8_t* arena, uint64_t arena_bytes,
                                                              const uint64_t* offs, uint64_t n,
                                                              const int32_t* verdicts, const LogConstsFixed c,
                                                              uint8_t* out, uint64_t cap, uint64_t* entry_offs,
                                                              const uint64_t* tile_base, const uint64_t* total) {
  extern __shared__ __attribute__((aligned(16))) uint8_t log_smem[];
  uint64_t* tmp = reinterpret_cast<uint64_t*>(log_smem + kLogStage);
  LogCtl* ctl = reinterpret_cast<LogCtl*>(tmp + kTileThreads);
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint64_t size = i < n ? entry_offs[i] : 0;  // the measure pass left the sizes here
  const uint64_t eoff = tile_exclusive(size, tmp, tile_base);
  const uint64_t all = *total;
  if (i < n) entry_offs[i] = eoff;
  if (i + 1 == n) entry_offs[n] = all;
  if (all > cap) return;  // uniform: the output stays untouched
  // a lane with an entry: the measure pass validated its record, arena[lo, hi)
  bool todo = size != 0;
  uint64_t lo = 0, hi = 0;
  int32_t vd = 0;
  if (todo) {
    lo = offs[i];
    hi = lo + ByteSrc{arena}.word(lo);
    vd = verdicts[i];
  }
  auto emit = [&](const auto& src) {
    LogView v;
    log_view(src, arena_bytes, lo, v);
    LogOutSink k(out + eoff);
    log_emit(src, v, vd, c, k);
    k.finish();
  };
  for (;;) {  // uniform
    if (threadIdx.x == 0) {
      ctl->lo = kLogNone;
      ctl->end = 0;
    }
    __syncthreads();
    if (todo) atomicMin(&ctl->lo, static_cast<unsigned long long>(lo));
    __syncthreads();
    const uint64_t first = ctl->lo;
    if (first == kLogNone) break;
    const uint64_t base = first & ~15ull;
    const bool staged = todo && hi - base <= kLogStage;  // lo >= first >= base
    if (staged) atomicMax(&ctl->end, static_cast<uint32_t>(hi - base));
    __syncthreads();
    // base + end <= arena_bytes, and the arena is readable to the next multiple of 16
    const uint32_t units = (ctl->end + 15u) >> 4;
    for (uint32_t u = threadIdx.x; u < units; u += kTileThreads)
      *reinterpret_cast<uint4*>(log_smem + 16u * u) = *reinterpret_cast<const uint4*>(arena + base + 16ull * u);
    __syncthreads();
    if (staged) {
      emit(LogLdsSrc{log_smem, base});
      todo = false;
    } else if (todo && lo == first) {  // larger than the window
      emit(ByteSrc{arena});
      todo = false;
    }
    __syncthreads();
  }
}

// ---- proxy statistics -------------------------------------------------------
constexpr uint32_t kStatsSpan = 8;                               // tiles per workgroup
constexpr uint32_t kStatsSlots = 2 * kStatsSpan * kTileThreads;  // LDS hash slots: at most half of them fill
constexpr uint32_t kStatsEmpty = 0xffffffffu;
static_assert(kStatsSlots == 1u << 12, "http_stats_count hashes a key to 12 bits");

__global__ __launch_bounds__(kTileThreads) void http_stats_count(const uint8_t* arena, uint64_t arena_bytes,
                                                                 const uint64_t* offs, const int32_t* verdicts,
                                                                 uint64_t n, uint32_t caller_row,
                                                                 unsigned long long* counters /* kStatsCounters */) {
  __shared__ uint32_t keys[kStatsSlots];
  __shared__ uint32_t counts[kStatsSlots];
  for (uint32_t s = threadIdx.x; s < kStatsSlots; s += kTileThreads) {
    keys[s] = kStatsEmpty;
    counts[s] = 0;
  }
  __syncthreads();
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * kStatsSpan * kTileThreads;
  const uint32_t lane = __lane_id();
  for (uint32_t t = 0; t < kStatsSpan; ++t) {  // uniform
    const uint64_t i = first + static_cast<uint64_t>(t) * kTileThreads + threadIdx.x;
    const bool active = i < n;
    uint32_t key = 0;
    if (active) {
      LogView v;
      uint32_t row = caller_row;  // a record that does not validate: the caller's port and direction
      if (log_view(ByteSrc{arena}, arena_bytes, offs[i], v))
        row = ((v.flags & L7M_HTTP_F_INGRESS) ? 65536u : 0u) | v.dport;
      key = row * kStatsClasses + flow_verdict(verdicts[i]);
    }
    // one LDS insertion per distinct key of the wave
    uint64_t left = __ballot(active);
    while (left) {
      const uint32_t leader = __builtin_ctzll(left);
      const uint32_t k = __shfl(key, leader);
      const uint64_t same = __ballot(active && key == k) & left;
      if (lane == leader) {
        uint32_t s = (k * 2654435761u) >> 20 & (kStatsSlots - 1);
        for (;;) {  // ends: the table never fills
          const uint32_t prev = atomicCAS(&keys[s], kStatsEmpty, k);
          if (prev == kStatsEmpty || prev == k) break;
          s = (s + 1) & (kStatsSlots - 1);
        }
        atomicAdd(&counts[s], static_cast<uint32_t>(__popcll(same)));
      }
      left &= ~same;
    }
  }
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < kStatsSlots; s += kTileThreads)
    if (counts[s]) atomicAdd(counters + keys[s], static_cast<unsigned long long>(counts[s]));
}

}  // namespace

hipError_t launch_http_log(const BatchView& b, const LogConstsFixed& c, uint32_t select, uint8_t* out, uint64_t cap,
                           uint64_t* entry_offs, uint64_t* total, hipStream_t stream) {
  if (b.n == 0) {
    hipError_t e = hipMemsetAsync(total, 0, sizeof(uint64_t), stream);
    if (e == hipSuccess && entry_offs) e = hipMemsetAsync(entry_offs, 0, sizeof(uint64_t), stream);
    return e;
  }
  const hipError_t e = set_lds_attr_once(reinterpret_cast<const void*>(&http_log_emit), kLogLds);
  if (e != hipSuccess) return e;
  return tile_pipeline(
      b.n, {total}, 0, stream,
      [&](uint32_t tiles, uint64_t* tile_sums, void*) {
        http_log_measure<<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(b.arena, b.arena_bytes, b.offs, b.n,
                                                                         b.verdicts, c, select, entry_offs, tile_sums);
      },
      [&](uint32_t tiles, const uint64_t* tile_base, void*) {
        http_log_emit<<<dim3(tiles), dim3(kTileThreads), kLogLds, stream>>>(
            b.arena, b.arena_bytes, b.offs, b.n, b.verdicts, c, out, cap, entry_offs, tile_base, total);
      });
}

hipError_t launch_http_stats(const BatchView& b, uint32_t caller_row, uint64_t* host_counters, hipStream_t stream) {
  const uint64_t groups = (b.n + kStatsSpan * kTileThreads - 1) / (kStatsSpan * kTileThreads);
  if (groups > 0x7fffffffull) return hipErrorInvalidValue;
  const size_t bytes = static_cast<size_t>(kStatsCounters) * sizeof(uint64_t);
  void* scratch = nullptr;  // one kernel, no sizes or scan: not a tile_pipeline, so the scratch is handled here
  hipError_t e = scratch_alloc_async(&scratch, bytes, stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(scratch, 0, bytes, stream);
  if (e == hipSuccess && groups) {
    http_stats_count<<<dim3(static_cast<uint32_t>(groups)), dim3(kTileThreads), 0, stream>>>(
        b.arena, b.arena_bytes, b.offs, b.verdicts, b.n, caller_row, static_cast<unsigned long long*>(scratch));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_counters, scratch, bytes, hipMemcpyDeviceToHost, stream);
  const hipError_t f = hipFreeAsync(scratch, stream);
  const hipError_t s = hipStreamSynchronize(stream);
  return e != hipSuccess ? e : f != hipSuccess ? f : s;
}

}  // namespace l7m
