// l7m_kafka_side.hip — verdict side effects of a Kafka batch on the device
// (include/l7match.h l7m_kafka_deny_responses_device,
// l7m_kafka_access_log_device; the request walk, the response and the record
// fields in l7m_kafka_side.h, shared with the host functions of l7m_side.cc).
//
// A measure / scan / emit pipeline on l7m_tile_scan.h's scaffold.  A workgroup
// owns a tile of kTileThreads consecutive requests, one per lane.
//   measure: the request is validated and walked; the response's size (or the
//            number of its topics) per request, the tile's sum
//   scan:    exclusive sum of the tile sums, the total
//   emit:    offsets [0, n] and, when the total fits, the output: the request
//            is walked once more and the visitor writes as it goes
// Both passes read the request from global memory byte by byte, each lane its
// own: Kafka requests carry no alignment, and neighbouring lanes read
// neighbouring requests, so the lines they share come from L2.  A request of
// any size is read the same way; there is no stage to outgrow.  A lane reads
// inside [offset, offset + 4 + size field) only, which kafka_rec checked
// against the arena, and its loops end with the request (kafka_walk).
// Responses are byte-packed, so neighbours share dwords: LogOutSink stores the
// dwords that lie wholly inside its response as dwords and the ragged head and
// tail as bytes, so every byte is stored once, by its owner.  Log records are
// 40-byte structs at 8-byte alignment: plain stores.
// The CRC-32 of a Produce request's messages (readMessageSet stops at a bad
// one) goes through a 256-entry table that the workgroup's 256 lanes build in
// LDS, one entry each: one LDS read per message byte where the bitwise loop
// takes eight dependent shift-and-select steps.
//
// Compiled as part of l7m_kernels.hip's translation unit (included at its
// end, after l7m_http_log.hip, whose LogOutSink it uses).
#include <hip/hip_runtime.h>

#include "l7m_device.h"
#include "l7m_kafka_side.h"
#include "l7m_tile_scan.h"

namespace l7m {
namespace {

static_assert(kTileThreads == 256, "a lane builds one entry of the CRC table");

// The arena is a ByteSrc read with at() only: record offsets have any alignment.

struct KsCrcLds {
  const uint32_t* tab;  // LDS, 256 entries
  __device__ uint32_t operator()(uint32_t c, uint8_t b) const { return tab[(c ^ b) & 0xffu] ^ (c >> 8); }
};

// Entry threadIdx.x of the table; the caller synchronises.
__device__ __forceinline__ void ks_crc_fill(uint32_t* tab) {
  tab[threadIdx.x] = KafkaCrcBitwise{}(0u, static_cast<uint8_t>(threadIdx.x));
}

// A response's bytes -> LogOutSink, never more than the measure pass counted.
// LogOutSink's members are inlined at these two call sites, so the sink stays
// in registers.
struct KsRespSink {
  LogOutSink k;
  uint64_t left;
  __device__ KsRespSink(uint8_t* p, uint64_t size) : k(p), left(size) {}
  __device__ __forceinline__ void put(uint8_t b) {
    if (left) {
      --left;
      [[clang::always_inline]] k.put(b);
    }
  }
  __device__ __forceinline__ void finish() { [[clang::always_inline]] k.finish(); }
};

// The records of one request -> out[0, left).
struct KsLogEmit {
  l7m_kafka_log_record* out;
  uint64_t left, request;
  int32_t verdict;
  __device__ void topics(const KafkaHead&, int32_t) {}
  __device__ void topic(const KafkaHead& h, uint64_t at, uint32_t nl, int32_t) {
    if (!left) return;
    l7m_kafka_log_record r;
    kafka_log_fill(r, request, verdict, h, at, nl);
    *out++ = r;
    --left;
  }
  __device__ void partition(const KafkaHead&, int32_t) {}
  __device__ void end(const KafkaHead&) {}
};

// kLog: log records (sizes count records, `select` as kafka_log_wanted takes
// it); otherwise deny responses (sizes count bytes, denied requests only).
template <bool kLog>
__global__ __launch_bounds__(kTileThreads) void kafka_side_measure(const uint8_t* arena, uint64_t arena_bytes,
                                                                   const uint64_t* offs, uint64_t n,
                                                                   const int32_t* verdicts, uint32_t select,
                                                                   uint64_t* sizes /* = the output's offsets */,
                                                                   uint64_t* tile_sums) {
  __shared__ uint64_t tmp[kTileThreads];
  __shared__ uint32_t crc_tab[256];
  ks_crc_fill(crc_tab);
  __syncthreads();
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  uint64_t size = 0;
  if (i < n) {
    const int32_t vd = verdicts[i];
    const ByteSrc src{arena};
    const uint64_t off = offs[i];
    uint64_t len = 0;
    if ((kLog ? kafka_log_wanted(vd, select) : vd == L7M_VERDICT_DENY) && kafka_rec(src, arena_bytes, off, &len)) {
      KafkaHead h;
      if (kLog) {
        KafkaTopicCount c;
        if (kafka_walk(src, off, len, KsCrcLds{crc_tab}, h, c) == L7M_OK) size = c.topics_seen;
      } else {
        KafkaRespSize c;
        if (kafka_walk(src, off, len, KsCrcLds{crc_tab}, h, c) == L7M_OK) size = c.bytes;
      }
    }
    sizes[i] = size;
  }
  tile_sum_out(size, tmp, tile_sums);
}

template <bool kLog>
__global__ __launch_bounds__(kTileThreads) void kafka_side_emit(const uint8_t* arena, uint64_t arena_bytes,
                                                                const uint64_t* offs, uint64_t n,
                                                                const int32_t* verdicts, uint8_t* out, uint64_t cap,
                                                                uint64_t* out_offs, const uint64_t* tile_base,
                                                                const uint64_t* total) {
  __shared__ uint64_t tmp[kTileThreads];
  __shared__ uint32_t crc_tab[256];
  ks_crc_fill(crc_tab);  // visible after tile_exclusive: its contract promises a barrier
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint64_t size = i < n ? out_offs[i] : 0;  // the measure pass left the sizes here
  const uint64_t eoff = tile_exclusive(size, tmp, tile_base);
  const uint64_t all = *total;
  if (i < n) out_offs[i] = eoff;
  if (i + 1 == n) out_offs[n] = all;
  if (all > cap) return;  // uniform: the output stays untouched
  if (!size) return;
  // the measure pass validated this lane's request and walked it to the end
  const ByteSrc src{arena};
  const uint64_t off = offs[i];
  uint64_t len = 0;
  if (!kafka_rec(src, arena_bytes, off, &len)) return;
  KafkaHead h;
  if (kLog) {
    KsLogEmit e{reinterpret_cast<l7m_kafka_log_record*>(out) + eoff, size, i, verdicts[i]};
    kafka_walk(src, off, len, KsCrcLds{crc_tab}, h, e);
  } else {
    KafkaRespEmit<ByteSrc, KsRespSink> e(src, KsRespSink(out + eoff, size), size);
    kafka_walk(src, off, len, KsCrcLds{crc_tab}, h, e);
    e.k.finish();
  }
}

template <bool kLog>
hipError_t launch_kafka_side_as(const BatchView& b, uint32_t select, uint8_t* out, uint64_t cap, uint64_t* out_offs,
                                uint64_t* total, hipStream_t stream) {
  if (b.n == 0) {
    hipError_t e = hipMemsetAsync(total, 0, sizeof(uint64_t), stream);
    if (e == hipSuccess && out_offs) e = hipMemsetAsync(out_offs, 0, sizeof(uint64_t), stream);
    return e;
  }
  return tile_pipeline(
      b.n, {total}, 0, stream,
      [&](uint32_t tiles, uint64_t* tile_sums, void*) {
        kafka_side_measure<kLog><<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(
            b.arena, b.arena_bytes, b.offs, b.n, b.verdicts, select, out_offs, tile_sums);
      },
      [&](uint32_t tiles, const uint64_t* tile_base, void*) {
        kafka_side_emit<kLog><<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(
            b.arena, b.arena_bytes, b.offs, b.n, b.verdicts, out, cap, out_offs, tile_base, total);
      });
}

}  // namespace

hipError_t launch_kafka_side(bool log, const BatchView& b, uint32_t select, uint8_t* out, uint64_t cap,
                             uint64_t* out_offs, uint64_t* total, hipStream_t stream) {
  return log ? launch_kafka_side_as<true>(b, select, out, cap, out_offs, total, stream)
             : launch_kafka_side_as<false>(b, select, out, cap, out_offs, total, stream);
}

}  // namespace l7m
