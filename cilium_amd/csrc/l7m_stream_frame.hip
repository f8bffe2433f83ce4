// l7m_stream_frame.hip — connection byte streams -> head slices / Kafka
// records on the device (include/l7match.h l7m_http_stream_frame_device,
// l7m_kafka_stream_frame_device; the framing rules in l7m_stream_frame.h,
// shared with the host functions of stream_frame.cc).
//
// Work is sequential inside a connection and independent across connections:
// a workgroup owns a tile of kTileThreads consecutive connections, one per
// lane.  Two measure / scan / emit pipelines on l7m_tile_scan.h's scaffold
// (and two more for streaming across calls, at the end of this file).
//   count: each lane walks its connection; status, consumed bytes, its number
//          of slices (Kafka: and of padded arena bytes), the tile's sums
//   scan:  exclusive sum of the tile sums, the totals (Kafka: two scans)
//   emit:  when the totals fit the capacities each lane walks its connection
//          again and writes its slices at tile base + sum inside the tile + k
//   copy:  (Kafka) balanced over the arena, not over records: a thread takes
//          16-byte units, finds the record of each by binary search in
//          rec_offsets and reads the unaligned source as aligned dwords joined
//          with v_alignbyte
// The walks read the wire from global memory byte by byte, as the Kafka side
// effects do (l7m_kafka_side.hip): a connection has no size limit, bodies and
// chunk data are skipped by their size, and neighbouring lanes read
// neighbouring connections.  A lane reads inside its connection's range
// clamped to the wire only, whatever the offsets hold.
//
// Compiled as part of l7m_kernels.hip's translation unit (included at its end).
#include <hip/hip_runtime.h>

#include "l7m_device.h"
#include "l7m_stream_frame.h"
#include "l7m_tile_scan.h"

namespace l7m {
namespace {

__global__ __launch_bounds__(kTileThreads) void stream_http_count(const uint8_t* wire, uint64_t wire_bytes,
                                                                  const uint64_t* conn_offs, uint64_t n,
                                                                  int32_t* conn_status, uint64_t* conn_consumed,
                                                                  uint32_t* counts, uint64_t* tile_sums) {
  __shared__ uint64_t tmp[kTileThreads];
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  uint64_t cnt = 0;
  if (c < n) {
    const ClampedRange r = clamped_range(conn_offs, c, n, wire_bytes);
    uint64_t used = 0;
    const int32_t st = http_stream_walk(ByteSrc{wire + r.lo}, r.hi - r.lo, &used, [&](uint64_t) { ++cnt; });
    conn_status[c] = st;
    conn_consumed[c] = used;
    counts[c] = static_cast<uint32_t>(cnt);  // <= (hi - lo) / 16 + 1
  }
  tile_sum_out(cnt, tmp, tile_sums);
}

__global__ __launch_bounds__(kTileThreads) void stream_http_emit(const uint8_t* wire, uint64_t wire_bytes,
                                                                 const uint64_t* conn_offs, uint64_t n,
                                                                 const l7m_http_wire_meta* conn_meta,
                                                                 uint64_t* head_offs, uint32_t* head_conn,
                                                                 l7m_http_wire_meta* head_meta, uint64_t cap,
                                                                 const uint32_t* counts, const uint64_t* tile_base,
                                                                 const uint64_t* total) {
  __shared__ uint64_t tmp[kTileThreads];
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint64_t cnt = c < n ? counts[c] : 0;
  const uint64_t base = tile_exclusive(cnt, tmp, tile_base);
  const uint64_t all = *total;
  if (all > cap || !head_offs) return;  // uniform: the per-head arrays stay untouched
  if (c >= n) return;
  const ClampedRange r = clamped_range(conn_offs, c, n, wire_bytes);
  if (c + 1 == n) head_offs[all] = r.hi;
  if (!cnt) return;
  l7m_http_wire_meta m{0, 0, 0, 1, {0, 0, 0}};  // no metadata: zeros, ingress
  if (conn_meta) m = conn_meta[c];
  uint64_t used = 0, k = 0;
  http_stream_walk(ByteSrc{wire + r.lo}, r.hi - r.lo, &used, [&](uint64_t start) {
    if (k < cnt) {  // never more than the count pass counted
      head_offs[base + k] = r.lo + start;
      head_conn[base + k] = static_cast<uint32_t>(c);
      if (head_meta) head_meta[base + k] = m;
    }
    ++k;
  });
}

// A record's source in the wire: its offset in the low 40 bits, the frame's
// bytes above them (a frame is under 2^23 bytes).
constexpr uint32_t kSrcShift = 40;

__global__ __launch_bounds__(kTileThreads) void stream_kafka_count(const uint8_t* wire, uint64_t wire_bytes,
                                                                   const uint64_t* conn_offs, uint64_t n,
                                                                   int32_t* conn_status, uint64_t* conn_consumed,
                                                                   uint32_t* counts, uint64_t* sizes,
                                                                   uint64_t* tile_recs, uint64_t* tile_bytes) {
  __shared__ uint64_t tmp[kTileThreads];
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  uint64_t cnt = 0, bytes = 0;
  if (c < n) {
    const ClampedRange r = clamped_range(conn_offs, c, n, wire_bytes);
    uint64_t used = 0;
    const int32_t st = kafka_stream_walk(ByteSrc{wire + r.lo}, r.hi - r.lo, &used, [&](uint64_t, uint64_t frame) {
      ++cnt;
      bytes += stream_padded(frame);
    });
    conn_status[c] = st;
    conn_consumed[c] = used;
    counts[c] = static_cast<uint32_t>(cnt);  // <= (hi - lo) / 12
    sizes[c] = bytes;
  }
  tile_sum_out(cnt, tmp, tile_recs);
  __syncthreads();  // before tmp is written again
  tile_sum_out(bytes, tmp, tile_bytes);
}

__global__ __launch_bounds__(kTileThreads) void stream_kafka_emit(
    const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs, uint64_t n, const uint32_t* conn_identity,
    uint64_t* rec_offsets, uint32_t* rec_conn, uint32_t* src_identities, uint64_t cap_recs, uint64_t cap_bytes,
    const uint32_t* counts, const uint64_t* sizes, const uint64_t* tile_recs, const uint64_t* tile_bytes,
    uint64_t* src /* src_cap */, uint64_t src_cap, const uint64_t* n_recs, const uint64_t* arena_bytes) {
  __shared__ uint64_t tmp[kTileThreads];
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint64_t cnt = c < n ? counts[c] : 0;
  const uint64_t bytes = c < n ? sizes[c] : 0;
  const uint64_t base = tile_exclusive(cnt, tmp, tile_recs);
  __syncthreads();  // before tmp is written again
  uint64_t off = tile_exclusive(bytes, tmp, tile_bytes);
  if (*n_recs > cap_recs || *n_recs > src_cap || *arena_bytes > cap_bytes) return;  // uniform: nothing per record
  if (!cnt) return;
  const ClampedRange r = clamped_range(conn_offs, c, n, wire_bytes);
  const uint32_t id = conn_identity ? conn_identity[c] : 0u;
  uint64_t used = 0, k = 0;
  kafka_stream_walk(ByteSrc{wire + r.lo}, r.hi - r.lo, &used, [&](uint64_t start, uint64_t frame) {
    if (k < cnt) {  // never more than the count pass counted
      rec_offsets[base + k] = off;
      rec_conn[base + k] = static_cast<uint32_t>(c);
      if (src_identities) src_identities[base + k] = id;
      src[base + k] = (r.lo + start) | frame << kSrcShift;
      off += stream_padded(frame);
    }
    ++k;
  });
}

// The aligned dword at address g of the wire [w0, w1); bytes outside it read as zero.
__device__ __forceinline__ uint32_t wire_dword(uint64_t g, uint64_t w0, uint64_t w1) {
  if (g >= w0 && g + 4 <= w1) return *reinterpret_cast<const uint32_t*>(g);
  uint32_t v = 0;
  for (uint32_t b = 0; b < 4; ++b)
    if (g + b >= w0 && g + b < w1) v |= static_cast<uint32_t>(*reinterpret_cast<const uint8_t*>(g + b)) << (8u * b);
  return v;
}

// Arena dword at offset q (a multiple of four) of a record whose frame is
// wire[s, s + len): the source bytes, zero past the frame.
__device__ __forceinline__ uint32_t frame_dword(uint64_t w0, uint64_t w1, uint64_t s, uint64_t len, uint64_t q) {
  const uint64_t a = w0 + s + q;
  const uint32_t sh = static_cast<uint32_t>(a & 3u);
  const uint64_t g = a & ~3ull;
  const uint32_t lo = wire_dword(g, w0, w1);
  const uint32_t hi = sh ? wire_dword(g + 4, w0, w1) : 0u;
  uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, sh);
  const uint64_t left = len - q;  // >= 1
  if (left < 4) v &= (1u << (8u * static_cast<uint32_t>(left))) - 1u;
  return v;
}

__global__ __launch_bounds__(kTileThreads) void stream_kafka_copy(const uint8_t* wire, uint64_t wire_bytes,
                                                                  uint8_t* arena, uint64_t cap_recs,
                                                                  uint64_t cap_bytes, const uint64_t* rec_offsets,
                                                                  const uint64_t* src, uint64_t src_cap,
                                                                  const uint64_t* n_recs, const uint64_t* arena_bytes) {
  const uint64_t n = *n_recs, total = *arena_bytes;  // a multiple of four
  if (n > cap_recs || n > src_cap || total > cap_bytes || n == 0) return;
  const uint64_t w0 = reinterpret_cast<uint64_t>(wire), w1 = w0 + wire_bytes;
  const uint64_t units = (total + 15) >> 4;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kTileThreads;
  for (uint64_t u = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x; u < units; u += stride) {
    const uint64_t d0 = u << 4;
    // the record that holds arena byte d0: the last one with rec_offsets[r] <= d0
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (rec_offsets[mid] <= d0) lo = mid;
      else hi = mid;
    }
    uint64_t r = lo, ro = rec_offsets[r];
    uint64_t rend = r + 1 < n ? rec_offsets[r + 1] : total;
    uint64_t sl = src[r];
    uint32_t w[4] = {0, 0, 0, 0};
    const uint32_t nd = total - d0 >= 16 ? 4u : static_cast<uint32_t>((total - d0) >> 2);
    const uint64_t s0 = sl & ((1ull << kSrcShift) - 1), len0 = sl >> kSrcShift;
    const uint64_t a0 = w0 + s0 + (d0 - ro);
    if (nd == 4 && d0 + 16 <= ro + len0 && (a0 & ~3ull) >= w0 && (a0 & ~3ull) + 20 <= w1) {
      // the whole unit inside one frame and its source window inside the wire: five aligned dwords
      const uint32_t* g = reinterpret_cast<const uint32_t*>(a0 & ~3ull);
      const uint32_t sh = static_cast<uint32_t>(a0 & 3u);
      const uint32_t x0 = g[0], x1 = g[1], x2 = g[2], x3 = g[3], x4 = sh ? g[4] : 0u;
      w[0] = __builtin_amdgcn_alignbyte(x1, x0, sh);
      w[1] = __builtin_amdgcn_alignbyte(x2, x1, sh);
      w[2] = __builtin_amdgcn_alignbyte(x3, x2, sh);
      w[3] = __builtin_amdgcn_alignbyte(x4, x3, sh);
    } else {
      for (uint32_t j = 0; j < nd; ++j) {
        const uint64_t d = d0 + 4u * j;
        while (d >= rend) {  // records are at least 12 bytes: at most two steps per unit
          ++r;
          ro = rend;
          rend = r + 1 < n ? rec_offsets[r + 1] : total;
          sl = src[r];
        }
        const uint64_t len = sl >> kSrcShift, q = d - ro;
        w[j] = q < len ? frame_dword(w0, w1, sl & ((1ull << kSrcShift) - 1), len, q) : 0u;
      }
    }
    if (nd == 4) {
      *reinterpret_cast<uint4*>(arena + d0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (uint32_t j = 0; j < nd; ++j) *reinterpret_cast<uint32_t*>(arena + d0 + 4u * j) = w[j];
    }
  }
}

}  // namespace

hipError_t launch_http_stream_frame(const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs, uint64_t n,
                                    const l7m_http_wire_meta* conn_meta, uint64_t* head_offs, uint32_t* head_conn,
                                    l7m_http_wire_meta* head_meta, uint64_t cap, int32_t* conn_status,
                                    uint64_t* conn_consumed, uint64_t* total, hipStream_t stream) {
  if (n == 0) {
    hipError_t e = hipMemsetAsync(total, 0, sizeof(uint64_t), stream);
    if (e == hipSuccess && head_offs)
      e = hipMemcpyAsync(head_offs, conn_offs, sizeof(uint64_t), hipMemcpyDeviceToDevice, stream);
    return e;
  }
  return tile_pipeline(  // beside the tile sums: counts, u32[n]
      n, {total}, n * sizeof(uint32_t), stream,
      [&](uint32_t tiles, uint64_t* tile_sums, void* counts) {
        stream_http_count<<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(
            wire, wire_bytes, conn_offs, n, conn_status, conn_consumed, static_cast<uint32_t*>(counts), tile_sums);
      },
      [&](uint32_t tiles, const uint64_t* tile_base, void* counts) {
        stream_http_emit<<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(
            wire, wire_bytes, conn_offs, n, conn_meta, head_offs, head_conn, head_meta, cap,
            static_cast<const uint32_t*>(counts), tile_base, total);
      });
}

hipError_t launch_kafka_stream_frame(const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs, uint64_t n,
                                     const uint32_t* conn_identity, uint8_t* arena, uint64_t cap_bytes,
                                     uint64_t* rec_offsets, uint32_t* rec_conn, uint32_t* src_identities,
                                     uint64_t cap_recs, int32_t* conn_status, uint64_t* conn_consumed,
                                     uint64_t* n_recs, uint64_t* arena_bytes, hipStream_t stream) {
  if (n == 0) {
    hipError_t e = hipMemsetAsync(n_recs, 0, sizeof(uint64_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(arena_bytes, 0, sizeof(uint64_t), stream);
    return e;
  }
  if (wire_bytes >> kSrcShift) return hipErrorInvalidValue;
  // what ascending offsets can yield, and no more than the caller's arrays hold
  const uint64_t bound = wire_bytes / 12;
  const uint64_t src_cap = cap_recs < bound ? cap_recs : bound;
  // two columns of tile sums (records, arena bytes); behind them sizes, u64[n]; src, u64[src_cap]; counts, u32[n]
  return tile_pipeline(
      n, {n_recs, arena_bytes}, (n + src_cap) * sizeof(uint64_t) + n * sizeof(uint32_t), stream,
      [&](uint32_t tiles, uint64_t* tile_sums, void* rest) {
        uint64_t *sizes = static_cast<uint64_t*>(rest), *src = sizes + n;
        uint32_t* counts = reinterpret_cast<uint32_t*>(src + src_cap);
        stream_kafka_count<<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(
            wire, wire_bytes, conn_offs, n, conn_status, conn_consumed, counts, sizes, tile_sums, tile_sums + tiles);
      },
      [&](uint32_t tiles, const uint64_t* tile_base, void* rest) {
        uint64_t *sizes = static_cast<uint64_t*>(rest), *src = sizes + n;
        uint32_t* counts = reinterpret_cast<uint32_t*>(src + src_cap);
        stream_kafka_emit<<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(
            wire, wire_bytes, conn_offs, n, conn_identity, rec_offsets, rec_conn, src_identities, cap_recs, cap_bytes,
            counts, sizes, tile_base, tile_base + tiles, src, src_cap, n_recs, arena_bytes);
        // the copy's grid from the capacity (the total is on the device): 16-byte units, at most 2048 workgroups
        const uint64_t abound = wire_bytes + wire_bytes / 4;
        const uint64_t units = ((cap_bytes < abound ? cap_bytes : abound) + 15) >> 4;
        if (units && src_cap) {
          uint64_t blocks = (units + kTileThreads - 1) / kTileThreads;
          if (blocks > 2048) blocks = 2048;
          stream_kafka_copy<<<dim3(static_cast<uint32_t>(blocks)), dim3(kTileThreads), 0, stream>>>(
              wire, wire_bytes, arena, cap_recs, cap_bytes, rec_offsets, src, src_cap, n_recs, arena_bytes);
        }
      });
}

// ---- streaming across calls (DESIGN.md "Streaming across calls") ----------
// The resumable HTTP framer is the one-shot's pipeline with a state per lane.
// conn_state_out may alias conn_state_in and the emit pass walks from the
// state the connection entered with, so the count pass leaves its result in
// the pipeline's scratch (`staged`) and the emit pass stores it, each lane
// after it has read its own entry.
//
// The carry is a measure / scan / emit pipeline over the connections (the
// next round's offsets and the updated states) and a copy kernel balanced
// over the next wire in 16-byte units, like stream_kafka_copy.  A connection
// has two sources, its tail in the wire and its segment; `CarrySrc` keeps
// where they start between the passes, because emit rewrites the state the
// plan was made from.
namespace {

__global__ __launch_bounds__(kTileThreads) void stream_http_resume_count(
    const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs, uint64_t n, int32_t* conn_status,
    uint64_t* conn_consumed, const l7m_stream_state* state_in, l7m_stream_state* staged, uint32_t* counts,
    uint64_t* tile_sums) {
  __shared__ uint64_t tmp[kTileThreads];
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  uint64_t cnt = 0;
  if (c < n) {
    const ClampedRange r = clamped_range(conn_offs, c, n, wire_bytes);
    l7m_stream_state st{0, 0, 0};
    if (state_in) st = state_in[c];
    uint64_t used = 0;
    const int32_t code =
        http_stream_walk_resume(ByteSrc{wire + r.lo}, r.hi - r.lo, st, &used, [&](uint64_t) { ++cnt; });
    conn_status[c] = code;
    conn_consumed[c] = used;
    staged[c] = st;
    counts[c] = static_cast<uint32_t>(cnt);  // <= (hi - lo) / 16 + 1
  }
  tile_sum_out(cnt, tmp, tile_sums);
}

__global__ __launch_bounds__(kTileThreads) void stream_http_resume_emit(
    const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs, uint64_t n,
    const l7m_http_wire_meta* conn_meta, uint64_t* head_offs, uint32_t* head_conn, l7m_http_wire_meta* head_meta,
    uint64_t cap, const l7m_stream_state* state_in, l7m_stream_state* state_out, const l7m_stream_state* staged,
    const uint32_t* counts, const uint64_t* tile_base, const uint64_t* total) {
  __shared__ uint64_t tmp[kTileThreads];
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint64_t cnt = c < n ? counts[c] : 0;
  const uint64_t base = tile_exclusive(cnt, tmp, tile_base);
  l7m_stream_state st{0, 0, 0};
  if (c < n) {
    if (state_in) st = state_in[c];  // before this lane's entry is overwritten
    state_out[c] = staged[c];
  }
  const uint64_t all = *total;
  if (all > cap || !head_offs) return;  // uniform: the per-head arrays stay untouched
  if (c >= n) return;
  const ClampedRange r = clamped_range(conn_offs, c, n, wire_bytes);
  if (c + 1 == n) head_offs[all] = r.hi;
  if (!cnt) return;
  l7m_http_wire_meta m{0, 0, 0, 1, {0, 0, 0}};  // no metadata: zeros, ingress
  if (conn_meta) m = conn_meta[c];
  uint64_t used = 0, k = 0;
  http_stream_walk_resume(ByteSrc{wire + r.lo}, r.hi - r.lo, st, &used, [&](uint64_t start) {
    if (k < cnt) {  // never more than the count pass counted
      head_offs[base + k] = r.lo + start;
      head_conn[base + k] = static_cast<uint32_t>(c);
      if (head_meta) head_meta[base + k] = m;
    }
    ++k;
  });
}

// Where the next round's connection comes from: tlen bytes at wire + tsrc,
// then the rest (its size less tlen) at seg + nsrc; `skip` body bytes of the
// segment were dropped in front of nsrc.
struct CarrySrc {
  uint64_t tsrc, tlen, nsrc, skip;
};

__device__ __forceinline__ CarryPlan carry_plan_of(uint64_t c, uint64_t wire_bytes, const uint64_t* conn_offs,
                                                   uint64_t n_prev, const int32_t* conn_status,
                                                   const uint64_t* conn_consumed, uint64_t seg_bytes,
                                                   const uint64_t* seg_offs, uint64_t n,
                                                   const l7m_stream_state* state) {
  const ClampedRange s = clamped_range(seg_offs, c, n, seg_bytes);
  l7m_stream_state st{0, 0, 0};
  if (state) st = state[c];
  if (c >= n_prev) return stream_carry_plan(0, 0, 0, L7M_STREAM_OK, s.lo, s.hi, st.mode, st.left);
  const ClampedRange r = clamped_range(conn_offs, c, n_prev, wire_bytes);
  uint64_t used = conn_consumed[c];
  if (used > r.hi - r.lo) used = r.hi - r.lo;
  return stream_carry_plan(r.lo, r.hi, used, conn_status[c], s.lo, s.hi, st.mode, st.left);
}

__global__ __launch_bounds__(kTileThreads) void stream_carry_measure(
    uint64_t wire_bytes, const uint64_t* conn_offs, uint64_t n_prev, const int32_t* conn_status,
    const uint64_t* conn_consumed, uint64_t seg_bytes, const uint64_t* seg_offs, uint64_t n,
    const l7m_stream_state* state, uint64_t* sizes, CarrySrc* srcs, uint64_t* tile_sums) {
  __shared__ uint64_t tmp[kTileThreads];
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  uint64_t size = 0;
  if (c < n) {
    const CarryPlan pl =
        carry_plan_of(c, wire_bytes, conn_offs, n_prev, conn_status, conn_consumed, seg_bytes, seg_offs, n, state);
    size = pl.tlen + pl.nlen;
    sizes[c] = size;
    srcs[c] = CarrySrc{pl.tsrc, pl.tlen, pl.nsrc, pl.skip};
  }
  tile_sum_out(size, tmp, tile_sums);
}

__global__ __launch_bounds__(kTileThreads) void stream_carry_emit(uint64_t n, l7m_stream_state* state,
                                                                  uint64_t* next_conn_offs, uint64_t cap_bytes,
                                                                  const uint64_t* sizes, const CarrySrc* srcs,
                                                                  const uint64_t* tile_base, const uint64_t* total) {
  __shared__ uint64_t tmp[kTileThreads];
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint64_t size = c < n ? sizes[c] : 0;
  const uint64_t off = tile_exclusive(size, tmp, tile_base);
  const uint64_t all = *total;
  if (all > cap_bytes || !next_conn_offs) return;  // uniform: nothing but the total is written
  if (c >= n) return;
  next_conn_offs[c] = off;
  if (c + 1 == n) next_conn_offs[n] = all;
  const uint64_t skip = srcs[c].skip;  // nonzero only with a state
  if (!skip) return;
  l7m_stream_state st = state[c];
  stream_carry_state(st, skip);
  state[c] = st;
}

// Byte d - co of the connection that starts at next-wire offset co.
__device__ __forceinline__ uint32_t carry_byte(const uint8_t* wire, const uint8_t* seg, const CarrySrc& s, uint64_t q) {
  return q < s.tlen ? wire[s.tsrc + q] : seg[s.nsrc + (q - s.tlen)];
}

__global__ __launch_bounds__(kTileThreads) void stream_carry_copy(const uint8_t* wire, uint64_t wire_bytes,
                                                                  const uint8_t* seg, uint64_t seg_bytes, uint64_t n,
                                                                  uint8_t* next_wire, uint64_t cap_bytes,
                                                                  const uint64_t* next_conn_offs,
                                                                  const CarrySrc* srcs, const uint64_t* next_bytes) {
  const uint64_t total = *next_bytes;
  if (total > cap_bytes || total == 0) return;
  const uint64_t units = (total + 15) >> 4;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kTileThreads;
  for (uint64_t u = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x; u < units; u += stride) {
    const uint64_t d0 = u << 4;
    // the connection that holds next-wire byte d0: the last one with next_conn_offs[c] <= d0
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (next_conn_offs[mid] <= d0) lo = mid;
      else hi = mid;
    }
    uint64_t c = lo, co = next_conn_offs[c], cend = next_conn_offs[c + 1];
    CarrySrc s = srcs[c];
    const uint32_t nb = total - d0 >= 16 ? 16u : static_cast<uint32_t>(total - d0);
    uint32_t w[4] = {0, 0, 0, 0};
    // the whole unit inside one source range of one connection?
    const uint64_t q0 = d0 - co;
    uint64_t a0 = 0, b0 = 0, b1 = 0;
    bool one = false;
    if (nb == 16 && d0 + 16 <= cend) {
      if (q0 + 16 <= s.tlen) {
        b0 = reinterpret_cast<uint64_t>(wire);
        b1 = b0 + wire_bytes;
        a0 = b0 + s.tsrc + q0;
        one = true;
      } else if (q0 >= s.tlen) {
        b0 = reinterpret_cast<uint64_t>(seg);
        b1 = b0 + seg_bytes;
        a0 = b0 + s.nsrc + (q0 - s.tlen);
        one = true;
      }
    }
    if (one && (a0 & ~3ull) >= b0 && (a0 & ~3ull) + 20 <= b1) {
      // and its aligned window inside that buffer: five aligned dwords
      const uint32_t* g = reinterpret_cast<const uint32_t*>(a0 & ~3ull);
      const uint32_t sh = static_cast<uint32_t>(a0 & 3u);
      const uint32_t x0 = g[0], x1 = g[1], x2 = g[2], x3 = g[3], x4 = sh ? g[4] : 0u;
      w[0] = __builtin_amdgcn_alignbyte(x1, x0, sh);
      w[1] = __builtin_amdgcn_alignbyte(x2, x1, sh);
      w[2] = __builtin_amdgcn_alignbyte(x3, x2, sh);
      w[3] = __builtin_amdgcn_alignbyte(x4, x3, sh);
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 16; ++j) {
        const uint64_t d = d0 + j;
        if (j < nb) {
          while (d >= cend) {  // d < total = next_conn_offs[n]: ends at a connection below n
            ++c;
            co = cend;
            cend = next_conn_offs[c + 1];
            s = srcs[c];
          }
          w[j >> 2] |= carry_byte(wire, seg, s, d - co) << (8u * (j & 3u));
        }
      }
    }
    if (nb == 16) {
      *reinterpret_cast<uint4*>(next_wire + d0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {  // the last unit: whole dwords, then bytes; nothing at or past the total
      for (uint32_t j = 0; j + 4 <= nb; j += 4) *reinterpret_cast<uint32_t*>(next_wire + d0 + j) = w[j >> 2];
      for (uint32_t j = nb & ~3u; j < nb; ++j) next_wire[d0 + j] = static_cast<uint8_t>(w[j >> 2] >> (8u * (j & 3u)));
    }
  }
}

}  // namespace

hipError_t launch_http_stream_frame_resume(const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs,
                                           uint64_t n, const l7m_http_wire_meta* conn_meta, uint64_t* head_offs,
                                           uint32_t* head_conn, l7m_http_wire_meta* head_meta, uint64_t cap,
                                           int32_t* conn_status, uint64_t* conn_consumed, uint64_t* total,
                                           const l7m_stream_state* state_in, l7m_stream_state* state_out,
                                           hipStream_t stream) {
  if (n == 0) {
    hipError_t e = hipMemsetAsync(total, 0, sizeof(uint64_t), stream);
    if (e == hipSuccess && head_offs)
      e = hipMemcpyAsync(head_offs, conn_offs, sizeof(uint64_t), hipMemcpyDeviceToDevice, stream);
    return e;
  }
  // beside the tile sums: the staged states, 16 bytes each; counts, u32[n]
  return tile_pipeline(
      n, {total}, n * (sizeof(l7m_stream_state) + sizeof(uint32_t)), stream,
      [&](uint32_t tiles, uint64_t* tile_sums, void* rest) {
        l7m_stream_state* staged = static_cast<l7m_stream_state*>(rest);
        stream_http_resume_count<<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(
            wire, wire_bytes, conn_offs, n, conn_status, conn_consumed, state_in, staged,
            reinterpret_cast<uint32_t*>(staged + n), tile_sums);
      },
      [&](uint32_t tiles, const uint64_t* tile_base, void* rest) {
        const l7m_stream_state* staged = static_cast<const l7m_stream_state*>(rest);
        stream_http_resume_emit<<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(
            wire, wire_bytes, conn_offs, n, conn_meta, head_offs, head_conn, head_meta, cap, state_in, state_out,
            staged, reinterpret_cast<const uint32_t*>(staged + n), tile_base, total);
      });
}

hipError_t launch_stream_carry(const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs, uint64_t n_prev,
                               const int32_t* conn_status, const uint64_t* conn_consumed, const uint8_t* seg,
                               uint64_t seg_bytes, const uint64_t* seg_offs, uint64_t n, l7m_stream_state* state,
                               uint8_t* next_wire, uint64_t cap_bytes, uint64_t* next_conn_offs, uint64_t* total,
                               hipStream_t stream) {
  if (n == 0) {
    hipError_t e = hipMemsetAsync(total, 0, sizeof(uint64_t), stream);
    if (e == hipSuccess && next_conn_offs) e = hipMemsetAsync(next_conn_offs, 0, sizeof(uint64_t), stream);
    return e;
  }
  // beside the tile sums: sizes, u64[n]; the sources, four u64 each
  return tile_pipeline(
      n, {total}, n * (sizeof(uint64_t) + sizeof(CarrySrc)), stream,
      [&](uint32_t tiles, uint64_t* tile_sums, void* rest) {
        uint64_t* sizes = static_cast<uint64_t*>(rest);
        stream_carry_measure<<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(
            wire_bytes, conn_offs, n_prev, conn_status, conn_consumed, seg_bytes, seg_offs, n, state, sizes,
            reinterpret_cast<CarrySrc*>(sizes + n), tile_sums);
      },
      [&](uint32_t tiles, const uint64_t* tile_base, void* rest) {
        const uint64_t* sizes = static_cast<const uint64_t*>(rest);
        stream_carry_emit<<<dim3(tiles), dim3(kTileThreads), 0, stream>>>(
            n, state, next_conn_offs, cap_bytes, sizes, reinterpret_cast<const CarrySrc*>(sizes + n), tile_base, total);
        // the copy's grid from the capacity (the total is on the device): 16-byte units, at most 2048 workgroups
        const uint64_t bound = wire_bytes + seg_bytes;
        const uint64_t units = ((cap_bytes < bound ? cap_bytes : bound) + 15) >> 4;
        if (units && next_conn_offs) {
          uint64_t blocks = (units + kTileThreads - 1) / kTileThreads;
          if (blocks > 2048) blocks = 2048;
          stream_carry_copy<<<dim3(static_cast<uint32_t>(blocks)), dim3(kTileThreads), 0, stream>>>(
              wire, wire_bytes, seg, seg_bytes, n, next_wire, cap_bytes, next_conn_offs,
              reinterpret_cast<const CarrySrc*>(sizes + n), total);
        }
      });
}

}  // namespace l7m
