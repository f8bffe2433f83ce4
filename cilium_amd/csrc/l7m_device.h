// l7m_device.h — launch entry points of the HIP kernels (l7m_kernels.hip,
// l7m_kafka.hip) used by the C ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <utility>

#include "../../include/l7match.h"
#include "program.h"

namespace l7m {

// Raise a kernel's dynamic-LDS limit (gfx950: up to 160 KiB per workgroup)
// once per (kernel, device), thread-safely: l7m_eval is reentrant and a rule
// set may be evaluated on several devices.  Returns the HIP status.
inline hipError_t set_lds_attr_once(const void* fn, uint32_t bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  // per-thread cache of the (kernel, device) pairs already done: the
  // batcher's flushers launch per batch and would contend on the mutex
  static thread_local const void* last_fn = nullptr;
  static thread_local int last_dev = -1;
  if (fn == last_fn && dev == last_dev) return hipSuccess;
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  std::lock_guard<std::mutex> g(mu);
  if (!done.count({fn, dev})) {
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
    if (e != hipSuccess) return e;
    done.insert({fn, dev});
  }
  last_fn = fn;
  last_dev = dev;
  return hipSuccess;
}

// Stream-ordered scratch (the slow pass's executor stacks, the search
// programs' code columns) comes from a PRIVATE memory pool per device, so
// the embedding process's default pool (its own hipMallocAsync behaviour) is
// left alone.  The private pool keeps up to 2 GiB mapped between
// launches instead of returning it at every synchronisation.  Falls back to
// the default pool (hipMallocAsync) if the runtime refuses to create one.
// Free with hipFreeAsync on the base pointer.
inline hipError_t scratch_alloc_async(void** p, size_t bytes, hipStream_t stream) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  static std::mutex mu;
  static std::map<int, hipMemPool_t> pools;
  hipMemPool_t pool = nullptr;
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = pools.find(dev);
    if (it == pools.end()) {
      hipMemPoolProps props;
      std::memset(&props, 0, sizeof props);
      props.allocType = hipMemAllocationTypePinned;
      props.handleTypes = hipMemHandleTypeNone;
      props.location.type = hipMemLocationTypeDevice;
      props.location.id = dev;
      if (hipMemPoolCreate(&pool, &props) == hipSuccess && pool) {
        uint64_t keep = 2ull << 30;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
      } else {
        pool = nullptr;
        (void)hipGetLastError();
      }
      pools[dev] = pool;  // nullptr: use the default pool
    } else {
      pool = it->second;
    }
  }
  return pool ? hipMallocFromPoolAsync(p, bytes, pool, stream) : hipMallocAsync(p, bytes, stream);
}

// LDS bytes of one HTTP workgroup with `stage` bytes of records per wave, and
// the stage the LDS leaves after the rule tables (0: the tables do not fit).
size_t http_lds_bytes(const HttpHeader& h, uint32_t stage);
uint32_t http_stage_bytes(const HttpHeader& h);
// Internal launch flag (beside the public L7M_FLAG_* bits): the program has
// literal tables (DfaDesc::lit_tab), so the kernel instantiation that uses
// them is launched.
constexpr uint32_t kLaunchLiterals = 1u << 29;  // L7M_FLAG_DIAG_* use bits 30, 31
// ... the program has dense automata (program.h kDfaDense): the instantiation
// that walks them (l7m_http_impl.h kFeatDense)
constexpr uint32_t kLaunchDense = 1u << 28;
// ... the program is of the lean class (l7m_dispatch.h http_program_lean,
// decided once when the rule set is created): the first pass runs the lean
// instantiation (l7m_http_impl.h kFeatLean)
constexpr uint32_t kLaunchLean = 1u << 27;
// (l7m_api.cc clears these from the flags a caller passes before it sets them)
constexpr uint32_t kLaunchInternal = kLaunchLiterals | kLaunchDense | kLaunchLean;
// Completion signal of a first-pass launch (the batcher's latency path):
// every wave, once its verdicts are visible system-wide, adds one to *ctr
// (device memory, zero between launches); the last one resets it and stores
// seq to *flag (pinned host memory, system scope), which the host polls
// instead of a HIP event.  Only for programs decided in one launch (no slow
// pass).
struct DoneSignal {
  uint32_t* ctr;
  uint32_t* flag;
  uint32_t seq;
};
// One batch as the verdict kernels see it: n records at offs[0..n) of the
// arena (device-visible addresses), one verdict each, the rule counters
// (nullptr: not counted) and the Kafka requests' source identities (nullptr:
// none).  Built once where a batch enters the launch path (l7m_api.cc
// batch_ref); every launcher below that only reads it.
struct BatchRef {
  const uint8_t* arena;
  uint64_t arena_bytes;
  const uint64_t* offs;
  uint64_t n;
  int32_t* verdicts;
  unsigned long long* hits;
  const uint32_t* ids;
};
// A decided batch, read-only: what the side-effect launchers (access log,
// proxy statistics, Kafka deny responses and log records) take.
struct BatchView {
  const uint8_t* arena;
  uint64_t arena_bytes;
  const uint64_t* offs;
  uint64_t n;
  const int32_t* verdicts;
};
// What a family's launcher (launch_http, launch_kafka) decides before it
// picks an instantiation: the first pass's grid, its dynamic LDS, the record
// stage per wave, the stream and the device program.  The per-instantiation
// launchers (launch_one, launch_slow, launch_k) only read it; launch_slow reads
// the stream and the program alone (the slow pass has its own grid and LDS).
struct LaunchPlan {
  dim3 grid;
  size_t lds;
  uint32_t stage;
  hipStream_t stream;
  const uint32_t* dprog;
};
// Persistent grid of a verdict kernel: per_cu workgroups of `block` threads
// per CU; fewer for small batches (>= 2 records per lane, two tiles per wave).
inline dim3 batch_grid(uint64_t n, int num_cus, uint32_t block, uint32_t per_cu = 1) {
  const uint64_t blocks = static_cast<uint64_t>(num_cus > 0 ? num_cus : 256) * per_cu;
  const uint64_t want = (n + 2 * block - 1) / (2 * block);
  return dim3(static_cast<uint32_t>(want < blocks ? want : blocks));
}
hipError_t launch_http(const uint32_t* dprog, const HttpHeader& h, const BatchRef& b, hipStream_t stream, int num_cus,
                       uint32_t flags, const DoneSignal* done = nullptr);
// The slow pass of launch_http (programs with kCrSlow rules): the two tiers'
// queues (count + up to n indices), executor scratch, workgroups and work
// counters ([0] tier 1, [64] tier 2), in one stream-ordered allocation.
struct HttpSlowPass {
  uint32_t* slowq = nullptr;
  uint32_t* slowq2 = nullptr;
  uint32_t* vms[2] = {nullptr, nullptr};
  uint32_t* work = nullptr;
  uint32_t blocks[2] = {0, 0};
};
// First-pass / slow-pass launches of the ECMAScript instantiations of feature
// set F (l7m_http_impl.h kFeat*): defined and explicitly instantiated in
// l7m_http_feat.hip, one translation unit per F < 4 holding F and F + 4.
// The definitions are deliberately not in a header: a use of any F in 0..7
// links against those four objects.
template <int F>
hipError_t launch_http_main(const LaunchPlan& p, const BatchRef& b, int mode, int R, bool lean, uint32_t* slowq,
                            DoneSignal done);
template <int F>
hipError_t launch_http_slow(const LaunchPlan& p, const HttpHeader& h, const BatchRef& b, const HttpSlowPass& s, int R,
                            int tier);

// HTTP/1.x request heads -> request arena (l7m_http_wire.hip): measure pass,
// scan and emit pass enqueued on `stream` by l7m_tile_scan.h's tile_pipeline,
// as in the four pipeline launchers after it; scratch from scratch_alloc_async.
// *total (u64) receives the arena bytes; nothing of `arena` is written when
// that exceeds cap.
hipError_t launch_http_wire(const uint8_t* wire, uint64_t wire_bytes, const uint64_t* head_offs, uint64_t n,
                            const l7m_http_wire_meta* meta, uint8_t* arena, uint64_t cap, uint64_t* rec_offsets,
                            int32_t* status, uint64_t* total, hipStream_t stream);

// HttpLogEntry messages of a decided batch (l7m_http_log.hip): measure pass,
// scan and emit pass enqueued on `stream`.  entry_offs (u64[n + 1]) and *total
// are always written; nothing of `out` is when the total exceeds cap.
struct LogConstsFixed;
hipError_t launch_http_log(const BatchView& b, const LogConstsFixed& c, uint32_t select, uint8_t* out, uint64_t cap,
                           uint64_t* entry_offs, uint64_t* total, hipStream_t stream);
// Request counters of a decided HTTP batch per (direction, port, verdict
// class) into host_counters (l7m_http_log.h kStatsCounters words; caller_row =
// ingress * 65536 + port for records that do not validate).  Synchronises
// `stream`.
hipError_t launch_http_stats(const BatchView& b, uint32_t caller_row, uint64_t* host_counters, hipStream_t stream);

// Deny responses (log = false: sizes and cap in bytes, `select` unused) or
// per-topic log records (log = true: in records) of a decided Kafka batch
// (l7m_kafka_side.hip): measure pass, scan and emit pass enqueued on `stream`.
// out_offs (u64[n + 1]) and *total are always written; nothing of `out` is
// when the total exceeds cap.
hipError_t launch_kafka_side(bool log, const BatchView& b, uint32_t select, uint8_t* out, uint64_t cap,
                             uint64_t* out_offs, uint64_t* total, hipStream_t stream);

// Connection byte streams -> head slices for the wire decoder, or Kafka
// records in a dword-aligned arena (l7m_stream_frame.hip): count pass, scan
// and emit pass (Kafka: two scans and a copy kernel) enqueued on `stream`.
// Statuses, consumed bytes and the totals (u64, device) are always written;
// nothing per head or record, and nothing of `arena`, when a total exceeds its
// capacity.
hipError_t launch_http_stream_frame(const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs, uint64_t n,
                                    const l7m_http_wire_meta* conn_meta, uint64_t* head_offs, uint32_t* head_conn,
                                    l7m_http_wire_meta* head_meta, uint64_t cap, int32_t* conn_status,
                                    uint64_t* conn_consumed, uint64_t* total, hipStream_t stream);
hipError_t launch_kafka_stream_frame(const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs, uint64_t n,
                                     const uint32_t* conn_identity, uint8_t* arena, uint64_t cap_bytes,
                                     uint64_t* rec_offsets, uint32_t* rec_conn, uint32_t* src_identities,
                                     uint64_t cap_recs, int32_t* conn_status, uint64_t* conn_consumed,
                                     uint64_t* n_recs, uint64_t* arena_bytes, hipStream_t stream);
// Streaming across calls (l7m_stream_frame.hip): the HTTP framer with a state
// per connection (state_out may alias state_in), and the next round's wire
// from the tails and the new segments: measure, scan, emit and a copy kernel.
// *total is always written; nothing else of the carry when it exceeds cap_bytes.
hipError_t launch_http_stream_frame_resume(const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs,
                                           uint64_t n, const l7m_http_wire_meta* conn_meta, uint64_t* head_offs,
                                           uint32_t* head_conn, l7m_http_wire_meta* head_meta, uint64_t cap,
                                           int32_t* conn_status, uint64_t* conn_consumed, uint64_t* total,
                                           const l7m_stream_state* state_in, l7m_stream_state* state_out,
                                           hipStream_t stream);
hipError_t launch_stream_carry(const uint8_t* wire, uint64_t wire_bytes, const uint64_t* conn_offs, uint64_t n_prev,
                               const int32_t* conn_status, const uint64_t* conn_consumed, const uint8_t* seg,
                               uint64_t seg_bytes, const uint64_t* seg_offs, uint64_t n, l7m_stream_state* state,
                               uint8_t* next_wire, uint64_t cap_bytes, uint64_t* next_conn_offs, uint64_t* total,
                               hipStream_t stream);

// Mailbox of a resident evaluator (l7m_kafka.hip kafka_resident_kernel),
// in pinned, device-mapped host memory.  The host fills slot seq %
// kResidentSlots, then raises post_seq to seq (release); the workgroup
// evaluates the slot and raises done_seq to seq.  Every field is read and
// written with system-scope atomics.
constexpr uint32_t kResidentSlots = 16;
constexpr uint32_t kResidentRound = 16;      // slots one resident round evaluates together (one per wave at most)
constexpr uint32_t kResidentLdsWords = 2 * (4 + 16 * kResidentRound);  // broadcast words at the end of its LDS
constexpr uint64_t kResidentIdleTicks = 2000000;  // 20 ms of s_memrealtime (100 MHz) without work: exit
constexpr uint64_t kResidentKafka = 16;          // kind of a Kafka slot: kResidentKafka | cli_lds | groups << 1
struct ResidentSlot {
  uint64_t kind;  // the instantiation: kResidentKafka | cli_lds | groups << 1
  uint64_t gen;   // program generation (a new program at a reused address reloads the image)
  uint64_t prog, arena, arena_bytes, offs, n, verdicts, stage, ids;
  uint64_t result;  // written by the workgroup: 1 = evaluate this batch again with the normal launches
  // written by the workgroup (s_memrealtime, 100 MHz): batch seen, slot read
  // and caches invalidated, batch evaluated, verdicts written back
  uint64_t stamp[4];
  uint64_t pad;
};
static_assert(sizeof(ResidentSlot) == 128, "the resident workgroup reads a slot as 16 words");
struct ResidentBox {
  alignas(64) uint64_t post_seq;
  alignas(64) uint64_t done_seq;
  alignas(64) uint64_t quit;
  alignas(64) uint64_t exited;  // set by the workgroup as it returns (cleared by the host before a launch)
  alignas(64) uint64_t rounds;  // rounds evaluated (statistics)
  alignas(64) ResidentSlot slots[kResidentSlots];
};
// Whether a Kafka program can be served by the resident evaluator, with
// which instantiation and record stage.
bool kafka_resident_ok(const KafkaHeader& h, int* kind, uint32_t* stage);
// Launch the resident workgroup of `kind` for slots first_seq, ...; qhdr: 16
// bytes of zeroed device memory (the Kafka instantiations' queue counter).
hipError_t launch_resident(ResidentBox* dbox, uint64_t first_seq, int kind, uint32_t* qhdr, hipStream_t stream);
hipError_t launch_kafka_resident(ResidentBox* dbox, uint64_t first_seq, int kind, uint32_t* qhdr,
                                 hipStream_t stream);

// Device scratch of the Kafka path's compressed-message second pass: the
// queue of request indices the first pass fills (header [0] pushed, [1] work
// counter, zeroed before each launch) and `workers` slabs of slab_bytes for
// decoded sets.
struct KafkaCodecQueue {
  uint32_t* recs = nullptr;
  uint32_t* qhdr = nullptr;
  uint32_t cap = 0;      // 0: every request with a compressed message reports -3
  uint32_t workers = 0;
  uint8_t* slabs = nullptr;
  uint64_t slab_bytes = 0;
};

hipError_t launch_kafka(const uint32_t* dprog, const KafkaHeader& h, const BatchRef& b, hipStream_t stream,
                        int num_cus, uint32_t flags, const KafkaCodecQueue& cq);
hipError_t launch_kafka_codec(const uint32_t* dprog, const BatchRef& b, hipStream_t stream, const KafkaCodecQueue& cq);

}  // namespace l7m
