// l7m_kernels.hip — CDNA4 (gfx950) kernel of the batched HTTP verdict path.
//
// Persistent layout: one 1024-thread workgroup (16 waves) per CU.  Each wave
// owns a contiguous range of the batch and consumes it in tiles of up to 64
// consecutive records (one lane per record):
//   1. the tile's byte window [off_first, end_last) is copied HBM -> the
//      wave's LDS stage with coalesced 16-byte non-temporal loads (the arena is
//      streamed exactly once; the tile is cut short so the window fits);
//   2. walk phase: every referenced field (method / path / authority / values
//      of headers whose lower-cased name a rule references) is walked through
//      its packed DFA groups (dfa_pack.h) in one loop of walk jobs: one
//      dependent 4-byte LDS read per input byte, tables copied to LDS once per
//      workgroup;
//   3. the next tile's bytes are requested;
//   4. verification phase: the end codes select precomputed candidate rule
//      lists (L2-resident); the first rule (input order) whose other
//      matchers hold is the verdict.
// A record that is not inside its tile window (non-contiguous offsets, a
// record larger than the stage, malformed lengths) is evaluated by the same
// code reading HBM directly.
// Reference semantics: NetworkPolicyMap::Allowed -> PortNetworkPolicyRule::
// Matches -> HttpNetworkPolicyRule::Matches -> ConfigUtility::matchHeaders
// (envoy/cilium_network_policy.h:68-237).
#include "l7m_dispatch.h"
#include "l7m_http_impl.h"

namespace l7m {

size_t http_lds_bytes(const HttpHeader& h, uint32_t stage) {
  const bool reg = h.n_dfas <= kRegDfas || h.search;  // search programs: codes in global scratch
  const size_t ctr = h.n_rules + 2 <= kMaxLdsCounters ? ((h.n_rules + 2 + 3) & ~size_t(3)) : 0;
  return 4u * (static_cast<size_t>(h.lds_image_words) + ctr + (reg ? 0u : static_cast<size_t>(h.n_dfas) * kBlock)) +
         static_cast<size_t>(kWaves) * (stage + 16u);
}

// Bytes of records staged per wave: what is left of the LDS after the tables.
uint32_t http_stage_bytes(const HttpHeader& h) {
  const size_t fixed = http_lds_bytes(h, 0) - kWaves * 16u;
  if (fixed + kWaves * (256u + 16u) > kHttpLdsBytes) return 0;
  size_t s = (kHttpLdsBytes - fixed) / kWaves - 16u;
  s &= ~size_t(15);
  return static_cast<uint32_t>(s > kMaxStage ? kMaxStage : s);
}

hipError_t launch_resident(ResidentBox* dbox, uint64_t first_seq, int kind, uint32_t* qhdr, hipStream_t stream) {
  return launch_kafka_resident(dbox, first_seq, kind, qhdr, stream);
}

hipError_t launch_http(const uint32_t* dprog, const HttpHeader& h, const BatchRef& b, hipStream_t stream, int num_cus,
                       uint32_t flags, const DoneSignal* done) {
  const uint64_t n = b.n;
  if (n == 0) return hipSuccess;
  const uint32_t stage = http_stage_bytes(h);
  if (stage == 0) return hipErrorInvalidValue;
  // kHttpWgPerCu resident workgroups per CU (1 by default)
  const LaunchPlan p{batch_grid(n, num_cus, kBlock, kHttpWgPerCu), http_lds_bytes(h, stage), stage, stream, dprog};
  const bool reg = h.n_dfas <= kRegDfas;
  if (flags & (L7M_FLAG_DIAG_WALK_ONLY | L7M_FLAG_DIAG_COPY_ONLY)) {  // diagnostic ablations
    // (register end codes only; no search or dense automata, no slow-path queue)
    if (!reg || h.search || h.n_slow || (flags & kLaunchDense)) return hipErrorInvalidValue;
    if (flags & L7M_FLAG_DIAG_COPY_ONLY) return launch_one<kNoHits, 8, 2>(p, b);
    return launch_one<kNoHits, 8, 1>(p, b);
  }
  const int mode = !b.hits ? kNoHits : (h.n_rules + 2 <= kMaxLdsCounters ? kLdsHits : kGlobalHits);
  if (h.search) {
    // RE2-dialect programs (search automata, program.h kDfaSearch): their own
    // instantiation, end codes in a stream-ordered global scratch column per
    // thread (n_dfas words each)
    uint32_t* scratch = nullptr;
    const size_t bytes = static_cast<size_t>(h.n_dfas ? h.n_dfas : 1) * p.grid.x * kBlock * 4u;
    hipError_t e = scratch_alloc_async(reinterpret_cast<void**>(&scratch), bytes, stream);
    if (e != hipSuccess) return e;
    const DoneSignal sig = done ? *done : DoneSignal{nullptr, nullptr, 0};
    e = dispatch_values<int, kNoHits, kLdsHits, kGlobalHits>(mode, hipErrorInvalidValue, [&](auto M) {
      return launch_one<decltype(M)::value, -1>(p, b, scratch, nullptr, sig);
    });
    const hipError_t e2 = hipFreeAsync(scratch, stream);
    return e != hipSuccess ? e : e2;
  }
  // end codes in 4 or 8 registers, or in LDS columns
  const bool lit = (flags & kLaunchLiterals) != 0;
  const int R = h.n_dfas <= 4 ? 4 : reg ? 8 : 0;
  // programs with slow-path rules (program.h kCrSlow): the first pass queues
  // the requests they may decide, http_slow_kernel decides them; the queue
  // (count + up to n indices) and the executor scratch are stream-ordered
  HttpSlowPass s;
  const size_t qbytes = (4ull * (n + 1) + 255) & ~size_t(255);
  // tier 1: kSlowWavesPerCu waves per CU (fewer for small batches), tier 2: kSlowBlocks2 waves
  const uint64_t waves = (n + kSlowBlock - 1) / kSlowBlock;
  const uint64_t w1 = static_cast<uint64_t>(num_cus > 0 ? num_cus : 256) * kSlowWavesPerCu;
  s.blocks[0] = static_cast<uint32_t>(waves < w1 ? waves : w1);
  s.blocks[1] = static_cast<uint32_t>(waves < kSlowBlocks2 ? waves : kSlowBlocks2);
  void* buf = nullptr;  // the one stream-ordered allocation of the slow pass (freed by its base)
  if (h.n_slow) {
    const size_t v1 = static_cast<size_t>(s.blocks[0]) * kSlowBlock * kVmScratchWords * 4u;
    const size_t v2 = static_cast<size_t>(s.blocks[1]) * kSlowBlock * kVmScratchWords2 * 4u;
    hipError_t e = scratch_alloc_async(&buf, 512 + 2 * qbytes + v1 + v2, stream);
    if (e == hipSuccess) e = hipMemsetAsync(buf, 0, 512, stream);
    if (e == hipSuccess) e = hipMemsetAsync(static_cast<uint8_t*>(buf) + 512, 0, 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(static_cast<uint8_t*>(buf) + 512 + qbytes, 0, 4, stream);
    if (e != hipSuccess) {
      if (buf) (void)hipFreeAsync(buf, stream);
      return e;
    }
    s.work = static_cast<uint32_t*>(buf);
    s.slowq = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(buf) + 512);
    s.slowq2 = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(buf) + 512 + qbytes);
    s.vms[0] = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(buf) + 512 + 2 * qbytes);
    s.vms[1] = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(buf) + 512 + 2 * qbytes + v1);
  }
  // the instantiation with the program's features (literal tables, forced
  // captures, dense automata); l7m_http_feat.hip compiles one translation
  // unit per literal / capture set, holding it and its dense twin (+ 4)
  const int feat = (lit ? kFeatLit : 0) | (h.lds_dcap != kNone ? kFeatDcap : 0) |
                   ((flags & kLaunchDense) ? kFeatDense : 0);
  // the completion signal only where this launch decides every request
  const DoneSignal sig = done && !h.n_slow ? *done : DoneSignal{nullptr, nullptr, 0};
  const bool lean = (flags & kLaunchLean) != 0;  // the lean kernels of the plain feature set; an error for any other
  hipError_t e = dispatch_values<int, 0, 1, 2, 3, 4, 5, 6, 7>(feat, hipErrorInvalidValue, [&](auto F) {
    hipError_t r = launch_http_main<decltype(F)::value>(p, b, mode, R, lean, s.slowq, sig);
    for (int tier = 1; h.n_slow && tier <= 2 && r == hipSuccess; ++tier)
      r = launch_http_slow<decltype(F)::value>(p, h, b, s, R, tier);
    return r;
  });
  if (h.n_slow) {
    const hipError_t e2 = hipFreeAsync(buf, stream);
    if (e == hipSuccess) e = e2;
  }
  return e;
}

}  // namespace l7m

// The tile pipelines (l7m_tile_scan.h), same code object: HTTP wire decoder and access log;
#include "l7m_http_wire.hip"
#include "l7m_http_log.hip"
// the Kafka deny-response and log-record encoders (l7m_http_log.hip's LogOutSink);
#include "l7m_kafka_side.hip"
// connection byte streams -> head slices / Kafka records.
#include "l7m_stream_frame.hip"
