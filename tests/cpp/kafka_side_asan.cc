// Stand-alone check of the host Kafka deny-response and log-record functions
// for sanitizer builds (no Python, no device):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tests/cpp/kafka_side_asan.cc cilium_amd/csrc/l7m_side.cc -o kafka_side_asan
//   python -c "import sys; sys.path[:0] = ['.', 'tests']; import kafka_side_cases as C; \
//              C.dump('kafka_side.bin', C.table_cases() + C.fuzz_cases())"
//   ./kafka_side_asan kafka_side.bin
// Reads the file kafka_side_cases.dump writes (the batch, records back to back
// with no padding, the responses and the log records expected for it), holds
// the arena and every output in a heap block of its exact size so that a read
// or write one byte out of place is caught, and runs
// l7m_kafka_deny_responses as the sizing call, with the exact capacity and
// with one byte less, l7m_kafka_deny_response on every record of the arena,
// l7m_kafka_access_log the same three ways and l7m_proxy_stats_update.  Exit
// status 0 and "OK" when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "l7match.h"

static int fail(const char* what, size_t i) {
  std::fprintf(stderr, "FAIL: %s (request %zu)\n", what, i);
  return 1;
}

template <class T>
static T* exact(size_t count) {  // a heap block of exactly count elements (one byte for none)
  return static_cast<T*>(std::malloc(count ? count * sizeof(T) : 1));
}

int main(int argc, char** argv) {
  if (argc < 2) return std::fprintf(stderr, "usage: %s kafka_side.bin\n", argv[0]), 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return std::perror(argv[1]), 2;
  auto take = [&](void* dst, size_t len) {
    if (len && std::fread(dst, 1, len, f) != len) std::exit(fail("short file", 0));
  };
  uint32_t n;
  uint64_t arena_bytes, want_recs;
  take(&n, 4);
  take(&arena_bytes, 8);
  take(&want_recs, 8);
  uint64_t* offs = exact<uint64_t>(n);
  take(offs, 8ull * n);
  uint8_t* arena = exact<uint8_t>(arena_bytes);
  take(arena, arena_bytes);
  int32_t* verdicts = exact<int32_t>(n);
  take(verdicts, 4ull * n);
  std::vector<uint64_t> want_offs(n + 1);
  take(want_offs.data(), 8ull * (n + 1));
  const uint64_t want_total = want_offs[n];
  std::vector<uint8_t> want(want_total);
  take(want.data(), want_total);
  std::vector<l7m_kafka_log_record> want_log(want_recs);
  take(want_log.data(), want_recs * sizeof(l7m_kafka_log_record));
  std::fclose(f);

  // ---- responses: sizing call
  uint64_t* ro = exact<uint64_t>(n + 1);
  int64_t rc = l7m_kafka_deny_responses(arena, arena_bytes, offs, n, verdicts, nullptr, 0, ro);
  if (rc != static_cast<int64_t>(want_total)) return fail("sizing call", 0);
  for (size_t i = 0; i <= n; ++i)
    if (ro[i] != want_offs[i]) return fail("response offsets of the sizing call", i);
  std::free(ro);

  // exactly enough
  ro = exact<uint64_t>(n + 1);
  uint8_t* out = exact<uint8_t>(want_total);
  rc = l7m_kafka_deny_responses(arena, arena_bytes, offs, n, verdicts, out, want_total, ro);
  if (rc != static_cast<int64_t>(want_total)) return fail("exact capacity", 0);
  for (size_t i = 0; i < n; ++i)
    if (ro[i] != want_offs[i] || std::memcmp(out + ro[i], want.data() + ro[i], want_offs[i + 1] - want_offs[i]) != 0)
      return fail("response", i);
  std::free(out);
  std::free(ro);

  // one byte short: L7M_ENOMEM, the offsets complete, the responses that fit written
  if (want_total) {
    ro = exact<uint64_t>(n + 1);
    out = exact<uint8_t>(want_total - 1);
    rc = l7m_kafka_deny_responses(arena, arena_bytes, offs, n, verdicts, out, want_total - 1, ro);
    if (rc != L7M_ENOMEM) return fail("short capacity", 0);
    for (size_t i = 0; i <= n; ++i)
      if (ro[i] != want_offs[i]) return fail("response offsets with a short capacity", i);
    for (size_t i = 0; i < n; ++i)
      if (want_offs[i + 1] <= want_total - 1 &&
          std::memcmp(out + ro[i], want.data() + ro[i], want_offs[i + 1] - want_offs[i]) != 0)
        return fail("response with a short capacity", i);
    std::free(out);
    std::free(ro);
  }

  // the per-request function on every record that lies in the arena, the
  // record copied to a block of its own size, the response into one of its size
  size_t singles = 0;
  for (size_t i = 0; i < n; ++i) {
    if (offs[i] > arena_bytes || arena_bytes - offs[i] < 4) continue;
    const uint8_t* p = arena + offs[i];
    const uint64_t sz = static_cast<uint64_t>(p[0]) << 24 | static_cast<uint64_t>(p[1]) << 16 |
                        static_cast<uint64_t>(p[2]) << 8 | p[3];
    if (sz > arena_bytes - offs[i] - 4) continue;
    uint8_t* rec = exact<uint8_t>(sz + 4);
    std::memcpy(rec, p, sz + 4);
    size_t len = 0;
    int r = l7m_kafka_deny_response(rec, sz + 4, nullptr, 0, &len);
    const uint64_t want_len = want_offs[i + 1] - want_offs[i];
    if (verdicts[i] == L7M_VERDICT_DENY && (r == L7M_ENOMEM ? len : 0) != want_len) return fail("single size", i);
    if (r == L7M_ENOMEM) {
      uint8_t* one = exact<uint8_t>(len);
      r = l7m_kafka_deny_response(rec, sz + 4, one, len, &len);
      if (r != L7M_OK) return fail("single response", i);
      if (verdicts[i] == L7M_VERDICT_DENY && std::memcmp(one, want.data() + want_offs[i], len) != 0)
        return fail("single response bytes", i);
      std::free(one);
      ++singles;
    }
    std::free(rec);
  }

  // ---- log records: the count, exactly enough, one record short
  rc = l7m_kafka_access_log(arena, arena_bytes, offs, n, verdicts, nullptr, 0);
  if (rc != static_cast<int64_t>(want_recs)) return fail("record count", 0);
  l7m_kafka_log_record* recs = exact<l7m_kafka_log_record>(want_recs);
  rc = l7m_kafka_access_log(arena, arena_bytes, offs, n, verdicts, recs, want_recs);
  if (rc != static_cast<int64_t>(want_recs)) return fail("records with the exact capacity", 0);
  for (size_t k = 0; k < want_recs; ++k)
    if (std::memcmp(&recs[k], &want_log[k], sizeof recs[k]) != 0) return fail("record", recs[k].request);
  std::free(recs);
  if (want_recs) {
    recs = exact<l7m_kafka_log_record>(want_recs - 1);
    rc = l7m_kafka_access_log(arena, arena_bytes, offs, n, verdicts, recs, want_recs - 1);
    if (rc != L7M_ENOMEM) return fail("records with a short capacity", 0);
    for (size_t k = 0; k + 1 < want_recs; ++k)
      if (std::memcmp(&recs[k], &want_log[k], sizeof recs[k]) != 0) return fail("record with a short capacity", k);
    std::free(recs);
  }

  // ---- statistics: a request is counted unless ReadRequest rejected it
  l7m_proxy_stats_table* t = l7m_proxy_stats_table_create();
  if (!t || l7m_proxy_stats_update(t, L7M_PROTO_KAFKA, arena, arena_bytes, offs, verdicts, n, 9092, 1) != L7M_OK)
    return fail("stats update", 0);
  l7m_proxy_stats_entry e[2];
  if (l7m_proxy_stats_get(t, e, 2) != 1) return fail("stats rows", 0);
  uint64_t counted = 0;
  for (size_t i = 0; i < n; ++i) counted += verdicts[i] != L7M_VERDICT_PARSE_ERROR;
  if (e[0].stats.received != counted || e[0].stats.forwarded + e[0].stats.denied + e[0].stats.error != counted)
    return fail("stats total", 0);
  l7m_proxy_stats_table_destroy(t);

  std::free(verdicts);
  std::free(arena);
  std::free(offs);
  std::printf("OK: %u requests, %llu response bytes, %zu per-request responses, %llu log records\n", n,
              static_cast<unsigned long long>(want_total), singles, static_cast<unsigned long long>(want_recs));
  return 0;
}
