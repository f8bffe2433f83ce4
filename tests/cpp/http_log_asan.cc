// Stand-alone check of the host access-log and proxy-statistics functions for
// sanitizer builds (no Python, no device):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tests/cpp/http_log_asan.cc cilium_amd/csrc/l7m_side.cc -o http_log_asan
//   python -c "import sys; sys.path[:0] = ['.', 'tests']; import http_log_cases as C; \
//              C.dump('log.bin', C.table_cases() + C.fuzz_cases(), **C.ALL_STRINGS)"
//   ./http_log_asan log.bin
// Reads the file http_log_cases.dump writes (the batch and the entries the
// Python encoder expects for the options below), holds the arena and every
// output in a heap block of its exact size so that a read or write one byte
// out of place is caught, and runs l7m_http_access_log as the sizing call, with
// the exact capacity and with one byte less, then l7m_proxy_stats_update.
// Exit status 0 and "OK" when everything agrees.
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
  if (argc < 2) return std::fprintf(stderr, "usage: %s log.bin\n", argv[0]), 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return std::perror(argv[1]), 2;
  auto take = [&](void* dst, size_t len) {
    if (len && std::fread(dst, 1, len, f) != len) std::exit(fail("short file", 0));
  };
  uint32_t n;
  uint64_t arena_bytes;
  take(&n, 4);
  take(&arena_bytes, 8);
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
  std::fclose(f);

  l7m_access_log_opts o;  // tests/http_log_cases.py ALL_STRINGS
  std::memset(&o, 0, sizeof o);
  o.struct_size = sizeof o;
  o.http_protocol = 1;
  o.timestamp_ns = 1700000000000ull;
  o.policy_name = "ep-7";
  o.local_identity = 99;
  o.source_address = "10.1.2.3:1";
  o.destination_address = "10.9.8.7:80";

  // sizing call
  uint64_t* eo = exact<uint64_t>(n + 1);
  int64_t rc = l7m_http_access_log(arena, arena_bytes, offs, n, verdicts, &o, nullptr, 0, eo);
  if (rc != static_cast<int64_t>(want_total)) return fail("sizing call", 0);
  for (size_t i = 0; i <= n; ++i)
    if (eo[i] != want_offs[i]) return fail("entry offsets of the sizing call", i);
  std::free(eo);

  // exactly enough
  eo = exact<uint64_t>(n + 1);
  uint8_t* out = exact<uint8_t>(want_total);
  rc = l7m_http_access_log(arena, arena_bytes, offs, n, verdicts, &o, out, want_total, eo);
  if (rc != static_cast<int64_t>(want_total)) return fail("exact capacity", 0);
  for (size_t i = 0; i < n; ++i)
    if (eo[i] != want_offs[i] || std::memcmp(out + eo[i], want.data() + eo[i], want_offs[i + 1] - want_offs[i]) != 0)
      return fail("entry", i);
  std::free(out);
  std::free(eo);

  // one byte short: L7M_ENOMEM, the offsets complete, the entries that fit written
  if (want_total) {
    eo = exact<uint64_t>(n + 1);
    out = exact<uint8_t>(want_total - 1);
    rc = l7m_http_access_log(arena, arena_bytes, offs, n, verdicts, &o, out, want_total - 1, eo);
    if (rc != L7M_ENOMEM) return fail("short capacity", 0);
    for (size_t i = 0; i <= n; ++i)
      if (eo[i] != want_offs[i]) return fail("entry offsets with a short capacity", i);
    for (size_t i = 0; i < n; ++i)
      if (want_offs[i + 1] <= want_total - 1 &&
          std::memcmp(out + eo[i], want.data() + eo[i], want_offs[i + 1] - want_offs[i]) != 0)
        return fail("entry with a short capacity", i);
    std::free(out);
    std::free(eo);
  }

  // statistics: every request counted once, whatever its record looks like
  l7m_proxy_stats_table* t = l7m_proxy_stats_table_create();
  if (!t || l7m_proxy_stats_update(t, L7M_PROTO_HTTP, arena, arena_bytes, offs, verdicts, n, 4242, 0) != L7M_OK)
    return fail("stats update", 0);
  const size_t rows = l7m_proxy_stats_get(t, nullptr, 0);
  l7m_proxy_stats_entry* e = exact<l7m_proxy_stats_entry>(rows);
  if (l7m_proxy_stats_get(t, e, rows) != rows) return fail("stats get", 0);
  uint64_t received = 0, classes = 0;
  for (size_t k = 0; k < rows; ++k) {
    received += e[k].stats.received;
    classes += e[k].stats.forwarded + e[k].stats.denied + e[k].stats.error;
  }
  if (received != n || classes != n) return fail("stats total", 0);
  std::free(e);
  l7m_proxy_stats_table_destroy(t);

  std::free(verdicts);
  std::free(arena);
  std::free(offs);
  std::printf("OK: %u requests, %llu entry bytes, %zu statistics rows\n", n,
              static_cast<unsigned long long>(want_total), rows);
  return 0;
}
