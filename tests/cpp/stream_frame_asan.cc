// Stand-alone check of the host stream framers for sanitizer builds (no
// Python, no device):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tests/cpp/stream_frame_asan.cc cilium_amd/csrc/stream_frame.cc cilium_amd/csrc/http_wire.cc \
//       -o stream_frame_asan
//   python -c "import sys; sys.path[:0] = ['.', 'tests']; import stream_cases as S; \
//              S.dump('stream_frame.bin', [S.http_table_conns(), S.fuzz_http_conns()], \
//                     [S.kafka_table_conns(), S.fuzz_kafka_conns()])"
//   ./stream_frame_asan stream_frame.bin
// Reads the file stream_cases.dump writes (connection sets of both protocols
// with the outputs the Python framer expects), holds the wire and every output
// in a heap block of its exact size so that a read or write one byte out of
// place is caught, and runs each framer as the sizing call, with the exact
// capacity and one head / one record / one byte short; the slices of the exact
// HTTP call also go through l7m_http_wire_decode.  Exit status 0 and "OK" when
// everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "l7match.h"

static int fail(const char* what, size_t set) {
  std::fprintf(stderr, "FAIL: %s (set %zu)\n", what, set);
  return 1;
}

template <class T>
static T* exact(size_t count) {  // a heap block of exactly count elements (one byte for none), sentinel-filled
  const size_t bytes = count ? count * sizeof(T) : 1;
  void* p = std::malloc(bytes);
  std::memset(p, 0xA5, bytes);
  return static_cast<T*>(p);
}

template <class T>
static bool untouched(const T* p, size_t count) {
  const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
  for (size_t i = 0; i < count * sizeof(T); ++i)
    if (b[i] != 0xA5) return false;
  return true;
}

template <class T>
static bool same(const T* p, const std::vector<T>& want) {
  return want.empty() || std::memcmp(p, want.data(), want.size() * sizeof(T)) == 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return std::fprintf(stderr, "usage: %s stream_frame.bin\n", argv[0]), 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return std::perror(argv[1]), 2;
  auto take = [&](void* dst, size_t len) {
    if (len && std::fread(dst, 1, len, f) != len) std::exit(fail("short file", 0));
  };
  size_t sets = 0, conns = 0, slices = 0;
  uint32_t hdr[2];
  while (std::fread(hdr, 4, 2, f) == 2) {
    const uint32_t proto = hdr[0], nc = hdr[1];
    uint64_t* coffs = exact<uint64_t>(nc + 1);
    take(coffs, 8ull * (nc + 1));
    const size_t wire_bytes = coffs[nc];
    uint8_t* wire = exact<uint8_t>(wire_bytes);
    take(wire, wire_bytes);
    std::vector<int32_t> want_status(nc);
    std::vector<uint64_t> want_consumed(nc);
    take(want_status.data(), 4ull * nc);
    take(want_consumed.data(), 8ull * nc);
    uint64_t n;
    take(&n, 8);
    int32_t* status = exact<int32_t>(nc);
    uint64_t* consumed = exact<uint64_t>(nc);
    auto conn_outputs_ok = [&] { return same(status, want_status) && same(consumed, want_consumed); };
    if (proto == 1) {
      std::vector<uint64_t> want_offs(n + 1);
      std::vector<uint32_t> want_conn(n);
      take(want_offs.data(), 8 * (n + 1));
      take(want_conn.data(), 4 * n);
      if (n > l7m_http_stream_heads_bound(wire_bytes, nc)) return fail("heads bound", sets);
      size_t got = 99;
      int rc = l7m_http_stream_frame(wire, wire_bytes, coffs, nc, nullptr, nullptr, nullptr, nullptr, 0, status,
                                     consumed, &got);
      if (rc != (n ? L7M_ENOMEM : L7M_OK) || got != n || !conn_outputs_ok()) return fail("http sizing call", sets);
      for (size_t cap : {static_cast<size_t>(n), static_cast<size_t>(n ? n - 1 : 0)}) {
        uint64_t* offs = exact<uint64_t>(cap + 1);
        uint32_t* hconn = exact<uint32_t>(cap);
        l7m_http_wire_meta* hmeta = exact<l7m_http_wire_meta>(cap);
        std::memset(status, 0xA5, 4ull * nc);
        std::memset(consumed, 0xA5, 8ull * nc);
        got = 99;
        rc = l7m_http_stream_frame(wire, wire_bytes, coffs, nc, nullptr, offs, hconn, hmeta, cap, status, consumed, &got);
        if (got != n || !conn_outputs_ok()) return fail("http totals", sets);
        if (cap == n) {
          if (rc != L7M_OK || !same(offs, want_offs) || !same(hconn, want_conn)) return fail("http exact capacity", sets);
          for (size_t i = 0; i < n; ++i)
            if (hmeta[i].ingress != 1 || hmeta[i].remote_id != 0) return fail("http default meta", sets);
          // the slices are what the decoder takes
          const size_t acap = l7m_http_wire_arena_bound(wire_bytes, n);
          uint8_t* arena = exact<uint8_t>(acap);
          uint64_t* roffs = exact<uint64_t>(n);
          int32_t* wstatus = exact<int32_t>(n);
          size_t used = 0;
          if (l7m_http_wire_decode(wire, wire_bytes, offs, n, hmeta, arena, acap, roffs, wstatus, &used) != L7M_OK)
            return fail("decode of the slices", sets);
          std::free(arena);
          std::free(roffs);
          std::free(wstatus);
        } else if (n) {
          if (rc != L7M_ENOMEM || !untouched(offs, cap + 1) || !untouched(hconn, cap) || !untouched(hmeta, cap))
            return fail("http one head short", sets);
        }
        std::free(offs);
        std::free(hconn);
        std::free(hmeta);
      }
    } else {
      uint64_t nb;
      take(&nb, 8);
      std::vector<uint64_t> want_offs(n);
      std::vector<uint32_t> want_conn(n);
      std::vector<uint8_t> want_arena(nb);
      take(want_offs.data(), 8 * n);
      take(want_conn.data(), 4 * n);
      take(want_arena.data(), nb);
      if (n > l7m_kafka_stream_records_bound(wire_bytes) || nb > l7m_kafka_stream_arena_bound(wire_bytes))
        return fail("kafka bounds", sets);
      size_t got = 99, gotb = 99;
      int rc = l7m_kafka_stream_frame(wire, wire_bytes, coffs, nc, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0,
                                      status, consumed, &got, &gotb);
      if (rc != (n ? L7M_ENOMEM : L7M_OK) || got != n || gotb != nb || !conn_outputs_ok())
        return fail("kafka sizing call", sets);
      const size_t caps[3][2] = {{static_cast<size_t>(n), static_cast<size_t>(nb)},
                                 {static_cast<size_t>(n ? n - 1 : 0), static_cast<size_t>(nb)},
                                 {static_cast<size_t>(n), static_cast<size_t>(nb ? nb - 1 : 0)}};
      for (const auto& cap : caps) {
        uint8_t* arena = exact<uint8_t>(cap[1]);
        uint64_t* offs = exact<uint64_t>(cap[0]);
        uint32_t* rconn = exact<uint32_t>(cap[0]);
        uint32_t* sids = exact<uint32_t>(cap[0]);
        std::memset(status, 0xA5, 4ull * nc);
        std::memset(consumed, 0xA5, 8ull * nc);
        got = gotb = 99;
        rc = l7m_kafka_stream_frame(wire, wire_bytes, coffs, nc, nullptr, arena, cap[1], offs, rconn, sids, cap[0],
                                    status, consumed, &got, &gotb);
        if (got != n || gotb != nb || !conn_outputs_ok()) return fail("kafka totals", sets);
        if (cap[0] == n && cap[1] == nb) {
          if (rc != L7M_OK || !same(offs, want_offs) || !same(rconn, want_conn) || !same(arena, want_arena))
            return fail("kafka exact capacity", sets);
          for (size_t i = 0; i < n; ++i)
            if (sids[i] != 0) return fail("kafka default identity", sets);
        } else {
          if (rc != L7M_ENOMEM || !untouched(arena, cap[1]) || !untouched(offs, cap[0]) || !untouched(rconn, cap[0]) ||
              !untouched(sids, cap[0]))
            return fail("kafka one short", sets);
        }
        std::free(arena);
        std::free(offs);
        std::free(rconn);
        std::free(sids);
      }
    }
    std::free(coffs);
    std::free(wire);
    std::free(status);
    std::free(consumed);
    ++sets;
    conns += nc;
    slices += n;
  }
  std::fclose(f);
  std::printf("OK: %zu sets, %zu connections, %zu heads and records\n", sets, conns, slices);
  return 0;
}
