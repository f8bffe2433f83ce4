// Stand-alone check of the host HTTP/1.x wire decoder for sanitizer builds:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tests/cpp/http_wire_asan.cc cilium_amd/csrc/http_wire.cc -o http_wire_asan
//   python -c "import sys; sys.path[:0] = ['.', 'tests']; import http_wire_cases as C; \
//              C.dump('heads.bin', C.table_heads() + C.fuzz_heads())"
//   ./http_wire_asan heads.bin
// Reads the file http_wire_cases.dump writes (heads and the Python decoder's
// answer), copies every buffer to its exact size on the heap so that a read or
// write one byte out of place is caught, decodes the batch as a whole, head by
// head and with a capacity one byte short, encodes the arena back and decodes
// that again.  Exit status 0 and "OK" when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "l7match.h"

static int fail(const char* what, size_t i) {
  std::fprintf(stderr, "FAIL: %s (head %zu)\n", what, i);
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 2) return std::fprintf(stderr, "usage: %s heads.bin\n", argv[0]), 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return std::perror(argv[1]), 2;
  std::vector<uint8_t> file;
  uint8_t buf[65536];
  for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
  std::fclose(f);
  size_t p = 0;
  auto take = [&](void* dst, size_t len) {
    if (p + len > file.size()) std::exit(fail("short file", 0));
    if (len) std::memcpy(dst, file.data() + p, len);
    p += len;
  };
  uint32_t n;
  take(&n, 4);
  std::vector<uint64_t> hoffs(n + 1);
  take(hoffs.data(), 8 * (n + 1));
  const size_t wire_bytes = hoffs[n];
  uint8_t* wire = static_cast<uint8_t*>(std::malloc(wire_bytes ? wire_bytes : 1));
  take(wire, wire_bytes);
  std::vector<int32_t> want_status(n);
  take(want_status.data(), 4 * n);
  uint64_t want_bytes;
  take(&want_bytes, 8);
  std::vector<uint8_t> want(want_bytes);
  take(want.data(), want_bytes);

  // the whole batch, into an arena of exactly the size it needs
  std::vector<uint64_t> offs(n);
  std::vector<int32_t> status(n);
  size_t used = 0;
  uint8_t* arena = static_cast<uint8_t*>(std::malloc(want_bytes ? want_bytes : 1));
  int rc = l7m_http_wire_decode(wire, wire_bytes, hoffs.data(), n, nullptr, arena, want_bytes, offs.data(),
                                status.data(), &used);
  if (rc != L7M_OK || used != want_bytes) return fail("batch decode", 0);
  if (std::memcmp(arena, want.data(), want_bytes) != 0) return fail("arena bytes", 0);
  for (size_t i = 0; i < n; ++i)
    if (status[i] != want_status[i]) return fail("status", i);
  if (want_bytes > l7m_http_wire_arena_bound(wire_bytes, n)) return fail("bound", 0);

  // one byte short: L7M_ENOMEM, the size still reported, nothing past the capacity
  if (want_bytes) {
    uint8_t* tight = static_cast<uint8_t*>(std::malloc(want_bytes - 1 ? want_bytes - 1 : 1));
    rc = l7m_http_wire_decode(wire, wire_bytes, hoffs.data(), n, nullptr, tight, want_bytes - 1, offs.data(),
                              status.data(), &used);
    std::free(tight);
    if (rc != L7M_ENOMEM || used != want_bytes) return fail("short capacity", 0);
  }

  // head by head, each in a heap block of its own size
  for (size_t i = 0; i < n; ++i) {
    const size_t len = hoffs[i + 1] - hoffs[i];
    uint8_t* head = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    if (len) std::memcpy(head, wire + hoffs[i], len);
    const uint64_t ho[2] = {0, len};
    const size_t rec_end = i + 1 < n ? offs[i + 1] : want_bytes;
    const size_t rec_len = rec_end - offs[i];
    uint8_t* rec = static_cast<uint8_t*>(std::malloc(rec_len));
    uint64_t o;
    int32_t st;
    rc = l7m_http_wire_decode(head, len, ho, 1, nullptr, rec, rec_len, &o, &st, &used);
    const bool ok = rc == L7M_OK && used == rec_len && st == want_status[i] &&
                    std::memcmp(rec, want.data() + offs[i], rec_len) == 0;
    std::free(rec);
    std::free(head);
    if (!ok) return fail("single decode", i);
  }

  // encode the arena, decode the result: the accepted records come back
  std::vector<uint64_t> eoffs(n + 1);
  std::vector<int32_t> est(n);
  const int64_t need = l7m_http_wire_encode(arena, want_bytes, offs.data(), n, nullptr, 0, eoffs.data(), est.data());
  if (need < 0) return fail("encode size", 0);
  uint8_t* enc = static_cast<uint8_t*>(std::malloc(need ? need : 1));
  if (l7m_http_wire_encode(arena, want_bytes, offs.data(), n, enc, need, eoffs.data(), est.data()) != need)
    return fail("encode", 0);
  const size_t cap2 = l7m_http_wire_arena_bound(need, n);
  uint8_t* arena2 = static_cast<uint8_t*>(std::malloc(cap2 ? cap2 : 1));
  std::vector<uint64_t> offs2(n);
  std::vector<int32_t> status2(n);
  rc = l7m_http_wire_decode(enc, need, eoffs.data(), n, nullptr, arena2, cap2, offs2.data(), status2.data(), &used);
  if (rc != L7M_OK) return fail("decode of encoded", 0);
  size_t accepted = 0;
  for (size_t i = 0; i < n; ++i) {
    if ((est[i] >= 0) != (want_status[i] >= 0)) return fail("encoder verdict", i);
    if (est[i] < 0) continue;
    ++accepted;
    const size_t rec_len = (i + 1 < n ? offs[i + 1] : want_bytes) - offs[i];
    if (status2[i] != est[i] || std::memcmp(arena2 + offs2[i], arena + offs[i], rec_len) != 0)
      return fail("round trip", i);
  }
  std::free(arena2);
  std::free(enc);
  std::free(arena);
  std::free(wire);
  std::printf("OK: %u heads, %zu accepted, %llu arena bytes\n", n, accepted,
              static_cast<unsigned long long>(want_bytes));
  return 0;
}
