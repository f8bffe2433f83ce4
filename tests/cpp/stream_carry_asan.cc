// Stand-alone check of the resumable HTTP framer and the stream carry for
// sanitizer builds (no Python, no device):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include tests/cpp/stream_carry_asan.cc cilium_amd/csrc/stream_frame.cc cilium_amd/csrc/http_wire.cc \
//       -o stream_carry_asan
//   python -c "import sys; sys.path[:0] = ['.', 'tests']; import stream_resume_cases as R; \
//              R.dump('stream_carry.bin', *R.dump_cases())"
//   ./stream_carry_asan stream_carry.bin
// Reads the file stream_resume_cases.dump writes (both rounds of the two-piece
// split set and the three fuzz rounds of both protocols, with the outputs the
// Python framer and carry expect), holds every input and output in a heap
// block of its exact size so that a read or write one byte out of place is
// caught, and makes each call as the sizing call, with the exact capacity and
// one head / one byte short; the framer also with its state arrays aliased,
// and its slices go through l7m_http_wire_decode.  Exit status 0 and "OK" when
// everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "l7match.h"

static int fail(const char* what, size_t set) {
  std::fprintf(stderr, "FAIL: %s (case %zu)\n", what, set);
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

static FILE* g_file;

static void take(void* dst, size_t len) {
  if (len && std::fread(dst, 1, len, g_file) != len) std::exit(fail("short file", 0));
}

template <class T>
static T* take_exact(size_t count) {
  T* p = exact<T>(count);
  take(p, count * sizeof(T));
  return p;
}

template <class T>
static std::vector<T> take_vector(size_t count) {
  std::vector<T> v(count);
  take(v.data(), count * sizeof(T));
  return v;
}

static size_t g_heads, g_bytes;

static int frame_case(size_t id) {
  uint32_t nc;
  take(&nc, 4);
  uint64_t* coffs = take_exact<uint64_t>(nc + 1);
  const size_t wire_bytes = coffs[nc];
  uint8_t* wire = take_exact<uint8_t>(wire_bytes);
  const std::vector<l7m_stream_state> state_in = take_vector<l7m_stream_state>(nc);
  const std::vector<int32_t> want_status = take_vector<int32_t>(nc);
  const std::vector<uint64_t> want_consumed = take_vector<uint64_t>(nc);
  const std::vector<l7m_stream_state> want_state = take_vector<l7m_stream_state>(nc);
  uint64_t n;
  take(&n, 8);
  const std::vector<uint64_t> want_offs = take_vector<uint64_t>(n + 1);
  const std::vector<uint32_t> want_conn = take_vector<uint32_t>(n);
  if (n > l7m_http_stream_heads_bound(wire_bytes, nc)) return fail("heads bound", id);
  int32_t* status = exact<int32_t>(nc);
  uint64_t* consumed = exact<uint64_t>(nc);
  struct Call {
    size_t cap;
    bool arrays, alias;
  };
  const Call calls[] = {{0, false, false},
                        {static_cast<size_t>(n), true, false},
                        {static_cast<size_t>(n ? n - 1 : 0), true, false},
                        {static_cast<size_t>(n), true, true}};
  for (const Call& call : calls) {
    const size_t cap = call.cap;
    uint64_t* offs = exact<uint64_t>(cap + 1);
    uint32_t* hconn = exact<uint32_t>(cap);
    l7m_http_wire_meta* hmeta = exact<l7m_http_wire_meta>(cap);
    l7m_stream_state* sin = exact<l7m_stream_state>(nc);
    if (nc) std::memcpy(sin, state_in.data(), nc * sizeof(l7m_stream_state));
    l7m_stream_state* sout = call.alias ? sin : exact<l7m_stream_state>(nc);
    std::memset(status, 0xA5, 4ull * nc);
    std::memset(consumed, 0xA5, 8ull * nc);
    size_t got = 99;
    const int rc = l7m_http_stream_frame_resume(wire, wire_bytes, coffs, nc, nullptr, call.arrays ? offs : nullptr,
                                                call.arrays ? hconn : nullptr, call.arrays ? hmeta : nullptr, cap,
                                                status, consumed, &got, sin, sout);
    if (got != n || !same(status, want_status) || !same(consumed, want_consumed) || !same(sout, want_state))
      return fail("frame: per-connection outputs", id);
    if (!call.alias && !same(sin, state_in)) return fail("frame: state in was written", id);
    if (cap == n && call.arrays) {
      if (rc != L7M_OK || !same(offs, want_offs) || !same(hconn, want_conn)) return fail("frame: exact capacity", id);
      if (!call.alias) {  // the slices, trailing foreign bytes included, are what the decoder takes
        const size_t acap = l7m_http_wire_arena_bound(wire_bytes, n);
        uint8_t* arena = exact<uint8_t>(acap);
        uint64_t* roffs = exact<uint64_t>(n);
        int32_t* wstatus = exact<int32_t>(n);
        size_t used = 0;
        if (l7m_http_wire_decode(wire, wire_bytes, offs, n, hmeta, arena, acap, roffs, wstatus, &used) != L7M_OK)
          return fail("frame: decode of the slices", id);
        for (size_t i = 0; i < n; ++i)
          if (wstatus[i] == L7M_WIRE_EINCOMPLETE) return fail("frame: an incomplete head was emitted", id);
        std::free(arena);
        std::free(roffs);
        std::free(wstatus);
      }
    } else {
      if (rc != (n > cap ? L7M_ENOMEM : L7M_OK)) return fail("frame: return code", id);
      if (n > cap && (!untouched(offs, cap + 1) || !untouched(hconn, cap) || !untouched(hmeta, cap)))
        return fail("frame: one head short", id);
    }
    std::free(offs);
    std::free(hconn);
    std::free(hmeta);
    if (sout != sin) std::free(sout);
    std::free(sin);
  }
  std::free(coffs);
  std::free(wire);
  std::free(status);
  std::free(consumed);
  g_heads += n;
  return 0;
}

static int carry_case(size_t id) {
  uint32_t hdr[3];
  take(hdr, 12);
  const uint32_t n_prev = hdr[0], nc = hdr[1], has_state = hdr[2];
  uint64_t* coffs = take_exact<uint64_t>(n_prev + 1);
  const size_t wire_bytes = coffs[n_prev];
  uint8_t* wire = take_exact<uint8_t>(wire_bytes);
  int32_t* status = take_exact<int32_t>(n_prev);
  uint64_t* consumed = take_exact<uint64_t>(n_prev);
  uint64_t* soffs = take_exact<uint64_t>(nc + 1);
  const size_t seg_bytes = soffs[nc];
  uint8_t* seg = take_exact<uint8_t>(seg_bytes);
  const std::vector<l7m_stream_state> state_in = take_vector<l7m_stream_state>(has_state ? nc : 0);
  uint64_t total;
  take(&total, 8);
  const std::vector<uint64_t> want_offs = take_vector<uint64_t>(nc + 1);
  const std::vector<uint8_t> want_wire = take_vector<uint8_t>(total);
  const std::vector<l7m_stream_state> want_state = take_vector<l7m_stream_state>(has_state ? nc : 0);
  if (total > l7m_stream_carry_bound(wire_bytes, seg_bytes)) return fail("carry bound", id);
  struct Call {
    size_t cap;
    bool outputs;
  };
  const Call calls[] = {{0, false}, {static_cast<size_t>(total), true}, {static_cast<size_t>(total ? total - 1 : 0), true}};
  for (const Call& call : calls) {
    uint8_t* next = exact<uint8_t>(call.cap);
    uint64_t* noffs = exact<uint64_t>(nc + 1);
    l7m_stream_state* state = has_state ? exact<l7m_stream_state>(nc) : nullptr;
    if (has_state && nc) std::memcpy(state, state_in.data(), nc * sizeof(l7m_stream_state));
    uint64_t got = 99;
    const int rc = l7m_stream_carry(wire, wire_bytes, coffs, n_prev, status, consumed, seg, seg_bytes, soffs, nc, state,
                                    call.outputs ? next : nullptr, call.cap, call.outputs ? noffs : nullptr, &got);
    if (got != total) return fail("carry: total", id);
    if (call.outputs && call.cap == total) {
      if (rc != L7M_OK || !same(noffs, want_offs) || !same(next, want_wire) || (has_state && !same(state, want_state)))
        return fail("carry: exact capacity", id);
    } else {
      if (rc != (total > call.cap ? L7M_ENOMEM : L7M_OK)) return fail("carry: return code", id);
      if (!untouched(next, call.cap) || !untouched(noffs, nc + 1) || (has_state && !same(state, state_in)))
        return fail("carry: sizing call or one byte short", id);
    }
    std::free(next);
    std::free(noffs);
    std::free(state);
  }
  std::free(coffs);
  std::free(wire);
  std::free(status);
  std::free(consumed);
  std::free(soffs);
  std::free(seg);
  g_bytes += total;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return std::fprintf(stderr, "usage: %s stream_carry.bin\n", argv[0]), 2;
  g_file = std::fopen(argv[1], "rb");
  if (!g_file) return std::perror(argv[1]), 2;
  size_t frames = 0, carries = 0;
  uint32_t kind;
  while (std::fread(&kind, 4, 1, g_file) == 1) {
    if (kind == 1) {
      if (frame_case(frames + carries)) return 1;
      ++frames;
    } else if (kind == 2) {
      if (carry_case(frames + carries)) return 1;
      ++carries;
    } else {
      return fail("unknown case kind", frames + carries);
    }
  }
  std::fclose(g_file);
  std::printf("OK: %zu frame calls and %zu carries, %zu heads, %zu carried bytes\n", frames, carries, g_heads, g_bytes);
  return 0;
}
