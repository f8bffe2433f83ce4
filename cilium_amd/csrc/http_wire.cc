// http_wire.cc — host side of the HTTP/1.x wire path: the decoder (the CPU
// path, and the definition l7m_http_wire.hip reproduces), the arena bound and
// the encoder that turns an arena back into request heads.  Needs no device.
#include <cstring>

#include "l7m_http_wire.h"

namespace {

using namespace l7m;

struct HostSrc {
  const uint8_t* p;
  uint8_t at(uint64_t i) const { return p[i]; }
};

struct HostSink {
  uint8_t* p;
  void put(uint8_t b) { *p++ = b; }
};

// Appends to wire[0, cap) while counting past it.
struct WireOut {
  uint8_t* wire;
  size_t cap, used;
  void put(const void* s, size_t len) {
    if (wire && used + len <= cap && len) std::memcpy(wire + used, s, len);
    used += len;
  }
};

// Size of record `r`'s head on the wire, or the reason it has none.
int64_t encode_one(const uint8_t* r, size_t avail, WireOut* out) {
  if (avail < L7M_HTTP_REC_FIXED) return L7M_WIRE_EBADHEADER;
  uint32_t w[5];
  std::memcpy(w, r, sizeof w);
  const uint32_t flags = (w[2] >> 16) & 0xffu, nhdr = w[2] >> 24;
  const uint32_t mlen = w[3] & 0xffffu, plen = w[3] >> 16, alen = w[4] & 0xffffu;
  uint64_t need = L7M_HTTP_REC_FIXED + 4ull * nhdr + mlen + plen + alen;
  if (need > w[0] || w[0] > avail) return L7M_WIRE_EBADHEADER;
  for (uint32_t j = 0; j < nhdr; ++j) {
    uint32_t e;
    std::memcpy(&e, r + L7M_HTTP_REC_FIXED + 4 * j, 4);
    need += (e & 0xffffu) + (e >> 16);
  }
  if (need != w[0]) return L7M_WIRE_EBADHEADER;
  if ((flags & (L7M_HTTP_F_METHOD | L7M_HTTP_F_PATH)) != (L7M_HTTP_F_METHOD | L7M_HTTP_F_PATH))
    return L7M_WIRE_EBADHEADER;
  if (!(flags & L7M_HTTP_F_AUTHORITY) && alen) return L7M_WIRE_EBADHEADER;
  const uint8_t* f = r + L7M_HTTP_REC_FIXED + 4 * nhdr;
  if (mlen == 0 || plen == 0) return L7M_WIRE_EBADLINE;
  for (uint32_t i = 0; i < mlen; ++i)
    if (!wire_tchar(f[i])) return L7M_WIRE_EBADLINE;
  for (uint32_t i = 0; i < plen; ++i)
    if (f[mlen + i] <= 0x20 || f[mlen + i] == 0x7f) return L7M_WIRE_EBADLINE;
  auto value_ok = [](const uint8_t* v, uint32_t len) {
    if (len && (wire_ows(v[0]) || wire_ows(v[len - 1]))) return false;
    for (uint32_t i = 0; i < len; ++i)
      if (v[i] == '\r' || v[i] == '\n' || v[i] == 0) return false;
    return true;
  };
  const uint8_t* auth = f + mlen + plen;
  if (!value_ok(auth, alen)) return L7M_WIRE_EBADHEADER;
  const uint8_t* p = auth + alen;
  for (uint32_t j = 0; j < nhdr; ++j) {
    uint32_t e;
    std::memcpy(&e, r + L7M_HTTP_REC_FIXED + 4 * j, 4);
    const uint32_t nl = e & 0xffffu, vl = e >> 16;
    if (nl == 0) return L7M_WIRE_EBADHEADER;
    for (uint32_t i = 0; i < nl; ++i)
      if (!wire_tchar(p[i]) || (p[i] >= 'A' && p[i] <= 'Z')) return L7M_WIRE_EBADHEADER;
    if (nl == 4 && std::memcmp(p, "host", 4) == 0) return L7M_WIRE_EDUPHOST;
    if (!value_ok(p + nl, vl)) return L7M_WIRE_EBADHEADER;
    p += nl + vl;
  }
  const size_t start = out->used;
  out->put(f, mlen);
  out->put(" ", 1);
  out->put(f + mlen, plen);
  out->put(" HTTP/1.1\r\n", 11);
  if (flags & L7M_HTTP_F_AUTHORITY) {
    out->put("host: ", 6);
    out->put(auth, alen);
    out->put("\r\n", 2);
  }
  p = auth + alen;
  for (uint32_t j = 0; j < nhdr; ++j) {
    uint32_t e;
    std::memcpy(&e, r + L7M_HTTP_REC_FIXED + 4 * j, 4);
    const uint32_t nl = e & 0xffffu, vl = e >> 16;
    out->put(p, nl);
    out->put(": ", 2);
    out->put(p + nl, vl);
    out->put("\r\n", 2);
    p += nl + vl;
  }
  out->put("\r\n", 2);
  return static_cast<int64_t>(out->used - start);
}

}  // namespace

namespace l7m {

// One head for the batcher (l7m_batch.cc): measure, then write into the slot.
void http_wire_scan_host(const uint8_t* head, size_t len, WireInfo* info) {
  wire_scan(HostSrc{head}, len, *info);
}
void http_wire_emit_host(const uint8_t* head, const WireInfo& info, const l7m_http_wire_meta* meta, uint8_t* dst) {
  HostSink k{dst};
  wire_emit(HostSrc{head}, info, meta, k);
}

}  // namespace l7m

extern "C" {

size_t l7m_http_wire_arena_bound(size_t wire_bytes, size_t n) {
  if (n == 0) return 0;
  const size_t g = wire_bytes + wire_bytes / 4;
  return 20 * n + (g > 15 ? g - 15 : 0);
}

int l7m_http_wire_decode(const uint8_t* wire, size_t wire_bytes, const uint64_t* head_offs, size_t n,
                         const l7m_http_wire_meta* meta, uint8_t* arena, size_t cap, uint64_t* rec_offsets,
                         int32_t* status, size_t* arena_bytes) {
  if (!arena_bytes || (n && (!head_offs || !rec_offsets || !status)) || (wire_bytes && !wire) || (cap && !arena))
    return L7M_EINVAL;
  *arena_bytes = 0;
  for (size_t i = 0; i < n; ++i)
    if (head_offs[i] > head_offs[i + 1] || head_offs[i + 1] > wire_bytes) return L7M_EINVAL;
  size_t used = 0;
  for (size_t i = 0; i < n; ++i) {
    const HostSrc src{wire + head_offs[i]};
    WireInfo info;
    wire_scan(src, head_offs[i + 1] - head_offs[i], info);
    const size_t sz = info.status < 0 ? L7M_HTTP_REC_FIXED : wire_padded(info.rec_len);
    const l7m_http_wire_meta* m = meta ? meta + i : nullptr;
    if (used + sz <= cap) {
      HostSink k{arena + used};
      if (info.status < 0) wire_emit_failed(m, k);
      else wire_emit(src, info, m, k);
    }
    status[i] = info.status;
    rec_offsets[i] = used;
    used += sz;
  }
  *arena_bytes = used;
  return used > cap ? L7M_ENOMEM : L7M_OK;
}

int64_t l7m_http_wire_encode(const uint8_t* arena, size_t arena_bytes, const uint64_t* rec_offsets, size_t n,
                             uint8_t* wire, size_t cap, uint64_t* head_offs, int32_t* status) {
  if ((n && (!arena || !rec_offsets)) || !head_offs || !status) return L7M_EINVAL;
  WireOut out{wire, cap, 0};
  for (size_t i = 0; i < n; ++i) {
    head_offs[i] = out.used;
    const int64_t s = rec_offsets[i] > arena_bytes
                          ? static_cast<int64_t>(L7M_WIRE_EBADHEADER)
                          : encode_one(arena + rec_offsets[i], arena_bytes - rec_offsets[i], &out);
    status[i] = s > 0x7fffffff ? L7M_WIRE_ETOOLONG : static_cast<int32_t>(s);
  }
  head_offs[n] = out.used;
  if (wire && out.used > cap) return L7M_ENOMEM;
  return static_cast<int64_t>(out.used);
}

}  // extern "C"
