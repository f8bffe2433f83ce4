// l7m_http_wire.h — the HTTP/1.x request-head grammar (DESIGN.md "HTTP/1.x
// wire decode"), written once for the host decoder (http_wire.cc) and the
// device decoder (l7m_http_wire.hip): both instantiate these templates, so a
// head decodes to the same bytes on either side.
//
// A head is read through a Src (`uint8_t at(uint64_t i) const`, i < len) and a
// record is written through a Sink (`void put(uint8_t)`, bytes in record
// order, a multiple of four of them per record).  wire_scan validates a head
// and measures its record; wire_emit writes the record of a head wire_scan
// accepted; wire_emit_failed writes the 20-byte record of one it refused.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/l7match.h"

#if defined(__HIP__)
#define L7M_WIRE_FN __host__ __device__ inline
#else
#define L7M_WIRE_FN inline
#endif

namespace l7m {

struct WireInfo {
  int32_t status;      // bytes consumed (>= 0) or L7M_WIRE_E*
  uint32_t n_hdr;      // regular headers (host excluded)
  uint32_t mlen, plen; // method at 0, target at mlen + 1
  uint32_t apos, alen; // value of the host header (have_host)
  uint32_t have_host;
  uint32_t hdr_pos;    // first header line
  uint32_t rec_len;    // unpadded record bytes
};

L7M_WIRE_FN uint32_t wire_padded(uint32_t rec_len) { return (rec_len + 3u) & ~3u; }

// RFC 7230 §3.2.6 tchar
L7M_WIRE_FN bool wire_tchar(uint32_t c) {
  if (c - '0' < 10u || (c | 0x20u) - 'a' < 26u) return true;
  switch (c) {
    case '!': case '#': case '$': case '%': case '&': case '\'': case '*': case '+':
    case '-': case '.': case '^': case '_': case '`': case '|': case '~':
      return true;
    default:
      return false;
  }
}

L7M_WIRE_FN bool wire_ows(uint32_t c) { return c == ' ' || c == '\t'; }

template <class Src>
L7M_WIRE_FN bool wire_is_host(const Src& s, uint64_t p, uint64_t nlen) {
  return nlen == 4 && (s.at(p) | 0x20u) == 'h' && (s.at(p + 1) | 0x20u) == 'o' && (s.at(p + 2) | 0x20u) == 's' &&
         (s.at(p + 3) | 0x20u) == 't';
}

// One pass from left to right; the first offending byte decides the code and
// running out of bytes is L7M_WIRE_EINCOMPLETE.  A length limit is checked
// when its field ends, the header count when the 256th regular header's line
// ends.
template <class Src>
L7M_WIRE_FN void wire_scan(const Src& s, uint64_t len, WireInfo& o) {
  o.status = L7M_WIRE_EINCOMPLETE;
  o.n_hdr = o.mlen = o.plen = o.apos = o.alen = o.have_host = o.hdr_pos = o.rec_len = 0;
  uint64_t p = 0;
  while (p < len && wire_tchar(s.at(p))) ++p;
  if (p >= len) return;
  if (p == 0 || s.at(p) != ' ') { o.status = L7M_WIRE_EBADLINE; return; }
  if (p > 0xffffu) { o.status = L7M_WIRE_ETOOLONG; return; }
  o.mlen = static_cast<uint32_t>(p);
  const uint64_t t0 = ++p;
  while (p < len && s.at(p) > 0x20u && s.at(p) != 0x7fu) ++p;
  if (p >= len) return;
  if (p == t0 || s.at(p) != ' ') { o.status = L7M_WIRE_EBADLINE; return; }
  if (p - t0 > 0xffffu) { o.status = L7M_WIRE_ETOOLONG; return; }
  o.plen = static_cast<uint32_t>(p - t0);
  ++p;
  for (uint32_t k = 0; k < 10; ++k, ++p) {
    if (p >= len) return;
    const uint32_t c = s.at(p);
    const bool ok = k == 7 ? (c == '0' || c == '1') : c == static_cast<uint8_t>("HTTP/1.1\r\n"[k]);
    if (!ok) { o.status = L7M_WIRE_EBADLINE; return; }
  }
  if (p > 0x7fffffffu) { o.status = L7M_WIRE_ETOOLONG; return; }
  o.hdr_pos = static_cast<uint32_t>(p);
  uint64_t fields = static_cast<uint64_t>(o.mlen) + o.plen;
  for (;;) {
    if (p >= len) return;
    uint32_t c = s.at(p);
    if (c == '\r') {
      if (p + 1 >= len) return;
      if (s.at(p + 1) != '\n') { o.status = L7M_WIRE_EBADHEADER; return; }
      p += 2;
      break;
    }
    const uint64_t n0 = p;
    while (p < len && wire_tchar(s.at(p))) ++p;
    if (p >= len) return;
    if (p == n0 || s.at(p) != ':') { o.status = L7M_WIRE_EBADHEADER; return; }  // LF, obs-fold, SP before ':'
    const uint64_t nlen = p - n0;
    if (nlen > 0xffffu) { o.status = L7M_WIRE_ETOOLONG; return; }
    ++p;
    while (p < len && wire_ows(s.at(p))) ++p;
    const uint64_t v0 = p;
    uint64_t vend = p;
    for (;;) {
      if (p >= len) return;
      c = s.at(p);
      if (c == '\r') {
        if (p + 1 >= len) return;
        if (s.at(p + 1) != '\n') { o.status = L7M_WIRE_EBADHEADER; return; }
        break;
      }
      if (c == '\n' || c == 0) { o.status = L7M_WIRE_EBADHEADER; return; }
      ++p;
      if (!wire_ows(c)) vend = p;
    }
    p += 2;
    const uint64_t vlen = vend - v0;
    if (vlen > 0xffffu) { o.status = L7M_WIRE_ETOOLONG; return; }
    if (wire_is_host(s, n0, nlen)) {
      if (o.have_host) { o.status = L7M_WIRE_EDUPHOST; return; }
      o.have_host = 1;
      if (v0 > 0x7fffffffu) { o.status = L7M_WIRE_ETOOLONG; return; }
      o.apos = static_cast<uint32_t>(v0);
      o.alen = static_cast<uint32_t>(vlen);
      fields += vlen;
    } else {
      if (o.n_hdr == 255) { o.status = L7M_WIRE_ETOOMANY; return; }
      ++o.n_hdr;
      fields += nlen + vlen;
    }
  }
  if (p > 0x7fffffffu) { o.status = L7M_WIRE_ETOOLONG; return; }
  o.rec_len = static_cast<uint32_t>(L7M_HTTP_REC_FIXED + 4u * o.n_hdr + fields);  // < 2^26
  o.status = static_cast<int32_t>(p);
}

template <class Sink>
L7M_WIRE_FN void wire_put_word(Sink& k, uint32_t w) {
  k.put(static_cast<uint8_t>(w));
  k.put(static_cast<uint8_t>(w >> 8));
  k.put(static_cast<uint8_t>(w >> 16));
  k.put(static_cast<uint8_t>(w >> 24));
}

L7M_WIRE_FN uint32_t wire_meta_flags(const l7m_http_wire_meta* m) {
  return (!m || m->ingress) ? static_cast<uint32_t>(L7M_HTTP_F_INGRESS) : 0u;
}

template <class Sink>
L7M_WIRE_FN void wire_emit_failed(const l7m_http_wire_meta* m, Sink& k) {
  wire_put_word(k, 0);
  wire_put_word(k, m ? m->remote_id : 0u);
  wire_put_word(k, (m ? m->dport : 0u) | wire_meta_flags(m) << 16);
  wire_put_word(k, 0);
  wire_put_word(k, (m ? static_cast<uint32_t>(m->policy) : 0u) << 16);
}

// Header lines of a head wire_scan accepted, one call of f(name_pos, name_len,
// value_pos, value_len) per line, the host line included.
template <class Src, class F>
L7M_WIRE_FN void wire_lines(const Src& s, const WireInfo& o, F&& f) {
  uint64_t p = o.hdr_pos;
  while (s.at(p) != '\r') {
    const uint64_t n0 = p;
    while (s.at(p) != ':') ++p;
    const uint64_t nlen = p - n0;
    ++p;
    while (wire_ows(s.at(p))) ++p;
    const uint64_t v0 = p;
    uint64_t vend = p;
    for (uint32_t c; (c = s.at(p)) != '\r';) {
      ++p;
      if (!wire_ows(c)) vend = p;
    }
    p += 2;
    f(n0, nlen, v0, vend - v0);
  }
}

template <class Src, class Sink>
L7M_WIRE_FN void wire_emit(const Src& s, const WireInfo& o, const l7m_http_wire_meta* m, Sink& k) {
  const uint32_t flags = L7M_HTTP_F_METHOD | L7M_HTTP_F_PATH | (o.have_host ? L7M_HTTP_F_AUTHORITY : 0) |
                         wire_meta_flags(m);
  wire_put_word(k, o.rec_len);
  wire_put_word(k, m ? m->remote_id : 0u);
  wire_put_word(k, (m ? m->dport : 0u) | flags << 16 | o.n_hdr << 24);
  wire_put_word(k, o.mlen | o.plen << 16);
  wire_put_word(k, o.alen | (m ? static_cast<uint32_t>(m->policy) : 0u) << 16);
  wire_lines(s, o, [&](uint64_t n0, uint64_t nlen, uint64_t, uint64_t vlen) {
    if (!wire_is_host(s, n0, nlen)) wire_put_word(k, static_cast<uint32_t>(nlen | vlen << 16));
  });
  for (uint32_t i = 0; i < o.mlen; ++i) k.put(s.at(i));
  for (uint32_t i = 0; i < o.plen; ++i) k.put(s.at(o.mlen + 1u + i));
  for (uint32_t i = 0; i < o.alen; ++i) k.put(s.at(o.apos + i));
  wire_lines(s, o, [&](uint64_t n0, uint64_t nlen, uint64_t v0, uint64_t vlen) {
    if (wire_is_host(s, n0, nlen)) return;
    for (uint64_t i = 0; i < nlen; ++i) {
      const uint32_t c = s.at(n0 + i);
      k.put(static_cast<uint8_t>(c - 'A' < 26u ? c + 32u : c));
    }
    for (uint64_t i = 0; i < vlen; ++i) k.put(s.at(v0 + i));
  });
  for (uint32_t i = o.rec_len; i & 3u; ++i) k.put(0);
}

}  // namespace l7m
