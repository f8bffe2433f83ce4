// l7m_stream_frame.h — the framing rules of connection byte streams (DESIGN.md
// "Stream framing"), written once for the host functions (stream_frame.cc) and
// the device kernels (l7m_stream_frame.hip): both instantiate these templates,
// so a connection frames to the same slices and the same status on either side.
//
// A connection is read through a Src (`uint8_t at(uint64_t i) const`, i < len).
// http_stream_walk finds the request heads of an HTTP/1.1 connection: the head
// grammar is wire_scan's (l7m_http_wire.h), the body framing RFC 7230 §3.3 and
// §4.1.  kafka_stream_walk finds the size-prefixed requests of a Kafka
// connection (proto.ReadReq).  Both call f once per slice, in order, and return
// the connection's L7M_STREAM_* status; *consumed receives the bytes up to the
// end of the last complete request.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "l7m_http_wire.h"

namespace l7m {

// A source that starts `off` bytes into another one.
template <class Src>
struct StreamAt {
  const Src& s;
  uint64_t off;
  L7M_WIRE_FN uint8_t at(uint64_t i) const { return s.at(off + i); }
};

// ASCII case-insensitive comparison of s[p, p + n) with a lower-case word.
template <class Src>
L7M_WIRE_FN bool stream_ieq(const Src& s, uint64_t p, uint64_t n, const char* word, uint32_t wlen) {
  if (n != wlen) return false;
  for (uint32_t i = 0; i < wlen; ++i) {
    uint32_t c = s.at(p + i);
    if (c - 'A' < 26u) c += 32u;
    if (c != static_cast<uint8_t>(word[i])) return false;
  }
  return true;
}

L7M_WIRE_FN int32_t stream_hex(uint32_t c) {
  if (c - '0' < 10u) return static_cast<int32_t>(c - '0');
  if ((c | 0x20u) - 'a' < 6u) return static_cast<int32_t>((c | 0x20u) - 'a' + 10u);
  return -1;
}

// A chunked body at s[q, len): L7M_STREAM_OK with *end behind the last
// trailer's empty line, L7M_STREAM_EBADCHUNK at the first offending byte,
// L7M_STREAM_EPARTIAL_BODY when the bytes run out first.  Chunk data is
// skipped by its size.
template <class Src>
L7M_WIRE_FN int32_t stream_chunked(const Src& s, uint64_t q, uint64_t len, uint64_t* end) {
  for (;;) {
    uint64_t size = 0;
    uint32_t nd = 0;
    for (;; ++q) {
      if (q >= len) return L7M_STREAM_EPARTIAL_BODY;
      const int32_t h = stream_hex(s.at(q));
      if (h < 0) break;
      if (nd == 15) return L7M_STREAM_EBADCHUNK;  // a 16th digit
      size = size << 4 | static_cast<uint64_t>(h);
      ++nd;
    }
    if (nd == 0) return L7M_STREAM_EBADCHUNK;
    uint32_t c = s.at(q);
    if (c == ';') {
      for (++q;; ++q) {
        if (q >= len) return L7M_STREAM_EPARTIAL_BODY;
        c = s.at(q);
        if (c == '\r') break;
        if (c == '\n' || c == 0) return L7M_STREAM_EBADCHUNK;
      }
    }
    if (c != '\r') return L7M_STREAM_EBADCHUNK;
    if (++q >= len) return L7M_STREAM_EPARTIAL_BODY;
    if (s.at(q) != '\n') return L7M_STREAM_EBADCHUNK;
    ++q;
    if (size == 0) break;
    if (size > len - q) return L7M_STREAM_EPARTIAL_BODY;
    q += size;
    if (q >= len) return L7M_STREAM_EPARTIAL_BODY;
    if (s.at(q) != '\r') return L7M_STREAM_EBADCHUNK;
    if (++q >= len) return L7M_STREAM_EPARTIAL_BODY;
    if (s.at(q) != '\n') return L7M_STREAM_EBADCHUNK;
    ++q;
  }
  // trailer lines (the head's header-line byte rules, no length limits), then the empty line
  for (;;) {
    if (q >= len) return L7M_STREAM_EPARTIAL_BODY;
    uint32_t c = s.at(q);
    if (c == '\r') {
      if (++q >= len) return L7M_STREAM_EPARTIAL_BODY;
      if (s.at(q) != '\n') return L7M_STREAM_EBADCHUNK;
      *end = q + 1;
      return L7M_STREAM_OK;
    }
    const uint64_t n0 = q;
    while (q < len && wire_tchar(s.at(q))) ++q;
    if (q >= len) return L7M_STREAM_EPARTIAL_BODY;
    if (q == n0 || s.at(q) != ':') return L7M_STREAM_EBADCHUNK;
    for (++q;; ++q) {
      if (q >= len) return L7M_STREAM_EPARTIAL_BODY;
      c = s.at(q);
      if (c == '\r') break;
      if (c == '\n' || c == 0) return L7M_STREAM_EBADCHUNK;
    }
    if (++q >= len) return L7M_STREAM_EPARTIAL_BODY;
    if (s.at(q) != '\n') return L7M_STREAM_EBADCHUNK;
    ++q;
  }
}

// The request heads of one HTTP/1.1 connection s[0, len): f(start) per slice
// (a slice runs to the next one's start, the last to len).  Returns the
// connection's status.
template <class Src, class F>
L7M_WIRE_FN int32_t http_stream_walk(const Src& s, uint64_t len, uint64_t* consumed, F&& f) {
  uint64_t p = 0;
  *consumed = 0;
  while (p < len) {
    f(p);
    const StreamAt<Src> h{s, p};
    WireInfo info;
    wire_scan(h, len - p, info);
    if (info.status < -1) return L7M_STREAM_EBADHEAD;
    if (info.status < 0) return L7M_STREAM_EPARTIAL_HEAD;
    const uint64_t body = p + static_cast<uint64_t>(info.status);
    if (info.mlen == 7 && h.at(0) == 'C' && h.at(1) == 'O' && h.at(2) == 'N' && h.at(3) == 'N' && h.at(4) == 'E' &&
        h.at(5) == 'C' && h.at(6) == 'T') {
      *consumed = body;  // the head; what follows is the tunnel's
      return L7M_STREAM_TUNNEL;
    }
    uint32_t n_te = 0, n_cl = 0;
    uint64_t te_pos = 0, te_len = 0, cl_pos = 0, cl_len = 0;
    wire_lines(h, info, [&](uint64_t n0, uint64_t nlen, uint64_t v0, uint64_t vlen) {
      if (stream_ieq(h, n0, nlen, "transfer-encoding", 17)) {
        ++n_te;
        te_pos = v0;
        te_len = vlen;
      } else if (stream_ieq(h, n0, nlen, "content-length", 14)) {
        ++n_cl;
        cl_pos = v0;
        cl_len = vlen;
      }
    });
    if (n_te && n_cl) return L7M_STREAM_EAMBIGUOUS;
    if (n_te) {
      if (n_te != 1 || !stream_ieq(h, te_pos, te_len, "chunked", 7)) return L7M_STREAM_EBADTE;
      uint64_t end = 0;
      const int32_t st = stream_chunked(s, body, len, &end);
      if (st != L7M_STREAM_OK) return st;
      p = end;
    } else if (n_cl) {
      if (n_cl != 1 || cl_len < 1 || cl_len > 18) return L7M_STREAM_EBADLENGTH;
      uint64_t v = 0;
      for (uint64_t i = 0; i < cl_len; ++i) {
        const uint32_t c = h.at(cl_pos + i);
        if (c - '0' >= 10u) return L7M_STREAM_EBADLENGTH;
        v = v * 10u + (c - '0');  // < 10^18
      }
      if (v > len - body) return L7M_STREAM_EPARTIAL_BODY;
      p = body + v;
    } else {
      p = body;
    }
    *consumed = p;
  }
  return L7M_STREAM_OK;
}

constexpr uint32_t kKafkaMinSize = 8;            // ReadRequest refuses a message under 12 bytes
constexpr uint32_t kKafkaMaxFrame = 100u * 65535u;  // maxParseBufSize: size + 4 may not pass it

// The requests of one Kafka connection s[0, len): f(start, frame_bytes) per
// frame, the size field included.  Returns the connection's status.
template <class Src, class F>
L7M_WIRE_FN int32_t kafka_stream_walk(const Src& s, uint64_t len, uint64_t* consumed, F&& f) {
  uint64_t p = 0;
  *consumed = 0;
  for (;;) {
    if (len - p < 4) return p == len ? L7M_STREAM_OK : L7M_STREAM_EPARTIAL_FRAME;
    const uint32_t u = static_cast<uint32_t>(s.at(p)) << 24 | static_cast<uint32_t>(s.at(p + 1)) << 16 |
                       static_cast<uint32_t>(s.at(p + 2)) << 8 | s.at(p + 3);
    const int32_t size = static_cast<int32_t>(u);
    if (size < static_cast<int32_t>(kKafkaMinSize) || u + 4u > kKafkaMaxFrame) return L7M_STREAM_EBADSIZE;
    if (u + 4u > len - p) return L7M_STREAM_EPARTIAL_FRAME;
    f(p, static_cast<uint64_t>(u) + 4u);
    p += u + 4u;
    *consumed = p;
  }
}

L7M_WIRE_FN uint64_t stream_padded(uint64_t frame_bytes) { return (frame_bytes + 3u) & ~static_cast<uint64_t>(3); }

}  // namespace l7m
