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

// ---- streaming across calls (DESIGN.md "Streaming across calls") ----------

L7M_WIRE_FN int32_t stream_close(l7m_stream_state& st, int32_t status) {
  st.left = 0;
  st.mode = L7M_STREAM_MODE_CLOSED;
  st.status = status;
  return status;
}

L7M_WIRE_FN int32_t stream_pause(l7m_stream_state& st, int32_t mode, uint64_t left, int32_t status) {
  st.left = left;
  st.mode = mode;
  st.status = 0;
  return status;
}

// http_stream_walk made resumable: the connection s[0, len) is entered in
// state `st` (what an earlier walk over the bytes in front of it left) and
// `st` receives the state it is left in.  f(start) per head wire_scan accepts
// or refuses, never for an incomplete one; *consumed is how far the walk has
// committed: a complete head is consumed when it is emitted and a body as it
// is skipped, so that wire[consumed, len) and the state are all a later walk
// needs.  The byte rules are http_stream_walk's and stream_chunked's, examined
// in the same order; a chunk-size line or a trailer line that the bytes end
// in is read again from its first byte.
template <class Src, class F>
L7M_WIRE_FN int32_t http_stream_walk_resume(const Src& s, uint64_t len, l7m_stream_state& st, uint64_t* consumed,
                                            F&& f) {
  int32_t mode = st.mode;
  uint64_t left = st.left;
  if (static_cast<uint32_t>(mode) >= static_cast<uint32_t>(L7M_STREAM_MODE_CLOSED)) {  // CLOSED, or no mode at all
    *consumed = len;
    return st.status;
  }
  uint64_t p = 0;
  *consumed = 0;
  for (;;) {
    if (mode == L7M_STREAM_MODE_HEAD) {
      if (p >= len) return stream_pause(st, L7M_STREAM_MODE_HEAD, 0, L7M_STREAM_OK);
      const StreamAt<Src> h{s, p};
      WireInfo info;
      wire_scan(h, len - p, info);
      if (info.status == L7M_WIRE_EINCOMPLETE) return stream_pause(st, L7M_STREAM_MODE_HEAD, 0, L7M_STREAM_EPARTIAL_HEAD);
      f(p);
      if (info.status < 0) return stream_close(st, L7M_STREAM_EBADHEAD);
      const uint64_t body = p + static_cast<uint64_t>(info.status);
      if (info.mlen == 7 && h.at(0) == 'C' && h.at(1) == 'O' && h.at(2) == 'N' && h.at(3) == 'N' && h.at(4) == 'E' &&
          h.at(5) == 'C' && h.at(6) == 'T') {
        *consumed = body;  // the head; what follows is the tunnel's
        return stream_close(st, L7M_STREAM_TUNNEL);
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
      if (n_te && n_cl) return stream_close(st, L7M_STREAM_EAMBIGUOUS);
      if (n_te) {
        if (n_te != 1 || !stream_ieq(h, te_pos, te_len, "chunked", 7)) return stream_close(st, L7M_STREAM_EBADTE);
        mode = L7M_STREAM_MODE_CHUNK_LINE;
      } else if (n_cl) {
        if (n_cl != 1 || cl_len < 1 || cl_len > 18) return stream_close(st, L7M_STREAM_EBADLENGTH);
        uint64_t v = 0;
        for (uint64_t i = 0; i < cl_len; ++i) {
          const uint32_t c = h.at(cl_pos + i);
          if (c - '0' >= 10u) return stream_close(st, L7M_STREAM_EBADLENGTH);
          v = v * 10u + (c - '0');  // < 10^18
        }
        left = v;
        if (v) mode = L7M_STREAM_MODE_BODY;
      }
      p = body;
      *consumed = p;
    } else if (mode == L7M_STREAM_MODE_BODY || mode == L7M_STREAM_MODE_CHUNK_DATA) {
      const uint64_t k = left < len - p ? left : len - p;
      p += k;
      left -= k;
      *consumed = p;
      if (left) return stream_pause(st, mode, left, L7M_STREAM_EPARTIAL_BODY);
      if (mode == L7M_STREAM_MODE_BODY) {
        mode = L7M_STREAM_MODE_HEAD;
        continue;
      }
      // the CRLF behind the chunk's data
      if (p >= len) return stream_pause(st, mode, 0, L7M_STREAM_EPARTIAL_BODY);
      if (s.at(p) != '\r') return stream_close(st, L7M_STREAM_EBADCHUNK);
      if (p + 1 >= len) return stream_pause(st, mode, 0, L7M_STREAM_EPARTIAL_BODY);
      if (s.at(p + 1) != '\n') return stream_close(st, L7M_STREAM_EBADCHUNK);
      p += 2;
      *consumed = p;
      mode = L7M_STREAM_MODE_CHUNK_LINE;
    } else if (mode == L7M_STREAM_MODE_CHUNK_LINE) {
      uint64_t q = p, size = 0;
      uint32_t nd = 0;
      for (;; ++q) {
        if (q >= len) return stream_pause(st, mode, 0, L7M_STREAM_EPARTIAL_BODY);
        const int32_t x = stream_hex(s.at(q));
        if (x < 0) break;
        if (nd == 15) return stream_close(st, L7M_STREAM_EBADCHUNK);  // a 16th digit
        size = size << 4 | static_cast<uint64_t>(x);
        ++nd;
      }
      if (nd == 0) return stream_close(st, L7M_STREAM_EBADCHUNK);
      uint32_t c = s.at(q);
      if (c == ';') {
        for (++q;; ++q) {
          if (q >= len) return stream_pause(st, mode, 0, L7M_STREAM_EPARTIAL_BODY);
          c = s.at(q);
          if (c == '\r') break;
          if (c == '\n' || c == 0) return stream_close(st, L7M_STREAM_EBADCHUNK);
        }
      }
      if (c != '\r') return stream_close(st, L7M_STREAM_EBADCHUNK);
      if (++q >= len) return stream_pause(st, mode, 0, L7M_STREAM_EPARTIAL_BODY);
      if (s.at(q) != '\n') return stream_close(st, L7M_STREAM_EBADCHUNK);
      p = q + 1;
      *consumed = p;
      left = size;
      mode = size ? L7M_STREAM_MODE_CHUNK_DATA : L7M_STREAM_MODE_TRAILER;
    } else {  // TRAILER: one line (the head's header-line byte rules, no length limits) or the empty line
      uint64_t q = p;
      if (q >= len) return stream_pause(st, mode, 0, L7M_STREAM_EPARTIAL_BODY);
      uint32_t c = s.at(q);
      if (c == '\r') {
        if (++q >= len) return stream_pause(st, mode, 0, L7M_STREAM_EPARTIAL_BODY);
        if (s.at(q) != '\n') return stream_close(st, L7M_STREAM_EBADCHUNK);
        mode = L7M_STREAM_MODE_HEAD;
      } else {
        while (q < len && wire_tchar(s.at(q))) ++q;
        if (q >= len) return stream_pause(st, mode, 0, L7M_STREAM_EPARTIAL_BODY);
        if (q == p || s.at(q) != ':') return stream_close(st, L7M_STREAM_EBADCHUNK);
        for (++q;; ++q) {
          if (q >= len) return stream_pause(st, mode, 0, L7M_STREAM_EPARTIAL_BODY);
          c = s.at(q);
          if (c == '\r') break;
          if (c == '\n' || c == 0) return stream_close(st, L7M_STREAM_EBADCHUNK);
        }
        if (++q >= len) return stream_pause(st, mode, 0, L7M_STREAM_EPARTIAL_BODY);
        if (s.at(q) != '\n') return stream_close(st, L7M_STREAM_EBADCHUNK);
      }
      p = q + 1;
      *consumed = p;
    }
  }
}

// What l7m_stream_carry takes from connection c: the tail wire[tsrc, tsrc +
// tlen), then seg[nsrc, nsrc + nlen), after `skip` body bytes of the segment
// were dropped.  [lo, hi) is the connection in the wire (empty for one opened
// this round), [slo, shi) its segment, (mode, left) its state: zeros for Kafka,
// which carries like a connection at a request boundary.
struct CarryPlan {
  uint64_t tsrc, tlen, nsrc, nlen, skip;
};

L7M_WIRE_FN CarryPlan stream_carry_plan(uint64_t lo, uint64_t hi, uint64_t consumed, int32_t status, uint64_t slo,
                                        uint64_t shi, int32_t mode, uint64_t left) {
  CarryPlan pl{0, 0, 0, 0, 0};
  const bool open = status == L7M_STREAM_OK || status == L7M_STREAM_EPARTIAL_HEAD ||
                    status == L7M_STREAM_EPARTIAL_BODY || status == L7M_STREAM_EPARTIAL_FRAME;
  if (!open || static_cast<uint32_t>(mode) >= static_cast<uint32_t>(L7M_STREAM_MODE_CLOSED)) return pl;
  pl.nsrc = slo;
  pl.nlen = shi - slo;
  if ((mode == L7M_STREAM_MODE_BODY || mode == L7M_STREAM_MODE_CHUNK_DATA) && left) {
    pl.skip = left < pl.nlen ? left : pl.nlen;  // the tail is empty by the framer's contract
    pl.nsrc += pl.skip;
    pl.nlen -= pl.skip;
    return pl;
  }
  pl.tsrc = lo + consumed;
  pl.tlen = hi - lo - consumed;
  return pl;
}

L7M_WIRE_FN void stream_carry_state(l7m_stream_state& st, uint64_t skip) {
  if (!skip) return;
  st.left -= skip;
  if (st.mode == L7M_STREAM_MODE_BODY && !st.left) st.mode = L7M_STREAM_MODE_HEAD;
}

}  // namespace l7m
