// stream_frame.cc — host side of stream framing (include/l7match.h
// l7m_http_stream_frame, l7m_kafka_stream_frame): connection byte streams ->
// head slices for the wire decoder, or dword-aligned Kafka records.  The rules
// are the templates of l7m_stream_frame.h, which l7m_stream_frame.hip
// instantiates for the device.  Needs no device.
#include <cstring>

#include "l7m_stream_frame.h"

namespace {

using namespace l7m;

struct HostSrc {
  const uint8_t* p;
  uint8_t at(uint64_t i) const { return p[i]; }
};

bool conns_ok(const uint64_t* conn_offs, size_t n_conns, size_t wire_bytes) {
  if (conn_offs[0] > wire_bytes) return false;
  for (size_t c = 0; c < n_conns; ++c)
    if (conn_offs[c] > conn_offs[c + 1] || conn_offs[c + 1] > wire_bytes) return false;
  return true;
}

}  // namespace

extern "C" {

size_t l7m_http_stream_heads_bound(size_t wire_bytes, size_t n_conns) { return wire_bytes / 16 + n_conns; }

int l7m_http_stream_frame(const uint8_t* wire, size_t wire_bytes, const uint64_t* conn_offs, size_t n_conns,
                          const l7m_http_wire_meta* conn_meta, uint64_t* head_offs, uint32_t* head_conn,
                          l7m_http_wire_meta* head_meta, size_t cap_heads, int32_t* conn_status,
                          uint64_t* conn_consumed, size_t* n_heads) {
  if (!n_heads || !conn_offs || (n_conns && (!conn_status || !conn_consumed)) || (wire_bytes && !wire) ||
      (cap_heads && (!head_offs || !head_conn)) || n_conns > 0xffffffffull)
    return L7M_EINVAL;
  *n_heads = 0;
  if (!conns_ok(conn_offs, n_conns, wire_bytes)) return L7M_EINVAL;
  size_t total = 0;
  for (size_t c = 0; c < n_conns; ++c) {
    const HostSrc src{wire + conn_offs[c]};
    conn_status[c] = http_stream_walk(src, conn_offs[c + 1] - conn_offs[c], &conn_consumed[c], [&](uint64_t) { ++total; });
  }
  *n_heads = total;
  if (total > cap_heads) return L7M_ENOMEM;
  if (!head_offs) return L7M_OK;  // no heads and nowhere to put the closing offset
  size_t i = 0;
  for (size_t c = 0; c < n_conns; ++c) {
    const HostSrc src{wire + conn_offs[c]};
    uint64_t used;
    http_stream_walk(src, conn_offs[c + 1] - conn_offs[c], &used, [&](uint64_t start) {
      head_offs[i] = conn_offs[c] + start;
      head_conn[i] = static_cast<uint32_t>(c);
      if (head_meta) {
        if (conn_meta) head_meta[i] = conn_meta[c];
        else head_meta[i] = l7m_http_wire_meta{0, 0, 0, 1, {0, 0, 0}};
      }
      ++i;
    });
  }
  head_offs[total] = conn_offs[n_conns];
  return L7M_OK;
}

size_t l7m_kafka_stream_records_bound(size_t wire_bytes) { return wire_bytes / 12; }
size_t l7m_kafka_stream_arena_bound(size_t wire_bytes) { return wire_bytes + wire_bytes / 4; }

int l7m_kafka_stream_frame(const uint8_t* wire, size_t wire_bytes, const uint64_t* conn_offs, size_t n_conns,
                           const uint32_t* conn_identity, uint8_t* arena, size_t cap_bytes, uint64_t* rec_offsets,
                           uint32_t* rec_conn, uint32_t* src_identities, size_t cap_recs, int32_t* conn_status,
                           uint64_t* conn_consumed, size_t* n_recs, size_t* arena_bytes) {
  if (!n_recs || !arena_bytes || !conn_offs || (n_conns && (!conn_status || !conn_consumed)) ||
      (wire_bytes && !wire) || (cap_recs && (!rec_offsets || !rec_conn)) || (cap_bytes && !arena) ||
      n_conns > 0xffffffffull)
    return L7M_EINVAL;
  *n_recs = 0;
  *arena_bytes = 0;
  if (!conns_ok(conn_offs, n_conns, wire_bytes)) return L7M_EINVAL;
  size_t total = 0, bytes = 0;
  for (size_t c = 0; c < n_conns; ++c) {
    const HostSrc src{wire + conn_offs[c]};
    conn_status[c] = kafka_stream_walk(src, conn_offs[c + 1] - conn_offs[c], &conn_consumed[c],
                                       [&](uint64_t, uint64_t frame) {
                                         ++total;
                                         bytes += stream_padded(frame);
                                       });
  }
  *n_recs = total;
  *arena_bytes = bytes;
  if (total > cap_recs || bytes > cap_bytes) return L7M_ENOMEM;
  size_t i = 0, used = 0;
  for (size_t c = 0; c < n_conns; ++c) {
    const uint8_t* base = wire + conn_offs[c];
    uint64_t consumed;
    kafka_stream_walk(HostSrc{base}, conn_offs[c + 1] - conn_offs[c], &consumed, [&](uint64_t start, uint64_t frame) {
      const uint64_t padded = stream_padded(frame);
      std::memcpy(arena + used, base + start, frame);
      std::memset(arena + used + frame, 0, padded - frame);
      rec_offsets[i] = used;
      rec_conn[i] = static_cast<uint32_t>(c);
      if (src_identities) src_identities[i] = conn_identity ? conn_identity[c] : 0u;
      used += padded;
      ++i;
    });
  }
  return L7M_OK;
}

int l7m_http_stream_frame_resume(const uint8_t* wire, size_t wire_bytes, const uint64_t* conn_offs, size_t n_conns,
                                 const l7m_http_wire_meta* conn_meta, uint64_t* head_offs, uint32_t* head_conn,
                                 l7m_http_wire_meta* head_meta, size_t cap_heads, int32_t* conn_status,
                                 uint64_t* conn_consumed, size_t* n_heads, const l7m_stream_state* conn_state_in,
                                 l7m_stream_state* conn_state_out) {
  if (!n_heads || !conn_offs || (n_conns && (!conn_status || !conn_consumed || !conn_state_out)) ||
      (wire_bytes && !wire) || (cap_heads && (!head_offs || !head_conn)) || n_conns > 0xffffffffull)
    return L7M_EINVAL;
  *n_heads = 0;
  if (!conns_ok(conn_offs, n_conns, wire_bytes)) return L7M_EINVAL;
  // Counting leaves the states where they are (the arrays may alias); the emit
  // walk, or a walk for the state alone, stores them.
  size_t total = 0;
  for (size_t c = 0; c < n_conns; ++c) {
    l7m_stream_state st = conn_state_in ? conn_state_in[c] : l7m_stream_state{0, 0, 0};
    conn_status[c] = http_stream_walk_resume(HostSrc{wire + conn_offs[c]}, conn_offs[c + 1] - conn_offs[c], st,
                                             &conn_consumed[c], [&](uint64_t) { ++total; });
  }
  *n_heads = total;
  const bool emit = total <= cap_heads && head_offs;
  size_t i = 0;
  for (size_t c = 0; c < n_conns; ++c) {
    l7m_stream_state st = conn_state_in ? conn_state_in[c] : l7m_stream_state{0, 0, 0};
    uint64_t used;
    http_stream_walk_resume(HostSrc{wire + conn_offs[c]}, conn_offs[c + 1] - conn_offs[c], st, &used,
                            [&](uint64_t start) {
                              if (!emit) return;
                              head_offs[i] = conn_offs[c] + start;
                              head_conn[i] = static_cast<uint32_t>(c);
                              if (head_meta) {
                                if (conn_meta) head_meta[i] = conn_meta[c];
                                else head_meta[i] = l7m_http_wire_meta{0, 0, 0, 1, {0, 0, 0}};
                              }
                              ++i;
                            });
    conn_state_out[c] = st;
  }
  if (total > cap_heads) return L7M_ENOMEM;
  if (head_offs) head_offs[total] = conn_offs[n_conns];
  return L7M_OK;
}

size_t l7m_stream_carry_bound(size_t wire_bytes, size_t seg_bytes) { return wire_bytes + seg_bytes; }

int l7m_stream_carry(const uint8_t* wire, size_t wire_bytes, const uint64_t* conn_offs, size_t n_prev,
                     const int32_t* conn_status, const uint64_t* conn_consumed, const uint8_t* seg, size_t seg_bytes,
                     const uint64_t* seg_offs, size_t n_conns, l7m_stream_state* conn_state, uint8_t* next_wire,
                     size_t cap_bytes, uint64_t* next_conn_offs, uint64_t* next_bytes) {
  if (!next_bytes || !seg_offs || n_prev > n_conns || (n_prev && (!conn_offs || !conn_status || !conn_consumed)) ||
      (wire_bytes && !wire) || (seg_bytes && !seg) || (cap_bytes && (!next_wire || !next_conn_offs)))
    return L7M_EINVAL;
  *next_bytes = 0;
  if (n_prev && !conns_ok(conn_offs, n_prev, wire_bytes)) return L7M_EINVAL;
  if (!conns_ok(seg_offs, n_conns, seg_bytes)) return L7M_EINVAL;
  for (size_t c = 0; c < n_prev; ++c)
    if (conn_consumed[c] > conn_offs[c + 1] - conn_offs[c]) return L7M_EINVAL;
  auto plan = [&](size_t c) {
    const int32_t mode = conn_state ? conn_state[c].mode : L7M_STREAM_MODE_HEAD;
    const uint64_t left = conn_state ? conn_state[c].left : 0;
    return c < n_prev ? stream_carry_plan(conn_offs[c], conn_offs[c + 1], conn_consumed[c], conn_status[c],
                                          seg_offs[c], seg_offs[c + 1], mode, left)
                      : stream_carry_plan(0, 0, 0, L7M_STREAM_OK, seg_offs[c], seg_offs[c + 1], mode, left);
  };
  uint64_t total = 0;
  for (size_t c = 0; c < n_conns; ++c) {
    const CarryPlan pl = plan(c);
    total += pl.tlen + pl.nlen;
  }
  *next_bytes = total;
  if (total > cap_bytes) return L7M_ENOMEM;
  if (!next_conn_offs) return L7M_OK;  // the sizing call
  uint64_t used = 0;
  for (size_t c = 0; c < n_conns; ++c) {
    const CarryPlan pl = plan(c);
    next_conn_offs[c] = used;
    if (pl.tlen) std::memcpy(next_wire + used, wire + pl.tsrc, pl.tlen);
    if (pl.nlen) std::memcpy(next_wire + used + pl.tlen, seg + pl.nsrc, pl.nlen);
    used += pl.tlen + pl.nlen;
    if (conn_state) stream_carry_state(conn_state[c], pl.skip);
  }
  next_conn_offs[n_conns] = used;
  return L7M_OK;
}

}  // extern "C"
