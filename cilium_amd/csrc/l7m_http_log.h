// l7m_http_log.h — the HttpLogEntry serialisation of a decided HTTP record
// (include/l7match.h l7m_http_access_log; envoy/accesslog.cc:59-170,
// envoy/cilium/accesslog.proto), written once for the host function
// (l7m_side.cc) and the device encoder (l7m_http_log.hip): both instantiate
// these templates, so a record serialises to the same bytes on either side.
//
// The arena is read through a Src addressed by arena offset
// (`uint8_t at(uint64_t i) const`, `uint32_t word(uint64_t i) const` for a
// 4-aligned i, both for i inside [0, arena_bytes) only) and an entry is
// written through a Sink (`void put(uint8_t)`, bytes in entry order).  The
// parts of an entry that are the same for every request of a call (fields 1-2,
// 4 and 7-8) arrive pre-serialised in a Consts (`head`, `policy`, `addrs`
// indexable bytes with `head_len`, `policy_len`, `addrs_len`, and
// `local_identity`).
//   log_view     validates a record and reads its fixed part
//   log_measure  the entry's size, from lengths alone
//   log_emit     the entry's bytes, log_measure of them
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/l7match.h"

#if defined(__HIP__)
#define L7M_LOG_FN __host__ __device__ inline
#else
#define L7M_LOG_FN inline
#endif

namespace l7m {

// A validated record: its offset and fixed part.  The directory starts at
// off + L7M_HTTP_REC_FIXED, the method behind it, then path, authority and
// the first header name.
struct LogView {
  uint64_t off;
  uint32_t remote_id, dport, flags, nhdr, mlen, plen, alen;
};

L7M_LOG_FN uint64_t log_dir(const LogView& v) { return v.off + L7M_HTTP_REC_FIXED; }
L7M_LOG_FN uint64_t log_method(const LogView& v) { return log_dir(v) + 4ull * v.nhdr; }
L7M_LOG_FN uint64_t log_path(const LogView& v) { return log_method(v) + v.mlen; }
L7M_LOG_FN uint64_t log_authority(const LogView& v) { return log_path(v) + v.plen; }
L7M_LOG_FN uint64_t log_names(const LogView& v) { return log_authority(v) + v.alen; }

// False if the record at `off` is malformed.  The checks run in this order and
// no byte outside [0, arena_bytes) is read: the offset is 4-aligned; the fixed
// part lies inside the arena; rec_len lies inside the arena; the fixed part,
// the directory and the three fields fit rec_len (so the directory lies inside
// the record before an entry of it is read); everything sums to rec_len.
template <class Src>
L7M_LOG_FN bool log_view(const Src& s, uint64_t arena_bytes, uint64_t off, LogView& v) {
  if ((off & 3) || off > arena_bytes || arena_bytes - off < L7M_HTTP_REC_FIXED) return false;
  const uint32_t rec_len = s.word(off);
  if (rec_len > arena_bytes - off) return false;
  const uint32_t w2 = s.word(off + 8), w3 = s.word(off + 12), w4 = s.word(off + 16);
  v.off = off;
  v.remote_id = s.word(off + 4);
  v.dport = w2 & 0xffffu;
  v.flags = (w2 >> 16) & 0xffu;
  v.nhdr = w2 >> 24;
  v.mlen = w3 & 0xffffu;
  v.plen = w3 >> 16;
  v.alen = w4 & 0xffffu;
  uint64_t need = L7M_HTTP_REC_FIXED + 4ull * v.nhdr + v.mlen + v.plen + v.alen;
  if (need > rec_len) return false;
  for (uint32_t j = 0; j < v.nhdr; ++j) {
    const uint32_t e = s.word(log_dir(v) + 4ull * j);
    need += (e & 0xffffu) + (e >> 16);
  }
  return need == rec_len;
}

// FlowVerdict of a decided request: 0 Forwarded, 1 Denied, 2 Error.
L7M_LOG_FN uint32_t flow_verdict(int32_t v) { return v >= 0 ? 0u : v == L7M_VERDICT_DENY ? 1u : 2u; }

// Whether a request with this verdict gets an entry under `select`
// (L7M_LOG_FORWARDED | L7M_LOG_DENIED): never at or below
// L7M_VERDICT_PARSE_ERROR.
L7M_LOG_FN bool log_wanted(int32_t verdict, uint32_t select) {
  const uint32_t fv = flow_verdict(verdict);
  return fv == 0 ? (select & L7M_LOG_FORWARDED) != 0 : fv == 1 ? (select & L7M_LOG_DENIED) != 0 : false;
}

// Protobuf wire format, proto3: a zero or empty field is omitted.  Every field
// number here is below 16, so a key is one byte.
L7M_LOG_FN uint32_t log_varint_len(uint64_t v) {
  uint32_t k = 1;
  for (; v >= 0x80; v >>= 7) ++k;
  return k;
}
L7M_LOG_FN uint64_t log_u64_len(uint64_t v) { return v ? 1u + log_varint_len(v) : 0u; }
L7M_LOG_FN uint64_t log_bytes_len(uint64_t n) { return n ? 1u + log_varint_len(n) + n : 0u; }

template <class Sink>
L7M_LOG_FN void log_put_varint(Sink& k, uint64_t v) {
  for (; v >= 0x80; v >>= 7) k.put(static_cast<uint8_t>(v | 0x80));
  k.put(static_cast<uint8_t>(v));
}
template <class Sink>
L7M_LOG_FN void log_put_u64(Sink& k, uint32_t field, uint64_t v) {
  if (!v) return;
  k.put(static_cast<uint8_t>(field << 3));
  log_put_varint(k, v);
}
template <class Src, class Sink>
L7M_LOG_FN void log_put_bytes(Sink& k, uint32_t field, const Src& s, uint64_t pos, uint64_t n) {
  if (!n) return;
  k.put(static_cast<uint8_t>(field << 3 | 2));
  log_put_varint(k, n);
  for (uint64_t i = 0; i < n; ++i) k.put(s.at(pos + i));
}

template <class Src>
L7M_LOG_FN bool log_is_scheme_name(const Src& s, uint64_t pos, uint32_t name_len) {
  if (name_len != 17) return false;
  for (uint32_t i = 0; i < 17; ++i)
    if (s.at(pos + i) != static_cast<uint8_t>("x-forwarded-proto"[i])) return false;
  return true;
}

// The headers of a record: the value of the last x-forwarded-proto (field 9)
// and the bytes the others take as field-14 submessages (accesslog.cc:103-131).
struct LogHeaders {
  uint64_t scheme_pos;
  uint32_t scheme_len;
  uint64_t kv_bytes;
};

L7M_LOG_FN uint64_t log_kv_len(uint32_t name_len, uint32_t value_len) {
  return log_bytes_len(name_len) + log_bytes_len(value_len);
}

template <class Src>
L7M_LOG_FN void log_headers(const Src& s, const LogView& v, LogHeaders& h) {
  h.scheme_pos = 0;
  h.scheme_len = 0;
  h.kv_bytes = 0;
  uint64_t pos = log_names(v);
  for (uint32_t j = 0; j < v.nhdr; ++j) {
    const uint32_t e = s.word(log_dir(v) + 4ull * j);
    const uint32_t nl = e & 0xffffu, vl = e >> 16;
    if (log_is_scheme_name(s, pos, nl)) {
      h.scheme_pos = pos + nl;
      h.scheme_len = vl;
    } else {
      const uint64_t kv = log_kv_len(nl, vl);
      h.kv_bytes += 1u + log_varint_len(kv) + kv;
    }
    pos += nl + vl;
  }
}

L7M_LOG_FN uint32_t log_source_id(const LogView& v, uint32_t local_identity) {
  return (v.flags & L7M_HTTP_F_INGRESS) ? v.remote_id : local_identity;  // SocketMarkOption identity_ (the source)
}

// Bytes of the entry of a valid record whose verdict is above
// L7M_VERDICT_PARSE_ERROR.
template <class Src, class Consts>
L7M_LOG_FN uint64_t log_measure(const Src& s, const LogView& v, int32_t verdict, const Consts& c) {
  const bool denied = verdict == L7M_VERDICT_DENY;
  LogHeaders h;
  log_headers(s, v, h);
  uint64_t b = static_cast<uint64_t>(c.head_len) + c.policy_len + c.addrs_len + h.kv_bytes;
  b += denied ? 2u + 3u : 0u;  // fields 3 and 13
  b += log_u64_len(log_source_id(v, c.local_identity));
  b += log_bytes_len(h.scheme_len);
  if (v.flags & L7M_HTTP_F_AUTHORITY) b += log_bytes_len(v.alen);
  if (v.flags & L7M_HTTP_F_PATH) b += log_bytes_len(v.plen);
  if (v.flags & L7M_HTTP_F_METHOD) b += log_bytes_len(v.mlen);
  if (v.flags & L7M_HTTP_F_INGRESS) b += 2u;  // field 15
  return b;
}

// The entry, fields in the order SerializeToString emits them (accesslog.proto
// numbers; 5 cilium_rule_ref is not set by this reference's filter).
template <class Src, class Consts, class Sink>
L7M_LOG_FN void log_emit(const Src& s, const LogView& v, int32_t verdict, const Consts& c, Sink& k) {
  const bool denied = verdict == L7M_VERDICT_DENY;
  LogHeaders h;
  log_headers(s, v, h);
  for (uint32_t i = 0; i < c.head_len; ++i) k.put(c.head[i]);      // 1 timestamp, 2 http_protocol
  log_put_u64(k, 3, denied ? 2u : 0u);  // EntryType Denied (encodeHeaders of the 403) / Request
  for (uint32_t i = 0; i < c.policy_len; ++i) k.put(c.policy[i]);  // 4 policy_name
  log_put_u64(k, 6, log_source_id(v, c.local_identity));
  for (uint32_t i = 0; i < c.addrs_len; ++i) k.put(c.addrs[i]);    // 7 source_address, 8 destination_address
  log_put_bytes(k, 9, s, h.scheme_pos, h.scheme_len);
  if (v.flags & L7M_HTTP_F_AUTHORITY) log_put_bytes(k, 10, s, log_authority(v), v.alen);
  if (v.flags & L7M_HTTP_F_PATH) log_put_bytes(k, 11, s, log_path(v), v.plen);
  if (v.flags & L7M_HTTP_F_METHOD) log_put_bytes(k, 12, s, log_method(v), v.mlen);
  log_put_u64(k, 13, denied ? 403u : 0u);  // responseCode of the local reply
  uint64_t pos = log_names(v);
  for (uint32_t j = 0; j < v.nhdr; ++j) {  // 14 headers, in request order
    const uint32_t e = s.word(log_dir(v) + 4ull * j);
    const uint32_t nl = e & 0xffffu, vl = e >> 16;
    if (!log_is_scheme_name(s, pos, nl)) {
      k.put(14u << 3 | 2u);
      log_put_varint(k, log_kv_len(nl, vl));
      log_put_bytes(k, 1, s, pos, nl);
      log_put_bytes(k, 2, s, pos + nl, vl);
    }
    pos += nl + vl;
  }
  log_put_u64(k, 15, (v.flags & L7M_HTTP_F_INGRESS) ? 1u : 0u);
}

// The constant parts as the device encoder carries them: kernel arguments, so
// each string is limited to kLogStringMax bytes there.
constexpr uint32_t kLogStringMax = 255;
struct LogConstsFixed {
  uint8_t head[20];                          // <= (1 + 10) + (1 + 5)
  uint8_t policy[3 + kLogStringMax + 2];     // <= 1 + 2 + 255
  uint8_t addrs[2 * (3 + kLogStringMax) + 4];
  uint32_t head_len, policy_len, addrs_len, local_identity;
};

// Keys of the proxy-statistics counters the device fills
// (l7m_proxy_stats_update_device): ((ingress * 65536 + port) * 3 + FlowVerdict).
constexpr uint32_t kStatsClasses = 3;
constexpr uint32_t kStatsRows = 2u * 65536u;
constexpr uint32_t kStatsCounters = kStatsRows * kStatsClasses;

}  // namespace l7m
