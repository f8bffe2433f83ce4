// l7m_kafka_side.h — what follows the verdict of a Kafka request: the walk
// over the request that the deny response
// (CreateResponse(ErrTopicAuthorizationFailed), pkg/kafka/request.go:158-182,
// pkg/kafka/response.go, serialised as optiopay's Resp.Bytes(version)) and the
// per-topic log records (kafkaLogRecord.log, pkg/proxy/kafka.go:168-230) are
// made from, written once for the host functions (l7m_side.cc) and the device
// encoders (l7m_kafka_side.hip): both instantiate these templates, so a request
// gives the same bytes on either side.
//
// The arena is read through a Src addressed by arena offset
// (`uint8_t at(uint64_t i) const`, for i inside the validated request only), a
// response is written through a Sink (`void put(uint8_t)`, bytes in response
// order), and a message's CRC-32 (IEEE) advances through a Crc
// (`uint32_t operator()(uint32_t crc, uint8_t byte) const`: the bitwise loop
// KafkaCrcBitwise here, a table where there is room for one).
//   kafka_rec         the size-prefixed request at an offset, if it lies in the arena
//   kafka_walk        header, topics and partitions of a request, handed to a visitor
//   KafkaRespSize     visitor: the response's size, from the walk alone
//   KafkaRespEmit     visitor: the response's bytes, KafkaRespSize of them
//   KafkaTopicCount   visitor: the number of log records
//   kafka_log_fill    the fields of one log record
// Nothing here keeps a list of topics: a visitor sees each topic and partition
// as the walk reads it, so a caller that needs sizes before bytes walks twice.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/l7match.h"
#include "l7m_http_log.h"
#include "program.h"

namespace l7m {

constexpr int kErrTopicAuthorizationFailed = 29;  // vendor/.../proto/errors.go:37
// time.Time{}.UnixNano() / int64(time.Millisecond) on a 64-bit Go: the zero
// Time's nanoseconds overflow int64 and wrap (OffsetResp v>=1 TimeStamp).
constexpr int64_t kZeroTimeMillis = -6795364578871LL;

// The request at arena offset `o`: its size field and the bytes it counts;
// false if either does not fit the arena.  *len = the request with its size
// field.
template <class Src>
L7M_LOG_FN bool kafka_rec(const Src& s, uint64_t arena_bytes, uint64_t o, uint64_t* len) {
  if (o > arena_bytes || arena_bytes - o < 4) return false;
  const uint64_t sz = static_cast<uint64_t>(s.at(o)) << 24 | static_cast<uint64_t>(s.at(o + 1)) << 16 |
                      static_cast<uint64_t>(s.at(o + 2)) << 8 | s.at(o + 3);
  if (sz > arena_bytes - o - 4) return false;
  *len = sz + 4;
  return true;
}

// Big-endian reader of arena[base, base + n) with optiopay's sticky-error
// semantics: a read past the end sets err and consumes the rest, and every
// later read gives zero.  A length is checked against what is left before the
// position moves, so pos <= n always.
template <class Src>
struct KafkaRd {
  const Src& s;
  uint64_t base, n, pos;
  bool err;
  L7M_LOG_FN KafkaRd(const Src& src, uint64_t b, uint64_t len) : s(src), base(b), n(len), pos(0), err(false) {}
  L7M_LOG_FN uint64_t be(uint32_t k) {
    if (err || n - pos < k) {
      err = true;
      pos = n;
      return 0;
    }
    uint64_t v = 0;
    for (uint32_t i = 0; i < k; ++i) v = v << 8 | s.at(base + pos + i);
    pos += k;
    return v;
  }
  L7M_LOG_FN int16_t i16() { return static_cast<int16_t>(be(2)); }
  L7M_LOG_FN int32_t i32() { return static_cast<int32_t>(be(4)); }
  // DecodeString: int16 length, < 1 -> "".  Returns the length; *at = the
  // position of the first byte.
  L7M_LOG_FN uint32_t str(uint64_t* at = nullptr) {
    const int16_t k = i16();
    if (at) *at = pos;
    if (err || k < 1) return 0;
    if (n - pos < static_cast<uint64_t>(k)) {
      err = true;
      pos = n;
      return 0;
    }
    pos += static_cast<uint64_t>(k);
    return static_cast<uint32_t>(k);
  }
  L7M_LOG_FN void skip(uint64_t k) {
    if (err || n - pos < k) {
      err = true;
      pos = n;
      return;
    }
    pos += k;
  }
  L7M_LOG_FN int32_t arraylen() {
    const int32_t v = i32();
    if (v < 0 || v > kKafkaMaxParseBuf) err = true;
    return err ? 0 : v;
  }
};

struct KafkaCrcBitwise {
  L7M_LOG_FN uint32_t operator()(uint32_t c, uint8_t b) const {
    c ^= b;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
  }
};

// Bytes readMessageSet (messages.go:357-483) consumes from its LimitReader of
// `size` bytes over arena[p, p + avail): it can stop inside the set (a bad CRC,
// attributes 3), and the request's next partition is then read from there.
template <class Src, class Crc>
L7M_LOG_FN uint64_t kafka_message_set_consumed(const Src& s, uint64_t p, uint64_t avail, int32_t size,
                                               const Crc& crc) {
  const uint64_t lim = avail < static_cast<uint64_t>(size) ? avail : static_cast<uint64_t>(size);
  uint64_t pos = 0;
  for (;;) {
    if (lim - pos < 12) return lim;  // offset / size: short reads consume the rest
    pos += 8;
    const int32_t msz =
        static_cast<int32_t>(static_cast<uint32_t>(s.at(p + pos)) << 24 | static_cast<uint32_t>(s.at(p + pos + 1)) << 16 |
                             static_cast<uint32_t>(s.at(p + pos + 2)) << 8 | s.at(p + pos + 3));
    pos += 4;
    if (msz <= 0) return pos;
    if (lim - pos < static_cast<uint64_t>(msz)) return lim;
    const uint64_t m = p + pos;  // the message: crc, magic, attributes, ...
    pos += static_cast<uint64_t>(msz);
    if (msz <= 4) return pos;
    uint32_t c = 0xffffffffu;
    for (int32_t i = 4; i < msz; ++i) c = crc(c, s.at(m + static_cast<uint64_t>(i)));
    const uint32_t want = static_cast<uint32_t>(s.at(m)) << 24 | static_cast<uint32_t>(s.at(m + 1)) << 16 |
                          static_cast<uint32_t>(s.at(m + 2)) << 8 | s.at(m + 3);
    if ((c ^ 0xffffffffu) != want) return pos;
    if (msz > 5 && (s.at(m + 5) & 3) == 3) return pos;  // attributes: an unknown codec
  }
}

// The header of a request (pkg/kafka/request.go:88-108 over optiopay's
// per-kind readers).
struct KafkaHead {
  int16_t kind, version;
  int32_t corr;
};

// Walks the request arena[off, off + len) (its size field included; the field
// is not compared with len here).  Returns L7M_OK, L7M_EINVAL (decode error) or
// L7M_EUNSUPPORTED (request == nil: a kind ReadRequest leaves untyped,
// request.go:204-220).  The visitor sees, in request order:
//   v.topics(h, nt)             once, before the first topic (nt = 0 for a
//                               kind without a topic array)
//   v.topic(h, at, nl, np)      a topic: its name arena[at, at + nl), np
//                               partitions (0 for a Metadata request's names)
//   v.partition(h, id)          a partition of the topic seen last
//   v.end(h)                    once, after the last topic
// When the result is not L7M_OK the visitor may have seen a part of the
// request only and what it gathered is void.  When it is, it saw exactly nt
// topics and np partitions of each.  Every loop here consumes at least two
// bytes of the request per round or ends, so the walk is bounded by len.
template <class Src, class Crc, class V>
L7M_LOG_FN int kafka_walk(const Src& s, uint64_t off, uint64_t len, const Crc& crc, KafkaHead& h, V& v) {
  KafkaRd<Src> r(s, off, len);
  r.i32();  // size
  h.kind = r.i16();
  h.version = r.i16();
  h.corr = r.i32();
  if (r.err) return L7M_EINVAL;
  const int16_t version = h.version;
  r.str();  // ClientID
  // what a partition carries behind its id: `fixed` bytes, a message set, or
  // the offset / metadata of a commit; names: a topic is its name alone
  uint64_t fixed = 0;
  bool produce = false, commit = false, names = false;
  switch (h.kind) {
    case 0:  // ReadProduceReq
      if (version >= 3) r.str();
      r.skip(6);
      produce = true;
      break;
    case 1:  // ReadFetchReq
      r.skip(12u + (version >= 3 ? 4u : 0u) + (version >= 4 ? 1u : 0u));
      fixed = 12u + (version >= 5 ? 8u : 0u);
      break;
    case 2:  // ReadOffsetReq
      r.skip(4u + (version >= 2 ? 1u : 0u));
      fixed = 8u + (version == 0 ? 4u : 0u);
      break;
    case 3:  // ReadMetadataReq
      names = true;
      break;
    case 8:  // ReadOffsetCommitReq
      r.str();
      if (version >= 1) {
        r.skip(4);
        r.str();
      }
      if (version >= 2) r.skip(8);
      commit = true;
      break;
    case 9:  // ReadOffsetFetchReq
      r.str();
      break;
    case 10:  // ReadConsumerMetadataReq
      r.str();
      if (version >= 1) r.skip(1);
      v.topics(h, 0);
      v.end(h);
      return r.err ? L7M_EINVAL : L7M_OK;
    default:
      return L7M_EUNSUPPORTED;
  }
  const int32_t nt = r.arraylen();
  v.topics(h, nt);
  for (int32_t k = 0; k < nt && !r.err; ++k) {
    uint64_t at = 0;
    const uint32_t nl = r.str(&at);
    if (names) {
      v.topic(h, off + at, nl, 0);
      continue;
    }
    const int32_t np = r.arraylen();
    v.topic(h, off + at, nl, np);
    for (int32_t j = 0; j < np && !r.err; ++j) {
      v.partition(h, r.i32());
      if (produce) {
        const int32_t sz = r.i32();
        if (r.err) break;
        if (sz < 0 || sz > kKafkaMaxParseBuf) r.err = true;
        else r.pos += kafka_message_set_consumed(s, off + r.pos, r.n - r.pos, sz, crc);
      } else if (commit) {
        r.skip(8u + (version == 1 ? 8u : 0u));
        r.str();
      } else {
        r.skip(fixed);
      }
    }
  }
  v.end(h);
  return r.err ? L7M_EINVAL : L7M_OK;
}

// ---- the deny response ------------------------------------------------------
// Resp.Bytes(version) of the response CreateResponse builds: every topic and
// partition of the request with ErrTopicAuthorizationFailed, everything else
// zero (ProduceResp messages.go:1697, FetchResp :896, OffsetResp :1956,
// MetadataResp :595, OffsetCommitResp :1327, OffsetFetchResp :1512,
// ConsumerMetadataResp :1102).  The sizes of its parts:
L7M_LOG_FN uint64_t kafka_resp_head_bytes(const KafkaHead& h) {  // size, correlation id, up to the topic count
  const int v = h.version;
  switch (h.kind) {
    case 0: return 8u + 4u;
    case 1: return 8u + (v >= 1 ? 4u : 0u) + 4u;
    case 2: return 8u + (v >= 2 ? 4u : 0u) + 4u;
    case 3: return 8u + (v >= 3 ? 4u : 0u) + 4u + (v >= 2 ? 2u : 0u) + (v >= 1 ? 4u : 0u) + 4u;
    case 8: return 8u + (v >= 3 ? 4u : 0u) + 4u;
    case 9: return 8u + (v >= 3 ? 4u : 0u) + 4u;
    default: return 8u;
  }
}
L7M_LOG_FN uint64_t kafka_resp_topic_bytes(const KafkaHead& h, uint32_t name_len) {
  if (h.kind == 3) return 2u + 2u + name_len + (h.version >= 1 ? 1u : 0u) + 4u;
  return 2u + name_len + 4u;
}
L7M_LOG_FN uint64_t kafka_resp_partition_bytes(const KafkaHead& h) {
  const int v = h.version;
  switch (h.kind) {
    case 0: return 4u + 2u + 8u + (v >= 2 ? 8u : 0u);
    case 1: return 4u + 2u + 8u + (v >= 4 ? 8u + (v >= 5 ? 8u : 0u) + 4u : 0u) + 4u;
    case 2: return 4u + 2u + (v >= 1 ? 8u : 0u) + 4u;
    case 8: return 4u + 2u;
    case 9: return 4u + 8u + 2u + 2u;
    default: return 0u;
  }
}
L7M_LOG_FN uint64_t kafka_resp_tail_bytes(const KafkaHead& h) {
  const int v = h.version;
  switch (h.kind) {
    case 0: return v >= 1 ? 4u : 0u;
    case 9: return v >= 2 ? 2u : 0u;
    case 10: return (v >= 1 ? 4u : 0u) + 2u + (v >= 1 ? 2u : 0u) + 4u + 2u + 4u;
    default: return 0u;
  }
}

struct KafkaRespSize {
  uint64_t bytes = 0;
  L7M_LOG_FN void topics(const KafkaHead& h, int32_t) { bytes += kafka_resp_head_bytes(h); }
  L7M_LOG_FN void topic(const KafkaHead& h, uint64_t, uint32_t nl, int32_t) { bytes += kafka_resp_topic_bytes(h, nl); }
  L7M_LOG_FN void partition(const KafkaHead& h, int32_t) { bytes += kafka_resp_partition_bytes(h); }
  L7M_LOG_FN void end(const KafkaHead& h) { bytes += kafka_resp_tail_bytes(h); }
};

// The response's bytes into a sink; `size` is what KafkaRespSize gave for the
// same request (the size field comes first).  But for the names, a response is
// zeros with a few big-endian values in them, so each part is written as one
// run of the length its kafka_resp_*_bytes function gives: what is emitted is
// what was measured, and a sink's put() is instantiated a handful of times.
struct KafkaRespField {  // `len` bytes of `v`, big-endian, at byte `at` of a run
  uint64_t v;
  uint32_t at, len;
};
template <class Src, class Sink>
struct KafkaRespEmit {
  Src s;
  Sink k;  // the visitor's own: read it back from here after the walk
  uint64_t size;
  L7M_LOG_FN KafkaRespEmit(const Src& src, const Sink& sink, uint64_t bytes) : s(src), k(sink), size(bytes) {}
  L7M_LOG_FN static KafkaRespField i16(int v, uint32_t at) { return KafkaRespField{static_cast<uint16_t>(v), at, 2}; }
  L7M_LOG_FN static KafkaRespField i32(int64_t v, uint32_t at) { return KafkaRespField{static_cast<uint32_t>(v), at, 4}; }
  L7M_LOG_FN static KafkaRespField none() { return KafkaRespField{0, 0, 0}; }
  // n bytes: zero outside the three fields (j - at wraps for j < at)
  L7M_LOG_FN void run(uint32_t n, const KafkaRespField& a, const KafkaRespField& b, const KafkaRespField& c) {
    for (uint32_t j = 0; j < n; ++j) {
      uint64_t x = 0;
      if (j - a.at < a.len) x = a.v >> (8u * (a.len - 1u - (j - a.at)));
      if (j - b.at < b.len) x = b.v >> (8u * (b.len - 1u - (j - b.at)));
      if (j - c.at < c.len) x = c.v >> (8u * (c.len - 1u - (j - c.at)));
      k.put(static_cast<uint8_t>(x));
    }
  }
  // size, correlation id, ThrottleTime / Brokers / ClusterID "" / ControllerID
  // where the version has them (all zero), the topic count
  L7M_LOG_FN void topics(const KafkaHead& h, int32_t nt) {
    const uint32_t n = static_cast<uint32_t>(kafka_resp_head_bytes(h));
    run(n, i32(static_cast<int64_t>(size - 4), 0), i32(h.corr, 4), n > 8 ? i32(nt, n - 4) : none());
  }
  // Encode(string) of the name (uint16 length + bytes) and the partition
  // count; Metadata: the error code before the name, IsInternal (v >= 1) and
  // an empty partition array behind it
  L7M_LOG_FN void topic(const KafkaHead& h, uint64_t at, uint32_t nl, int32_t np) {
    const bool md = h.kind == 3;
    run(md ? 4u : 2u, md ? i16(kErrTopicAuthorizationFailed, 0) : none(), i16(static_cast<int>(nl), md ? 2u : 0u), none());
    for (uint32_t i = 0; i < nl; ++i) k.put(s.at(at + i));
    run(static_cast<uint32_t>(kafka_resp_topic_bytes(h, nl)) - nl - (md ? 4u : 2u), md ? none() : i32(np, 0), none(),
        none());
  }
  // the id, the error code behind it (OffsetFetch: behind Offset and Metadata
  // "", at the end), OffsetResp v >= 1: TimeStamp of the zero Time; Offset,
  // LogAppendTime, TipOffset, LastStableOffset, LogStartOffset,
  // AbortedTransactions, the message set size, Offsets: zero
  L7M_LOG_FN void partition(const KafkaHead& h, int32_t id) {
    const uint32_t n = static_cast<uint32_t>(kafka_resp_partition_bytes(h));
    run(n, i32(id, 0), i16(kErrTopicAuthorizationFailed, h.kind == 9 ? n - 2 : 4u),
        h.kind == 2 && h.version >= 1 ? KafkaRespField{static_cast<uint64_t>(kZeroTimeMillis), 6, 8} : none());
  }
  // Produce v >= 1: ThrottleTime; OffsetFetch v >= 2: resp.Err, left nil by
  // createOffsetFetchResponse; ConsumerMetadata: ThrottleTime (v >= 1), the
  // error code, ErrMsg "" (v >= 1), CoordinatorID, CoordinatorHost "",
  // CoordinatorPort
  L7M_LOG_FN void end(const KafkaHead& h) {
    run(static_cast<uint32_t>(kafka_resp_tail_bytes(h)),
        h.kind == 10 ? i16(kErrTopicAuthorizationFailed, h.version >= 1 ? 4u : 0u) : none(), none(), none());
  }
};

// ---- the log records --------------------------------------------------------
// Whether a request with this verdict is logged at all: not one ReadRequest
// rejected (the connection is closed, pkg/proxy/kafka.go:349-354), nor -3 (a
// codec limit of this library); under a `select` of L7M_LOG_FORWARDED |
// L7M_LOG_DENIED only the records of that FlowVerdict (0: every record).
L7M_LOG_FN bool kafka_log_wanted(int32_t verdict, uint32_t select) {
  if (verdict == L7M_VERDICT_PARSE_ERROR || verdict == L7M_VERDICT_UNSUPPORTED) return false;
  if (!select) return true;
  const uint32_t fv = flow_verdict(verdict);
  return fv == 0 ? (select & L7M_LOG_FORWARDED) != 0 : fv == 1 ? (select & L7M_LOG_DENIED) != 0 : false;
}

struct KafkaTopicCount {  // one record per topic (kafka.go:207-211)
  uint64_t topics_seen = 0;
  L7M_LOG_FN void topics(const KafkaHead&, int32_t) {}
  L7M_LOG_FN void topic(const KafkaHead&, uint64_t, uint32_t, int32_t) { ++topics_seen; }
  L7M_LOG_FN void partition(const KafkaHead&, int32_t) {}
  L7M_LOG_FN void end(const KafkaHead&) {}
};

// The record of one topic of request `request`: allowed -> Forwarded /
// ErrNone; denied -> Denied / ErrTopicAuthorizationFailed, since
// CreateResponse succeeds for every typed request (kafka.go:240-262,296).
L7M_LOG_FN void kafka_log_fill(l7m_kafka_log_record& r, uint64_t request, int32_t verdict, const KafkaHead& h,
                               uint64_t topic_off, uint32_t topic_len) {
  const uint32_t fv = flow_verdict(verdict);
  r.request = request;
  r.verdict = fv;
  r.error_code = fv == 1 ? kErrTopicAuthorizationFailed : 0;
  r.api_key = h.kind;
  r.api_version = h.version;
  r.correlation_id = h.corr;
  r.topic_off = topic_off;
  r.topic_len = topic_len;
  r.pad = 0;
}

}  // namespace l7m
