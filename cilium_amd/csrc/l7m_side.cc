// l7m_side.cc — verdict side effects on the host (include/l7match.h):
//   * the 403 body Envoy's filter sends on deny (envoy/cilium_l7policy.cc:89-95,
//     169-181);
//   * the Kafka response the proxy sends for a denied request:
//     (*RequestMessage).CreateResponse(proto.ErrTopicAuthorizationFailed)
//     (pkg/kafka/request.go:158-182, pkg/kafka/response.go:81-303) serialised
//     as optiopay's Resp.Bytes(version) (vendor/.../proto/messages.go:595,
//     896, 1102, 1327, 1512, 1697, 1956);
//   * per-endpoint proxy statistics from a batch of verdicts
//     (Endpoint.UpdateProxyStatistics, pkg/endpoint/endpoint.go:2099-2122),
//     flat (l7m_proxy_stats_add) or keyed by (protocol, port, direction,
//     request) as the endpoint keeps them (l7m_proxy_stats_table);
//   * access-log records: the HttpLogEntry protobuf the Envoy filter sends
//     per request (envoy/accesslog.cc:59-170, cilium_l7policy.cc:166-191,
//     envoy/cilium/accesslog.proto) and the Kafka proxy's per-topic log
//     records (pkg/proxy/kafka.go:168-230, pkg/proxy/accesslog/record.go
//     :200-241, pkg/proxy/logger/logger.go:84-357).
// These run only for requests the GPU already decided; no verdict is
// computed here.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/l7match.h"
#include "l7m_http_log.h"
#include "l7m_internal.h"
#include "program.h"

namespace {

// Big-endian request reader with optiopay's sticky-error semantics.
struct Rd {
  const uint8_t* p;
  size_t n, pos = 0;
  bool err = false;
  uint64_t be(size_t k) {
    if (err || n - pos < k) {
      err = true;
      pos = n;
      return 0;
    }
    uint64_t v = 0;
    for (size_t i = 0; i < k; ++i) v = v << 8 | p[pos + i];
    pos += k;
    return v;
  }
  int16_t i16() { return static_cast<int16_t>(be(2)); }
  int32_t i32() { return static_cast<int32_t>(be(4)); }
  std::string str(size_t* at = nullptr) {  // DecodeString: int16 length, < 1 -> ""
    const int16_t k = i16();
    if (at) *at = pos;
    if (err || k < 1) return "";
    if (n - pos < static_cast<size_t>(k)) {
      err = true;
      pos = n;
      return "";
    }
    std::string s(reinterpret_cast<const char*>(p + pos), static_cast<size_t>(k));
    pos += static_cast<size_t>(k);
    return s;
  }
  void skip(size_t k) {
    if (err || n - pos < k) {
      err = true;
      pos = n;
      return;
    }
    pos += k;
  }
  int32_t arraylen() {
    const int32_t v = i32();
    if (v < 0 || v > l7m::kKafkaMaxParseBuf) err = true;
    return err ? 0 : v;
  }
  void bytes() {  // DecodeBytes, value discarded
    const int32_t k = i32();
    if (err || k < 1) return;
    if (k > l7m::kKafkaMaxParseBuf || n - pos < static_cast<size_t>(k)) {
      err = true;
      pos = n;
      return;
    }
    pos += static_cast<size_t>(k);
  }
};

struct Wr {
  std::vector<uint8_t> b;
  void be(uint64_t v, int k) {
    for (int i = k - 1; i >= 0; --i) b.push_back(static_cast<uint8_t>(v >> (8 * i)));
  }
  void i8(int v) { be(static_cast<uint8_t>(v), 1); }
  void i16(int v) { be(static_cast<uint16_t>(v), 2); }
  void i32(int64_t v) { be(static_cast<uint32_t>(v), 4); }
  void i64(int64_t v) { be(static_cast<uint64_t>(v), 8); }
  void str(const std::string& s) {  // Encode(string): uint16 length + bytes
    i16(static_cast<int>(s.size()));
    b.insert(b.end(), s.begin(), s.end());
  }
};

constexpr int kErrTopicAuthorizationFailed = 29;  // vendor/.../proto/errors.go:37
// time.Time{}.UnixNano() / int64(time.Millisecond) on a 64-bit Go: the zero
// Time's nanoseconds overflow int64 and wrap (OffsetResp v>=1 TimeStamp).
constexpr int64_t kZeroTimeMillis = -6795364578871LL;

// Bytes readMessageSet (messages.go:357-483) consumes from its LimitReader:
// it can stop inside the set (a bad CRC, attributes 3), and the request's
// next partition is then read from there.  Only called for requests whose
// verdict is a deny, i.e. whose decode succeeded.
size_t message_set_consumed(const uint8_t* p, size_t avail, int32_t size, int16_t version) {
  const size_t lim = avail < static_cast<size_t>(size) ? avail : static_cast<size_t>(size);
  size_t pos = 0;
  for (;;) {
    if (lim - pos < 12) return lim;  // offset / size: short reads consume the rest
    pos += 8;
    const int32_t msz = static_cast<int32_t>(static_cast<uint32_t>(p[pos]) << 24 | static_cast<uint32_t>(p[pos + 1]) << 16 |
                                             static_cast<uint32_t>(p[pos + 2]) << 8 | p[pos + 3]);
    pos += 4;
    if (msz <= 0) return pos;
    if (lim - pos < static_cast<size_t>(msz)) return lim;
    const uint8_t* m = p + pos;
    pos += static_cast<size_t>(msz);
    if (msz <= 4) return pos;
    uint32_t c = 0xffffffffu;
    for (int32_t i = 4; i < msz; ++i) {
      c ^= m[i];
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    const uint32_t crc = static_cast<uint32_t>(m[0]) << 24 | static_cast<uint32_t>(m[1]) << 16 |
                         static_cast<uint32_t>(m[2]) << 8 | m[3];
    if ((c ^ 0xffffffffu) != crc) return pos;
    const size_t ap = 5;  // crc, magic
    if (msz > static_cast<int32_t>(ap) && (m[ap] & 3) == 3) return pos;
    (void)version;
  }
}

struct TopicParts {
  std::string name;
  size_t at = 0;  // offset of the name's bytes in the request
  std::vector<int32_t> parts;
};

// What GetTopics / CreateResponse need of a request whose decode succeeded
// (pkg/kafka/request.go:88-108,158-182 over optiopay's per-kind readers).
struct KReq {
  int16_t kind = 0, version = 0;
  int32_t corr = 0;
  std::vector<TopicParts> topics;
};

// L7M_OK, L7M_EINVAL (decode error), L7M_EUNSUPPORTED (request == nil: a kind
// ReadRequest leaves untyped, request.go:204-220).
int read_kafka(const uint8_t* req, size_t len, KReq* q) {
  Rd r{req, len};
  r.i32();  // size
  q->kind = r.i16();
  q->version = r.i16();
  q->corr = r.i32();
  if (r.err) return L7M_EINVAL;
  const int16_t version = q->version;
  auto partitions = [&](TopicParts& t, size_t fixed, bool produce, bool commit) {
    const int32_t np = r.arraylen();
    for (int32_t k = 0; k < np && !r.err; ++k) {
      t.parts.push_back(r.i32());
      if (produce) {
        const int32_t sz = r.i32();
        if (r.err) break;
        if (sz < 0 || sz > l7m::kKafkaMaxParseBuf) r.err = true;
        else r.pos += message_set_consumed(r.p + r.pos, r.n - r.pos, sz, version);
      } else if (commit) {
        r.skip(8 + (version == 1 ? 8 : 0));
        r.str();
      } else {
        r.skip(fixed);
      }
    }
  };
  auto read_topics = [&](size_t fixed, bool produce, bool commit, bool names_only) {
    const int32_t nt = r.arraylen();
    for (int32_t k = 0; k < nt && !r.err; ++k) {
      TopicParts t;
      t.name = r.str(&t.at);
      if (!names_only) partitions(t, fixed, produce, commit);
      q->topics.push_back(std::move(t));
    }
  };
  r.str();  // ClientID
  switch (q->kind) {
    case 0:  // ReadProduceReq
      if (version >= 3) r.str();
      r.skip(6);
      read_topics(0, true, false, false);
      break;
    case 1:  // ReadFetchReq
      r.skip(12 + (version >= 3 ? 4 : 0) + (version >= 4 ? 1 : 0));
      read_topics(12 + (version >= 5 ? 8 : 0), false, false, false);
      break;
    case 2:  // ReadOffsetReq
      r.skip(4 + (version >= 2 ? 1 : 0));
      read_topics(8 + (version == 0 ? 4 : 0), false, false, false);
      break;
    case 3:  // ReadMetadataReq
      read_topics(0, false, false, true);
      break;
    case 8:  // ReadOffsetCommitReq
      r.str();
      if (version >= 1) {
        r.skip(4);
        r.str();
      }
      if (version >= 2) r.skip(8);
      read_topics(0, false, true, false);
      break;
    case 9:  // ReadOffsetFetchReq
      r.str();
      read_topics(0, false, false, false);
      break;
    case 10:  // ReadConsumerMetadataReq
      r.str();
      if (version >= 1) r.skip(1);
      break;
    default:
      return L7M_EUNSUPPORTED;
  }
  return r.err ? L7M_EINVAL : L7M_OK;
}

// Protobuf wire writer (proto3: default-valued fields are omitted).
struct Pb {
  std::string b;
  void varint(uint64_t v) {
    while (v >= 0x80) {
      b.push_back(static_cast<char>(v | 0x80));
      v >>= 7;
    }
    b.push_back(static_cast<char>(v));
  }
  void key(uint32_t field, uint32_t wire) { varint(static_cast<uint64_t>(field) << 3 | wire); }
  void u64(uint32_t field, uint64_t v) {
    if (!v) return;
    key(field, 0);
    varint(v);
  }
  void bytes(uint32_t field, const char* p, size_t n) {
    if (!n) return;
    key(field, 2);
    varint(n);
    b.append(p, n);
  }
};

const char* const kApiKeyNames[] = {  // api.KafkaReverseAPIKeyMap (pkg/policy/api/kafka.go:193-227)
    "produce", "fetch", "offsets", "metadata", "leaderandisr", "stopreplica", "updatemetadata",
    "controlledshutdown", "offsetcommit", "offsetfetch", "findcoordinator", "joingroup", "heartbeat",
    "leavegroup", "syncgroup", "describegroups", "listgroups", "saslhandshake", "apiversions",
    "createtopics", "deletetopics", "deleterecords", "initproducerid", "offsetforleaderepoch",
    "addpartitionstotxn", "addoffsetstotxn", "endtxn", "writetxnmarkers", "txnoffsetcommit",
    "describeacls", "createacls", "deleteacls", "describeconfigs", "alterconfigs"};

// Kafka record at offs[i]: the size-prefixed request; false if it does not fit.
bool kafka_rec(const uint8_t* arena, size_t arena_bytes, uint64_t o, size_t* len) {
  if (o > arena_bytes || arena_bytes - o < 4) return false;
  const uint8_t* p = arena + o;
  const uint64_t sz = static_cast<uint64_t>(p[0]) << 24 | static_cast<uint64_t>(p[1]) << 16 |
                      static_cast<uint64_t>(p[2]) << 8 | p[3];
  if (sz > arena_bytes - o - 4) return false;
  *len = static_cast<size_t>(sz + 4);
  return true;
}

// The host's instantiation of l7m_http_log.h: the arena in host memory, an
// entry written where the caller's buffer has room for it.
struct HostSrc {
  const uint8_t* p;
  uint8_t at(uint64_t i) const { return p[i]; }
  uint32_t word(uint64_t i) const {
    uint32_t w;
    std::memcpy(&w, p + i, 4);
    return w;
  }
};
struct HostSink {
  uint8_t* p;
  void put(uint8_t b) { *p++ = b; }
};
struct HostConsts {  // fields 1-2, 4, 7-8 of every entry of a call
  std::string head, policy, addrs;
  size_t head_len = 0, policy_len = 0, addrs_len = 0;
  uint32_t local_identity = 0;
};

using l7m::flow_verdict;

}  // namespace

namespace l7m {

l7m_access_log_opts log_norm_opts(const l7m_access_log_opts* opts) {
  l7m_access_log_opts o{};
  o.http_protocol = 1;  // HTTP11: Envoy's default branch (accesslog.cc:68-79)
  if (opts) {
    const size_t k = opts->struct_size == 0 || opts->struct_size > sizeof o ? sizeof o : opts->struct_size;
    std::memcpy(&o, opts, k);
  }
  return o;
}

void log_const_fields(const l7m_access_log_opts& o, std::string* head, std::string* policy, std::string* addrs) {
  Pb pb;
  pb.u64(1, o.timestamp_ns);
  pb.u64(2, o.http_protocol);
  *head = pb.b;
  pb.b.clear();
  pb.bytes(4, o.policy_name, o.policy_name ? std::strlen(o.policy_name) : 0);
  *policy = pb.b;
  pb.b.clear();
  pb.bytes(7, o.source_address, o.source_address ? std::strlen(o.source_address) : 0);
  pb.bytes(8, o.destination_address, o.destination_address ? std::strlen(o.destination_address) : 0);
  *addrs = pb.b;
}

}  // namespace l7m

extern "C" {

size_t l7m_http_deny_body(const char* configured, char* out, size_t cap) {
  // cilium_l7policy.cc:89-95: empty -> "Access denied"; ensure a trailing CRLF
  std::string b = configured && *configured ? configured : "Access denied";
  const size_t len = b.size();
  if (len < 2 || b[len - 2] != '\r' || b[len - 1] != '\n') b += "\r\n";
  if (out && cap) {
    const size_t k = b.size() < cap - 1 ? b.size() : cap - 1;
    std::memcpy(out, b.data(), k);
    out[k] = 0;
  }
  return b.size();
}

int l7m_kafka_deny_response(const uint8_t* req, size_t len, uint8_t* out, size_t cap, size_t* out_len) {
  if (!req || !out_len) return L7M_EINVAL;
  KReq q;
  const int rc = read_kafka(req, len, &q);
  if (rc != L7M_OK) return rc;
  const int16_t version = q.version;
  const std::vector<TopicParts>& topics = q.topics;
  Wr w;
  w.i32(0);  // size placeholder
  w.i32(q.corr);
  switch (q.kind) {
    case 0:  // ProduceResp.Bytes (messages.go:1697)
      w.i32(static_cast<int64_t>(topics.size()));
      for (const auto& t : topics) {
        w.str(t.name);
        w.i32(static_cast<int64_t>(t.parts.size()));
        for (int32_t id : t.parts) {
          w.i32(id);
          w.i16(kErrTopicAuthorizationFailed);
          w.i64(0);                     // Offset
          if (version >= 2) w.i64(0);   // LogAppendTime
        }
      }
      if (version >= 1) w.i32(0);  // ThrottleTime
      break;
    case 1:  // FetchResp.Bytes (messages.go:896)
      if (version >= 1) w.i32(0);  // ThrottleTime
      w.i32(static_cast<int64_t>(topics.size()));
      for (const auto& t : topics) {
        w.str(t.name);
        w.i32(static_cast<int64_t>(t.parts.size()));
        for (int32_t id : t.parts) {
          w.i32(id);
          w.i16(kErrTopicAuthorizationFailed);
          w.i64(0);  // TipOffset
          if (version >= 4) {
            w.i64(0);                    // LastStableOffset
            if (version >= 5) w.i64(0);  // LogStartOffset
            w.i32(0);                    // AbortedTransactions
          }
          w.i32(0);  // message set size: no messages
        }
      }
      break;
    case 2:  // OffsetResp.Bytes (messages.go:1956)
      if (version >= 2) w.i32(0);  // ThrottleTime
      w.i32(static_cast<int64_t>(topics.size()));
      for (const auto& t : topics) {
        w.str(t.name);
        w.i32(static_cast<int64_t>(t.parts.size()));
        for (int32_t id : t.parts) {
          w.i32(id);
          w.i16(kErrTopicAuthorizationFailed);
          if (version >= 1) w.i64(kZeroTimeMillis);
          w.i32(0);  // Offsets
        }
      }
      break;
    case 3:  // MetadataResp.Bytes (messages.go:595)
      if (version >= 3) w.i32(0);  // ThrottleTime
      w.i32(0);                    // Brokers
      if (version >= 2) w.str("");  // ClusterID
      if (version >= 1) w.i32(0);   // ControllerID
      w.i32(static_cast<int64_t>(topics.size()));
      for (const auto& t : topics) {
        w.i16(kErrTopicAuthorizationFailed);
        w.str(t.name);
        if (version >= 1) w.i8(0);  // IsInternal
        w.i32(0);                   // Partitions
      }
      break;
    case 8:  // OffsetCommitResp.Bytes (messages.go:1327)
      if (version >= 3) w.i32(0);
      w.i32(static_cast<int64_t>(topics.size()));
      for (const auto& t : topics) {
        w.str(t.name);
        w.i32(static_cast<int64_t>(t.parts.size()));
        for (int32_t id : t.parts) {
          w.i32(id);
          w.i16(kErrTopicAuthorizationFailed);
        }
      }
      break;
    case 9:  // OffsetFetchResp.Bytes (messages.go:1512)
      if (version >= 3) w.i32(0);
      w.i32(static_cast<int64_t>(topics.size()));
      for (const auto& t : topics) {
        w.str(t.name);
        w.i32(static_cast<int64_t>(t.parts.size()));
        for (int32_t id : t.parts) {
          w.i32(id);
          w.i64(0);    // Offset
          w.str("");   // Metadata
          w.i16(kErrTopicAuthorizationFailed);
        }
      }
      if (version >= 2) w.i16(0);  // resp.Err: left nil by createOffsetFetchResponse
      break;
    case 10:  // ConsumerMetadataResp.Bytes (messages.go:1102)
      if (version >= 1) w.i32(0);  // ThrottleTime
      w.i16(kErrTopicAuthorizationFailed);
      if (version >= 1) w.str("");  // ErrMsg
      w.i32(0);                     // CoordinatorID
      w.str("");                    // CoordinatorHost
      w.i32(0);                     // CoordinatorPort
      break;
  }
  const uint32_t sz = static_cast<uint32_t>(w.b.size() - 4);
  w.b[0] = static_cast<uint8_t>(sz >> 24);
  w.b[1] = static_cast<uint8_t>(sz >> 16);
  w.b[2] = static_cast<uint8_t>(sz >> 8);
  w.b[3] = static_cast<uint8_t>(sz);
  *out_len = w.b.size();
  if (!out || cap < w.b.size()) return L7M_ENOMEM;
  std::memcpy(out, w.b.data(), w.b.size());
  return L7M_OK;
}

size_t l7m_kafka_api_key_name(int16_t key, char* out, size_t cap) {
  // apiKeyToString (pkg/proxy/kafka.go:161-166): the map's name, else the number
  const std::string s = key >= 0 && key < static_cast<int16_t>(sizeof kApiKeyNames / sizeof *kApiKeyNames)
                            ? kApiKeyNames[key]
                            : std::to_string(key);
  if (out && cap) {
    const size_t k = s.size() < cap - 1 ? s.size() : cap - 1;
    std::memcpy(out, s.data(), k);
    out[k] = 0;
  }
  return s.size();
}

int64_t l7m_http_access_log(const uint8_t* arena, size_t arena_bytes, const uint64_t* offs, size_t n,
                            const int32_t* verdicts, const l7m_access_log_opts* opts, uint8_t* out, size_t cap,
                            uint64_t* entry_offs) {
  if (n && (!arena || !offs || !verdicts || !entry_offs)) return L7M_EINVAL;
  const l7m_access_log_opts o = l7m::log_norm_opts(opts);
  HostConsts c;
  l7m::log_const_fields(o, &c.head, &c.policy, &c.addrs);
  c.head_len = c.head.size();
  c.policy_len = c.policy.size();
  c.addrs_len = c.addrs.size();
  c.local_identity = o.local_identity;
  const HostSrc src{arena};
  uint64_t total = 0;
  const bool write = out != nullptr;
  for (size_t i = 0; i < n; ++i) {
    entry_offs[i] = total;
    l7m::LogView v;
    if (!l7m::log_wanted(verdicts[i], L7M_LOG_FORWARDED | L7M_LOG_DENIED) ||
        !l7m::log_view(src, arena_bytes, offs[i], v))
      continue;
    const uint64_t size = l7m::log_measure(src, v, verdicts[i], c);
    if (write && total + size <= cap) {
      HostSink k{out + total};
      l7m::log_emit(src, v, verdicts[i], c, k);
    }
    total += size;
  }
  if (n) entry_offs[n] = total;
  return write && total > cap ? static_cast<int64_t>(L7M_ENOMEM) : static_cast<int64_t>(total);
}

int64_t l7m_kafka_access_log(const uint8_t* arena, size_t arena_bytes, const uint64_t* offs, size_t n,
                             const int32_t* verdicts, l7m_kafka_log_record* out, size_t cap) {
  if (n && (!arena || !offs || !verdicts)) return L7M_EINVAL;
  uint64_t k = 0;
  for (size_t i = 0; i < n; ++i) {
    const int32_t vd = verdicts[i];
    // ReadRequest failed: the connection is closed, nothing is logged
    // (pkg/proxy/kafka.go:349-354); -3 (a codec limit of this library) too.
    if (vd == L7M_VERDICT_PARSE_ERROR || vd == L7M_VERDICT_UNSUPPORTED) continue;
    size_t len;
    if (!kafka_rec(arena, arena_bytes, offs[i], &len)) continue;
    KReq q;
    const int rc = read_kafka(arena + offs[i], len, &q);
    if (rc != L7M_OK) continue;  // request == nil: GetTopics() is nil, no records
    // allowed: Forwarded / ErrNone; denied: CreateResponse succeeds for every
    // typed request -> Denied / ErrTopicAuthorizationFailed (kafka.go:240-262,296)
    const uint32_t fv = flow_verdict(vd);
    for (const auto& t : q.topics) {  // one record per topic (kafka.go:207-211)
      if (out && k < cap) {
        l7m_kafka_log_record& r = out[k];
        r.request = i;
        r.verdict = fv;
        r.error_code = fv == 1 ? kErrTopicAuthorizationFailed : 0;
        r.api_key = q.kind;
        r.api_version = q.version;
        r.correlation_id = q.corr;
        r.topic_off = offs[i] + t.at;
        r.topic_len = static_cast<uint32_t>(t.name.size());
        r.pad = 0;
      }
      ++k;
    }
  }
  return out && k > cap ? static_cast<int64_t>(L7M_ENOMEM) : static_cast<int64_t>(k);
}

}  // extern "C"

// Per-endpoint proxy statistics keyed as Endpoint.proxyStatistics
// (pkg/endpoint/endpoint.go:2060-2122): (protocol, port, ingress) -> request /
// response MessageForwardingStatistics.
struct l7m_proxy_stats_table {
  std::mutex mu;
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, l7m_proxy_stats> m;
};

namespace l7m {

void proxy_stats_merge_http(l7m_proxy_stats_table* t, const uint64_t* counters) {
  std::lock_guard<std::mutex> g(t->mu);
  for (uint32_t row = 0; row < kStatsRows; ++row) {
    const uint64_t* c = counters + static_cast<size_t>(row) * kStatsClasses;
    if (!(c[0] | c[1] | c[2])) continue;
    l7m_proxy_stats& s = t->m[std::make_tuple(static_cast<uint32_t>(L7M_PROTO_HTTP), row & 0xffffu, row >> 16, 1u)];
    s.received += c[0] + c[1] + c[2];
    s.forwarded += c[0];
    s.denied += c[1];
    s.error += c[2];
  }
}

}  // namespace l7m

extern "C" {

l7m_proxy_stats_table* l7m_proxy_stats_table_create(void) { return new (std::nothrow) l7m_proxy_stats_table(); }

void l7m_proxy_stats_table_destroy(l7m_proxy_stats_table* t) { delete t; }

int l7m_proxy_stats_update(l7m_proxy_stats_table* t, uint32_t proto, const uint8_t* arena, size_t arena_bytes,
                           const uint64_t* offs, const int32_t* verdicts, size_t n, uint16_t port, int ingress) {
  if (!t || (n && !verdicts) || (proto != L7M_PROTO_HTTP && proto != L7M_PROTO_KAFKA)) return L7M_EINVAL;
  if (n && (!arena || !offs)) return L7M_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  for (size_t i = 0; i < n; ++i) {
    const int32_t vd = verdicts[i];
    uint32_t p = port, ing = ingress ? 1u : 0u;
    if (proto == L7M_PROTO_HTTP) {
      // from the access-log entry: DestinationEndpoint.Port and the entry's
      // direction (pkg/envoy/accesslog_server.go:165-169)
      l7m::LogView v;
      if (!l7m::log_view(HostSrc{arena}, arena_bytes, offs[i], v)) {
        p = port;
      } else {
        p = v.dport;
        ing = (v.flags & L7M_HTTP_F_INGRESS) ? 1u : 0u;
      }
    } else {
      // the redirect's port and direction; port 0 is not counted, nor a
      // request ReadRequest rejected (the connection closes) (kafka.go:213-229,349-354)
      if (vd == L7M_VERDICT_PARSE_ERROR) continue;
    }
    uint32_t fv = flow_verdict(vd);
    if (proto == L7M_PROTO_KAFKA && vd == L7M_VERDICT_DENY) {
      // a denied request is answered with CreateResponse(ErrTopicAuthorizationFailed),
      // which fails for the kinds ReadRequest leaves untyped (request == nil,
      // request.go:174-175): the record is then logged as VerdictError
      // (kafka.go:246-252)
      size_t len = 0;
      KReq q;
      if (kafka_rec(arena, arena_bytes, offs[i], &len) && read_kafka(arena + offs[i], len, &q) == L7M_EUNSUPPORTED)
        fv = 2;
    }
    if (p == 0 && proto == L7M_PROTO_KAFKA) continue;
    l7m_proxy_stats& s = t->m[std::make_tuple(proto, p, ing, 1u)];
    s.received++;
    if (fv == 0) s.forwarded++;
    else if (fv == 1) s.denied++;
    else s.error++;
  }
  return L7M_OK;
}

size_t l7m_proxy_stats_get(l7m_proxy_stats_table* t, l7m_proxy_stats_entry* out, size_t cap) {
  if (!t) return 0;
  std::lock_guard<std::mutex> g(t->mu);
  size_t k = 0;
  for (const auto& e : t->m) {
    if (out && k < cap) {
      l7m_proxy_stats_entry& r = out[k];
      r.proto = std::get<0>(e.first);
      r.port = static_cast<uint16_t>(std::get<1>(e.first));
      r.ingress = static_cast<uint8_t>(std::get<2>(e.first));
      r.request = static_cast<uint8_t>(std::get<3>(e.first));
      r.stats = e.second;
    }
    ++k;
  }
  return k;
}

int l7m_proxy_stats_add(const int32_t* verdicts, size_t n, l7m_proxy_stats* st) {
  if ((n && !verdicts) || !st) return L7M_EINVAL;
  for (size_t i = 0; i < n; ++i) {
    const int32_t v = verdicts[i];
    st->received++;
    if (v >= 0) st->forwarded++;                 // VerdictForwarded
    else if (v == L7M_VERDICT_DENY) st->denied++;  // VerdictDenied
    else st->error++;                            // VerdictError: ReadRequest failed
  }
  return L7M_OK;
}

}  // extern "C"
