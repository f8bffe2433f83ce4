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
#include "l7m_kafka_side.h"
#include "program.h"

namespace {

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

// The host's instantiation of l7m_kafka_side.h: a request is walked once for
// what it takes (the response's size, the number of topics) and, when that
// succeeded and the caller's buffer has room, once more for the output.
// L7M_OK, L7M_EINVAL or L7M_EUNSUPPORTED as kafka_walk answers.
int kafka_resp_size(const HostSrc& src, uint64_t off, uint64_t len, uint64_t* size) {
  l7m::KafkaHead h;
  l7m::KafkaRespSize m;
  const int rc = l7m::kafka_walk(src, off, len, l7m::KafkaCrcBitwise{}, h, m);
  *size = m.bytes;
  return rc;
}
void kafka_resp_emit(const HostSrc& src, uint64_t off, uint64_t len, uint64_t size, uint8_t* out) {
  l7m::KafkaHead h;
  l7m::KafkaRespEmit<HostSrc, HostSink> e(src, HostSink{out}, size);
  l7m::kafka_walk(src, off, len, l7m::KafkaCrcBitwise{}, h, e);
}
// The log records of request `request` into out[k, cap), counting in k.
struct HostLogEmit {
  l7m_kafka_log_record* out;
  size_t cap;
  uint64_t k, request;
  int32_t verdict;
  void topics(const l7m::KafkaHead&, int32_t) {}
  void topic(const l7m::KafkaHead& h, uint64_t at, uint32_t nl, int32_t) {
    if (k < cap) l7m::kafka_log_fill(out[k], request, verdict, h, at, nl);
    ++k;
  }
  void partition(const l7m::KafkaHead&, int32_t) {}
  void end(const l7m::KafkaHead&) {}
};

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
  const HostSrc src{req};
  uint64_t size = 0;
  const int rc = kafka_resp_size(src, 0, len, &size);
  if (rc != L7M_OK) return rc;
  *out_len = static_cast<size_t>(size);
  if (!out || cap < size) return L7M_ENOMEM;
  kafka_resp_emit(src, 0, len, size, out);
  return L7M_OK;
}

int64_t l7m_kafka_deny_responses(const uint8_t* arena, size_t arena_bytes, const uint64_t* offs, size_t n,
                                 const int32_t* verdicts, uint8_t* out, size_t cap, uint64_t* resp_offs) {
  if (n && (!arena || !offs || !verdicts || !resp_offs)) return L7M_EINVAL;
  const HostSrc src{arena};
  uint64_t total = 0;
  const bool write = out != nullptr;
  for (size_t i = 0; i < n; ++i) {
    resp_offs[i] = total;
    uint64_t len = 0, size = 0;
    if (verdicts[i] != L7M_VERDICT_DENY || !l7m::kafka_rec(src, arena_bytes, offs[i], &len) ||
        kafka_resp_size(src, offs[i], len, &size) != L7M_OK)
      continue;
    if (write && total + size <= cap) kafka_resp_emit(src, offs[i], len, size, out + total);
    total += size;
  }
  if (n) resp_offs[n] = total;
  return write && total > cap ? static_cast<int64_t>(L7M_ENOMEM) : static_cast<int64_t>(total);
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
  const HostSrc src{arena};
  uint64_t k = 0;
  for (size_t i = 0; i < n; ++i) {
    const int32_t vd = verdicts[i];
    // ReadRequest failed: the connection is closed, nothing is logged
    // (pkg/proxy/kafka.go:349-354); -3 (a codec limit of this library) too.
    if (!l7m::kafka_log_wanted(vd, 0)) continue;
    uint64_t len = 0;
    if (!l7m::kafka_rec(src, arena_bytes, offs[i], &len)) continue;
    l7m::KafkaHead h;
    l7m::KafkaTopicCount c;
    // request == nil: GetTopics() is nil, no records
    if (l7m::kafka_walk(src, offs[i], len, l7m::KafkaCrcBitwise{}, h, c) != L7M_OK) continue;
    if (out && k < cap) {  // one record per topic (kafka.go:207-211)
      HostLogEmit e{out, cap, k, i, vd};
      l7m::kafka_walk(src, offs[i], len, l7m::KafkaCrcBitwise{}, h, e);
    }
    k += c.topics_seen;
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
      uint64_t len = 0;
      l7m::KafkaHead h;
      l7m::KafkaTopicCount c;
      const HostSrc src{arena};
      if (l7m::kafka_rec(src, arena_bytes, offs[i], &len) &&
          l7m::kafka_walk(src, offs[i], len, l7m::KafkaCrcBitwise{}, h, c) == L7M_EUNSUPPORTED)
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
