/*
 * l7match.h — C ABI of libl7match.so, the MI355X-native batched L7 policy
 * evaluator for Cilium's L7 rule model (PortRuleHTTP / PortRuleKafka).
 *
 * This is the drop-in boundary.  Each entry point replaces one reference
 * interface (all paths relative to the uniberg/cilium tree):
 *
 *   l7m_compile_http   replaces the rule-import half of the HTTP path:
 *                      getHTTPRule  pkg/envoy/server.go:261-320  (PortRuleHTTP ->
 *                      HeaderMatcher list) followed by the std::regex construction
 *                      in Envoy's HeaderData (envoy/cilium_network_policy.h:52-66,
 *                      policy instantiation envoy/cilium_network_policy.cc:63-65).
 *                      A regex that std::regex rejects makes the call fail
 *                      (L7M_EINVAL_REGEX) exactly where Envoy would NACK the
 *                      policy; the caller keeps its previous handle.
 *   l7m_compile_kafka  replaces PortRuleKafka.Sanitize
 *                      (pkg/policy/api/rule_validation.go:190-233) applied to the
 *                      rule slice handed to MatchesRule (pkg/kafka/policy.go:200).
 *   l7m_compile_http_policies
 *                      the rule import of whole NPDS NetworkPolicy resources
 *                      (envoy/cilium/npds.proto:32-118) into Envoy's
 *                      NetworkPolicyMap (envoy/cilium_network_policy.cc:42-108,
 *                      PolicyInstance / PortNetworkPolicy construction
 *                      envoy/cilium_network_policy.h:40-208): per endpoint policy
 *                      name, ingress and egress per-port rule sets.
 *   l7m_eval           replaces, for a batch of N requests,
 *                        HTTP : NetworkPolicyMap::Allowed
 *                               envoy/cilium_network_policy.h:223-237 (-> :198-203,
 *                               :169-192, :128-146, :90-108, :68-71)
 *                        Kafka: kafka.ReadRequest pkg/kafka/request.go:186-229 +
 *                               (*RequestMessage).MatchesRule pkg/kafka/policy.go:200-225
 *                      The reference returns a bare bool per request; this ABI
 *                      returns an int32 verdict per request (see L7M_VERDICT_*):
 *                      -1 deny, i >= 0 allow decided by rule i (input order).
 *   l7m_eval_device    the same on buffers already resident in HBM, enqueued on a
 *                      caller-provided HIP stream (no host synchronisation).
 *
 * Conventions: every int-returning function returns L7M_OK (0) or a negative
 * L7M_E* code.  When err != NULL and errlen > 0 a NUL-terminated message is
 * written on failure.  Handles are immutable after compile and reference
 * counted; l7m_eval / l7m_eval_device are reentrant and may be called
 * concurrently from many threads on the same handle (each call uses its own
 * stream and scratch), mirroring Envoy's lock-free per-worker read path.
 *
 * Nothing in this header depends on HIP or torch types: streams are passed
 * as void* (hipStream_t), device buffers as void*.
 */
#ifndef L7MATCH_H
#define L7MATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L7M_ABI_VERSION 4

/* ---- status codes ------------------------------------------------------ */
#define L7M_OK 0
#define L7M_EINVAL (-1)         /* bad argument (NULL pointer, bad size)          */
#define L7M_EINVAL_REGEX (-2)   /* std::regex would throw: Envoy NACKs the policy */
#define L7M_EINVAL_RULE (-3)    /* Sanitize() error / getHTTPRule sort panic      */
#define L7M_EUNSUPPORTED (-4)   /* valid regex outside the compiled subset        */
#define L7M_ENOMEM (-5)         /* host or device allocation failed               */
#define L7M_EDEVICE (-6)        /* HIP runtime error / no device                  */
#define L7M_ETOOBIG (-7)        /* rule set exceeds a compile-time limit          */

/* ---- verdicts (int32 per request) --------------------------------------- */
#define L7M_VERDICT_DENY (-1)         /* no rule allows the request               */
#define L7M_VERDICT_PARSE_ERROR (-2)  /* Kafka: ReadRequest would return an error  */
#define L7M_VERDICT_UNSUPPORTED (-3)  /* Kafka: a gzip/snappy message set past the second
                                        pass's limits (nesting depth 8, slab, queue).
                                        HTTP: a rule with a back-reference / look-around
                                        matcher (slow path, regex_vm.h) ran past the
                                        executor's second-tier limits before any
                                        earlier rule decided the request: more than
                                        1 MiB of backtracking stack (262144 words),
                                        which std::regex_match's recursion turns into
                                        more than 8 MiB of native stack (>= 8 native
                                        bytes per executor byte, measured >= 12 on
                                        every family in tests/test_slow_tiers_cpu.py):
                                        it overflows an Envoy worker's default thread
                                        stack there; or more than 2^25 backtracking
                                        steps (exponential patterns the reference
                                        spends seconds on)                          */
#define L7M_VERDICT_ALLOW_NO_L7 (0x7fffffff) /* HTTP rule list empty: port has no L7
                                        rules, Envoy allows (cilium_network_policy.h:129-135) */
#define L7M_VERDICT_ALLOW_NO_PORT_POLICY (0x7ffffffe) /* no per-port policy for the
                                        request's port, not even port 0: Envoy allows
                                        (cilium_network_policy.h:187-191) */

/* ---- dialects ------------------------------------------------------------ */
#define L7M_DIALECT_ENVOY_ECMA_FULL 0 /* std::regex ECMAScript, regex_match (full)  */
#define L7M_DIALECT_RE2_SEARCH 1      /* Go regexp MatchString: RE2, unanchored     */

#define L7M_PROTO_HTTP 1
#define L7M_PROTO_KAFKA 2

typedef struct l7m_ruleset l7m_ruleset; /* opaque */

/* Verbatim api.PortRuleHTTP (pkg/policy/api/http.go:26-58).  NULL or "" = unset.
 * remote_ids: allowed_remotes_ of the PortNetworkPolicyRule this HTTP rule
 * belongs to (envoy/cilium_network_policy.h:90-97, NPDS remote_policies);
 * n_remote_ids == 0 means any remote identity.  A request is allowed by rule i
 * iff its remote_id is in the set AND every matcher of the rule holds. */
typedef struct {
  const char* path;
  const char* method;
  const char* host;
  const char* const* headers; /* "Name: value" (literal) or "Name" (presence) */
  uint32_t n_headers;
  uint32_t n_remote_ids;
  const uint32_t* remote_ids;
} l7m_http_rule;

/* ---- NPDS network policies (the full NetworkPolicyMap::Allowed boundary) --
 * PortNetworkPolicyRule (npds.proto:78-95; cilium_network_policy.h:76-112):
 * remote identities (empty = any) and, when has_http_rules != 0, the OR of its
 * HTTP rules (each an AND of getHTTPRule matchers; the rules' own remote_ids
 * must be empty).  has_http_rules == 0 = no L7 predicate: any request from an
 * allowed remote matches.  has_http_rules with n_http_rules == 0 violates
 * HttpNetworkPolicyRules.http_rules min_items = 1 (L7M_EINVAL_RULE). */
typedef struct {
  const uint32_t* remote_ids;
  uint32_t n_remote_ids;
  uint32_t has_http_rules;
  const l7m_http_rule* http_rules;
  size_t n_http_rules;
} l7m_port_rule;

#define L7M_L4_TCP 0 /* envoy SocketAddress.Protocol: only TCP policies are installed */
#define L7M_L4_UDP 1

/* PortNetworkPolicy (npds.proto:58-76): port 0 = every port.  A port may
 * appear once per direction (else L7M_EINVAL_RULE, Envoy's "Duplicate port
 * number"); non-TCP entries are skipped as Envoy does
 * (cilium_network_policy.h:154-166). */
typedef struct {
  uint32_t port;
  uint32_t protocol; /* L7M_L4_* */
  const l7m_port_rule* rules;
  size_t n_rules;
} l7m_port_policy;

/* NetworkPolicy (npds.proto:32-56) of one endpoint, keyed by name. */
typedef struct {
  const char* name;
  const l7m_port_policy* ingress;
  size_t n_ingress;
  const l7m_port_policy* egress;
  size_t n_egress;
} l7m_network_policy;

/* Where a verdict's rule index comes from (l7m_ruleset_rule_origin).  The
 * index space of l7m_compile_http_policies is the policies' HTTP rules
 * flattened in this order: policies as given; ingress, then egress; port
 * entries as given except that the port-0 entry of a direction comes last
 * (so the smallest matching index is the exact-port match Envoy checks first,
 * cilium_network_policy.h:169-186); port rules as given; a port rule with
 * has_http_rules == 0 contributes one matcher-less pseudo rule
 * (http_rule = -1), else one index per HTTP rule. */
typedef struct {
  uint32_t policy;    /* index into the compiled policies               */
  uint32_t ingress;   /* 1 ingress, 0 egress                            */
  uint32_t port;      /* PortNetworkPolicy.port (0 = wildcard)          */
  uint32_t port_rule; /* index into that PortNetworkPolicy's rules      */
  int32_t http_rule;  /* index into the port rule's http_rules, or -1   */
  uint32_t reserved;
} l7m_rule_origin;

/* Verbatim api.PortRuleKafka (pkg/policy/api/kafka.go:26-106).  NULL or "" = unset. */
typedef struct {
  const char* role;
  const char* api_key;
  const char* api_version;
  const char* client_id;
  const char* topic;
} l7m_kafka_rule;

/* The Kafka redirect's L7DataMap (pkg/policy/l4.go:110-129 GetRelevantRules):
 * one entry per endpoint selector with that selector's PortRuleKafka rules.
 * `wildcard` marks api.WildcardEndpointSelector, whose rules apply to every
 * source; the others apply to the source identities whose labels the
 * selector matches, listed per identity in an l7m_identity_selectors
 * table; the control plane evaluates selector.Matches(labels).  At most 64
 * entries. */
typedef struct {
  const l7m_kafka_rule* rules;
  size_t n_rules;
  uint32_t wildcard;
  uint32_t reserved;
} l7m_kafka_selector_rules;

typedef struct {
  uint32_t identity;          /* numeric security identity (!= 0)                 */
  uint32_t reserved;
  const uint32_t* selectors;  /* indices of the L7DataMap entries that select it  */
  size_t n_selectors;
} l7m_identity_selectors;

typedef struct {
  uint32_t struct_size;     /* sizeof(l7m_opts); 0 = use defaults               */
  uint32_t dialect;         /* L7M_DIALECT_*                                    */
  uint32_t max_dfa_states;  /* per DFA group before splitting (0 = default)     */
  uint32_t flags;           /* L7M_OPT_* bits (below); 0 = defaults             */
  uint64_t max_table_bytes; /* per DFA group before splitting (0 = default)     */
  uint32_t lds_budget_bytes;/* DFA slot tables kept in LDS per workgroup
                               (0 = default 64 KiB); the rest is walked from HBM */
  uint32_t reserved;
} l7m_opts;

/* l7m_opts.flags (HTTP, ECMAScript dialect; ignored elsewhere).  An automaton
 * too large for LDS is walked from device memory in its packed double-array
 * form, one slot per explicit transition spread over up to 2^24 slots.  The
 * dense kind stores the same automaton as one 16-bit target per (state, byte
 * class): smaller when the states have many transitions (`.*`, look-ahead,
 * \b products: 50 MB -> 4 MB for a 50 k-state :path automaton), larger for
 * prefix tries.  Automata of more than 65,535 states, automata walked from
 * LDS, the header-name automaton and RE2-dialect programs keep the packed
 * form.  Verdicts and counters do not depend on the flags.  The environment
 * variable L7M_DENSE_DFA=1 / =2, read at each compile, ORs the same bits in. */
#define L7M_OPT_DENSE_DFA 1u        /* dense form where its table is the smaller one */
#define L7M_OPT_DENSE_DFA_ALWAYS 2u /* dense form wherever it can be built (tests)   */

typedef struct {
  uint32_t proto;           /* L7M_PROTO_*                                       */
  uint32_t n_rules;
  uint32_t n_fields;        /* HTTP: distinct header fields referenced          */
  uint32_t n_dfas;          /* HTTP: DFA groups (incl. the header-name DFA)     */
  uint64_t total_dfa_states;
  uint64_t program_bytes;   /* size of the device program blob                  */
  uint32_t n_counters;      /* length of rule_hits arrays = n_rules + 2         */
  uint32_t n_dense_dfas;    /* HTTP: DFA groups in the dense form (L7M_OPT_DENSE_DFA) */
} l7m_ruleset_info;

/* ---- rule compilation (cold path) ---------------------------------------- */
int l7m_compile_http(const l7m_http_rule* rules, size_t n, const l7m_opts* opts,
                     l7m_ruleset** out, char* err, size_t errlen);
int l7m_compile_kafka(const l7m_kafka_rule* rules, size_t n, const l7m_opts* opts,
                      l7m_ruleset** out, char* err, size_t errlen);
/* canAccess with GetRelevantRules (pkg/proxy/kafka.go:116-152): a request
 * from source identity s is decided by MatchesRule over the rules of the
 * entries that select s (none when s == 0 or s is not listed: the reference's
 * nil identity) followed by the wildcard entries' rules; no such rule ->
 * deny.  Verdict indices number the rules entry by entry in `map` order.
 * The source identities travel beside the arena (l7m_eval_ids);
 * l7m_compile_kafka(rules, n) is the map of one wildcard entry. */
int l7m_compile_kafka_map(const l7m_kafka_selector_rules* map, size_t n_entries,
                          const l7m_identity_selectors* identities, size_t n_identities,
                          const l7m_opts* opts, l7m_ruleset** out, char* err, size_t errlen);
/* A NetworkPolicyMap of n endpoint policies.  A request names its policy by
 * index in the record (l7m_ruleset_policy_index; 0xffff = a name the map does
 * not hold -> deny, cilium_network_policy.h:231-235); its direction and dport
 * select the per-port rule sets (exact port, then port 0, then allow).
 * l7m_compile_http(rules, n) is the one-policy map whose every port and
 * direction use `rules`. */
int l7m_compile_http_policies(const l7m_network_policy* policies, size_t n, const l7m_opts* opts,
                              l7m_ruleset** out, char* err, size_t errlen);
/* Index of an endpoint policy name in the record's policy field, or -1. */
int l7m_ruleset_policy_index(const l7m_ruleset* rs, const char* name);
/* Origin of verdict index `rule` (L7M_EINVAL if out of range). */
int l7m_ruleset_rule_origin(const l7m_ruleset* rs, uint32_t rule, l7m_rule_origin* out);
void l7m_retain(l7m_ruleset* rs);
void l7m_release(l7m_ruleset* rs);
int l7m_ruleset_get_info(const l7m_ruleset* rs, l7m_ruleset_info* out);
/* 1 if the HTTP rule set's first pass runs the lean kernel (a single-entry
 * program without slow-path rules, forced captures, literal tables or dense
 * automata whose <= 4 value automata are walked from LDS), else 0.  Decided
 * when the rule set is compiled; L7M_HTTP_GENERIC=1 in the environment at
 * that time keeps every rule set on the generic kernels. */
int l7m_ruleset_http_lean(const l7m_ruleset* rs);
/* Copy of the packed device program (for inspection / tests).  *len receives
 * the size; when buf is NULL only the size is returned. */
int l7m_ruleset_program(const l7m_ruleset* rs, void* buf, size_t* len);

/* getHTTPRule translation of one rule (pkg/envoy/server.go:261-320), sorted as
 * SortHeaderMatchers (pkg/envoy/sort.go:205-250).  Writes up to cap matchers;
 * returns the number of matchers (>= 0) or a negative status.  kind: 0 regex,
 * 1 literal value, 2 presence (Envoy HeaderMatchType Regex/Value/Present). Name
 * and value pointers stay valid until the next call on the same thread. */
typedef struct {
  const char* name;  /* as in the NPDS HeaderMatcher (not lower-cased)           */
  const char* value;
  uint32_t kind;
  uint32_t has_regex_flag; /* HeaderMatcher.Regex != nil                        */
} l7m_header_matcher;
int l7m_http_translate(const l7m_http_rule* rule, l7m_header_matcher* out, size_t cap,
                       char* err, size_t errlen);

/* ---- request arena --------------------------------------------------------
 * A batch is a byte arena holding N records plus an array of N uint64 byte
 * offsets (each record 4-byte aligned).
 *
 * HTTP record (little endian), L7M_HTTP_REC_FIXED bytes of fixed header:
 *   u32 rec_len        bytes of this record, unpadded (>= 20 + 4*n_hdr)
 *   u32 remote_id      source security identity (Envoy remote_id)
 *   u16 dport          destination port
 *   u8  flags          L7M_HTTP_F_*
 *   u8  n_hdr          number of regular headers
 *   u16 method_len, u16 path_len, u16 authority_len, u16 policy
 *                      policy: endpoint policy index (l7m_ruleset_policy_index),
 *                      0xffff = unknown endpoint policy (deny)
 *   n_hdr x { u16 name_len, u16 value_len }           header directory
 *   method | path | authority | name0 | value0 | name1 | value1 | ...
 * Header names must already be lower case (Envoy's codec lower-cases them);
 * the first occurrence of a name is the one matched (HeaderMap::get).
 *
 * Kafka record: the request exactly as proto.ReadReq returns it
 * (vendor/github.com/optiopay/kafka/proto/messages.go:124-165): big-endian
 * int32 size followed by size bytes; record length = 4 + size.
 */
#define L7M_HTTP_REC_FIXED 20
#define L7M_HTTP_F_METHOD 0x01
#define L7M_HTTP_F_PATH 0x02
#define L7M_HTTP_F_AUTHORITY 0x04
#define L7M_HTTP_F_INGRESS 0x08

typedef struct {
  const char* method;    /* NULL = absent */
  const char* path;      /* NULL = absent */
  const char* authority; /* NULL = absent */
  const char* const* header_names;  /* lower-cased by the packer */
  const char* const* header_values;
  uint32_t n_headers;
  uint32_t remote_id;
  uint16_t dport;
  uint16_t ingress;
  uint32_t policy;  /* endpoint policy index (0 for l7m_compile_http rule sets) */
} l7m_http_request;
#define L7M_POLICY_UNKNOWN 0xffffu

/* Bytes one request occupies in the arena (4-byte padded); 0 if not encodable. */
size_t l7m_http_record_size(const l7m_http_request* req);
/* Pack n requests; writes offsets[i]; returns bytes used or 0 on overflow. */
size_t l7m_pack_http(const l7m_http_request* reqs, size_t n, uint8_t* arena, size_t cap,
                     uint64_t* offsets);

/* ---- HTTP/1.x request heads as received (DESIGN.md "HTTP/1.x wire decode") --
 * The HTTP twin of the Kafka wire path: the caller holds request heads as
 * bytes off a socket or out of a capture, back to back in `wire`; head i is
 * wire[head_offs[i], head_offs[i+1]) (n + 1 ascending offsets, the last
 * <= wire_bytes).  Decoding turns them into the request arena above.
 *
 * Grammar (strict RFC 7230): `method SP target SP HTTP/1.0|HTTP/1.1 CRLF`,
 * then `name ":" OWS value OWS CRLF` lines, then an empty line; bytes of the
 * slice after it are ignored.  method and name are 1+ tchar (names are lower-
 * cased in the record); target is 1+ bytes above 0x20 other than 0x7f, copied
 * verbatim into :path; a value holds any byte but CR, LF and NUL, OWS (SP /
 * HTAB) stripped at both ends.  The first `host` header becomes :authority and
 * is not a regular header; the other headers keep wire order.
 *
 * status[i] >= 0: bytes of the head consumed, the empty line included.
 * status[i] < 0: an L7M_WIRE_E* code; the head still gets a record, of
 * L7M_HTTP_REC_FIXED bytes: remote_id, dport, the ingress flag and policy
 * from its metadata, everything else zero (rec_len too), which l7m_eval
 * answers with L7M_VERDICT_PARSE_ERROR.  The first offending byte from the
 * left decides the code. */
#define L7M_WIRE_EINCOMPLETE (-1) /* the slice ends before the empty line                     */
#define L7M_WIRE_EBADLINE (-2)    /* request line: bad method / target / version / line end   */
#define L7M_WIRE_EBADHEADER (-3)  /* header line: bad name, obs-fold, bare LF, CR without LF,
                                     NUL in a value                                           */
#define L7M_WIRE_EDUPHOST (-4)    /* a second host header                                     */
#define L7M_WIRE_ETOOMANY (-5)    /* more than 255 regular headers                            */
#define L7M_WIRE_ETOOLONG (-6)    /* a method, target, name or value above 65535 bytes (or a
                                     head above 2^31 - 1)                                     */

typedef struct {
  uint32_t remote_id;
  uint16_t dport;
  uint16_t policy;
  uint8_t ingress;
  uint8_t reserved[3];
} l7m_http_wire_meta; /* 12 bytes */

/* Arena capacity that is enough for any n heads in wire_bytes bytes:
 *   20 * n + max(0, wire_bytes + wire_bytes / 4 - 15)       (0 when n == 0).
 * Derivation: a refused head costs 20 bytes.  An accepted head of W bytes
 * with h regular headers spends 14 wire bytes the record does not hold (two
 * SP, the 8-byte version, two CRLF) against the record's 20 fixed bytes, and
 * a header line spends at least `":" CRLF` (3 bytes) where the record spends
 * a 4-byte directory entry; OWS and a host line only make the record smaller.
 * So its record is at most W + 6 + h bytes, W + 9 + h padded, and since a
 * line has a name, h <= (W - 16) / 4: at most W + W / 4 + 5, that is
 * 20 + (W + W / 4 - 15).  g(W) = max(0, W + W / 4 - 15) is superadditive, so
 * the sum over the heads is at most g(wire_bytes).  The bound is met by one
 * head `G / HTTP/1.1 CRLF a: CRLF a: CRLF a: CRLF CRLF` (28 bytes -> 40)
 * beside n - 1 empty slices.  A device arena additionally needs the
 * evaluator's readable slack: allocate round_up(bound, 16). */
size_t l7m_http_wire_arena_bound(size_t wire_bytes, size_t n);
/* Host decoder (no device needed), and the definition the device decoder
 * reproduces byte for byte.  meta: one entry per head, or NULL for zeros with
 * the ingress flag set.  Writes rec_offsets[n], status[n] and *arena_bytes,
 * the bytes the records need; pad bytes are zero.  L7M_ENOMEM when that is
 * more than cap (*arena_bytes, rec_offsets and status are still complete; the
 * arena then holds only the records that fit entirely); L7M_EINVAL for
 * offsets that do not ascend or pass wire_bytes. */
int l7m_http_wire_decode(const uint8_t* wire, size_t wire_bytes, const uint64_t* head_offs /* n+1 */,
                         size_t n, const l7m_http_wire_meta* meta /* NULL: zeros, ingress */,
                         uint8_t* arena, size_t cap, uint64_t* rec_offsets, int32_t* status,
                         size_t* arena_bytes);
/* The same on device buffers, enqueued on hip_stream (NULL = default stream)
 * without synchronising: a measure pass, a scan and an emit pass.  d_arena
 * must be 16-byte aligned; the output is what l7m_eval_device takes on the
 * same stream (d_arena readable up to round_up(total, 16)).  *d_arena_bytes
 * (u64) receives the total; when it exceeds cap no byte of d_arena is written
 * while offsets, status and the total are still produced.  Offsets that do not
 * ascend decode to unspecified records, without reading outside d_wire. */
int l7m_http_wire_decode_device(const void* d_wire, size_t wire_bytes, const void* d_head_offs, size_t n,
                                const void* d_meta, void* d_arena, size_t cap, void* d_rec_offsets,
                                void* d_status, void* d_arena_bytes /* u64 */, void* hip_stream);
/* The inverse (host only): `method SP path SP HTTP/1.1 CRLF`, `host:
 * <authority>` when the record has one, the regular headers as `name: value`,
 * the empty line.  status[i] = the head's size, or a negative code and an
 * empty head for a record the grammar cannot carry (L7M_WIRE_EBADLINE: method
 * or path; L7M_WIRE_EBADHEADER: a name, a value with OWS at an end or CR / LF /
 * NUL, a record that does not parse or lacks method or path;
 * L7M_WIRE_EDUPHOST: a regular header named host).  Returns the wire bytes
 * (wire == NULL: the size needed; L7M_ENOMEM when cap is too small). */
int64_t l7m_http_wire_encode(const uint8_t* arena, size_t arena_bytes, const uint64_t* rec_offsets, size_t n,
                             uint8_t* wire, size_t cap, uint64_t* head_offs /* n+1 */, int32_t* status);

/* ---- connection byte streams (DESIGN.md "Stream framing") -----------------
 * What a proxy or a capture holds is connections, not heads or records:
 * connection c is wire[conn_offs[c], conn_offs[c+1]) (n_conns + 1 ascending
 * offsets, the last <= wire_bytes).  Framing finds the requests inside each
 * connection, sequentially within it and independently across connections,
 * and writes the arrays the decoder (HTTP) or the evaluator (Kafka) takes.
 *
 * conn_status[c] is one of the codes below; conn_consumed[c] is the number of
 * the connection's bytes up to the end of its last complete request (head and
 * whole body, or frame; after L7M_STREAM_TUNNEL the CONNECT head included).
 * Carrying the unconsumed tail over to a later call is the caller's job.
 *
 * HTTP: every attempt to read a head at a position yields one slice that
 * starts there, so the slices of a connection tile its bytes and
 * head_offs[0 .. n_heads] (head_offs[n_heads] = conn_offs[n_conns]) is what
 * l7m_http_wire_decode(_device) takes unchanged.  A refused or partial last
 * head is a slice too: it decodes to the L7M_WIRE_E* code that ended the
 * connection.  How to read conn_status for the LAST slice of a connection:
 *   EAMBIGUOUS / EBADTE / EBADLENGTH  the head is complete and is evaluated,
 *       but a proxy would have answered 400 instead: discard its verdict;
 *   EBADCHUNK / EPARTIAL_BODY  the head was complete and its verdict stands;
 *   EBADHEAD / EPARTIAL_HEAD   the slice decodes to a negative wire status.
 * Kafka: a frame is the 4-byte big-endian size and `size` bytes; a bad size
 * or a cut frame ends the connection and emits nothing (the reference's
 * handler is never called for it).  A well-framed request that the evaluator
 * answers with L7M_VERDICT_PARSE_ERROR also closes its connection in the
 * reference; the framer does not look inside frames: rec_conn lets a caller
 * drop a connection's records after its first such verdict. */
#define L7M_STREAM_OK 0              /* the connection ends where a request ends (or is empty) */
#define L7M_STREAM_TUNNEL 1          /* HTTP: a CONNECT head; the rest is opaque               */
#define L7M_STREAM_EBADHEAD (-1)     /* HTTP: the decoder refuses the head (status < -1)       */
#define L7M_STREAM_EPARTIAL_HEAD (-2)  /* HTTP: the bytes end inside a head                    */
#define L7M_STREAM_EAMBIGUOUS (-3)   /* HTTP: transfer-encoding together with content-length   */
#define L7M_STREAM_EBADTE (-4)       /* HTTP: transfer-encoding is not one line `chunked`      */
#define L7M_STREAM_EBADLENGTH (-5)   /* HTTP: content-length is not one line of 1-18 digits    */
#define L7M_STREAM_EBADCHUNK (-6)    /* HTTP: chunk size, extension, line end or trailer       */
#define L7M_STREAM_EPARTIAL_BODY (-7)  /* HTTP: the bytes end inside a body                    */
#define L7M_STREAM_EPARTIAL_FRAME (-8) /* Kafka: the bytes end inside a size field or a frame  */
#define L7M_STREAM_EBADSIZE (-9)     /* Kafka: size < 8 or size + 4 > 6553500                  */

/* Heads that any n_conns connections in wire_bytes bytes can yield:
 * wire_bytes / 16 + n_conns.  A slice that is followed by another one in its
 * connection holds a complete head, and a complete head is at least 16 bytes
 * (`G / HTTP/1.1 CRLF CRLF`); each connection adds at most one last slice. */
size_t l7m_http_stream_heads_bound(size_t wire_bytes, size_t n_conns);
/* Host framer (no device needed), and the definition the device framer
 * reproduces byte for byte.  head_conn[i] is the connection of head i and
 * head_meta[i] = conn_meta[head_conn[i]] (what lookupNewDest gives once per
 * connection; head_meta NULL: not written; conn_meta NULL: zeros, ingress).
 * conn_status, conn_consumed and *n_heads are always complete.  When
 * *n_heads > cap_heads the per-head arrays are untouched and the call returns
 * L7M_ENOMEM (cap_heads == 0 with NULL arrays is the sizing call); otherwise
 * head_offs[0 .. *n_heads] and the first *n_heads entries of the others are
 * written.  L7M_EINVAL for conn_offs that do not ascend or pass wire_bytes. */
int l7m_http_stream_frame(const uint8_t* wire, size_t wire_bytes, const uint64_t* conn_offs /* n_conns + 1 */,
                          size_t n_conns, const l7m_http_wire_meta* conn_meta /* NULL or n_conns */,
                          uint64_t* head_offs /* cap_heads + 1 */, uint32_t* head_conn /* cap_heads */,
                          l7m_http_wire_meta* head_meta /* NULL or cap_heads */, size_t cap_heads,
                          int32_t* conn_status, uint64_t* conn_consumed, size_t* n_heads);
/* The same on device buffers, enqueued on hip_stream (NULL = default stream)
 * without synchronising: a count pass, a scan and an emit pass, one
 * connection per lane.  *d_n_heads (u64) stays on the device; the decoder and
 * the evaluator take n as a host argument, so the caller reads those 8 bytes
 * back once between framing and decoding.  Offsets that do not ascend give
 * unspecified output, without reading outside d_wire. */
int l7m_http_stream_frame_device(const void* d_wire, size_t wire_bytes, const void* d_conn_offs, size_t n_conns,
                                 const void* d_conn_meta, void* d_head_offs, void* d_head_conn, void* d_head_meta,
                                 size_t cap_heads, void* d_conn_status, void* d_conn_consumed,
                                 void* d_n_heads /* u64 */, void* hip_stream);

/* Records that wire_bytes bytes can yield: wire_bytes / 12 (the smallest frame
 * is the size field and 8 bytes).  Arena bytes that are enough for them:
 * wire_bytes + wire_bytes / 4.  Derivation: a frame of F >= 12 bytes takes
 * round_up(F, 4) <= F + 3 <= F + F / 4 arena bytes, and F + F / 4 (integer
 * division) is superadditive, so the sum over the frames is at most
 * g(wire_bytes).  The bound is met by frames of 13 bytes (size 9): 16 arena
 * bytes each.  A device arena additionally needs the evaluator's readable
 * slack: allocate round_up(bound, 16). */
size_t l7m_kafka_stream_records_bound(size_t wire_bytes);
size_t l7m_kafka_stream_arena_bound(size_t wire_bytes);
/* Host framer.  Each frame is copied to a 4-byte-aligned slot of `arena`
 * (the evaluator wants dword-aligned records, a socket does not give them)
 * with zero pad bytes: arena + rec_offsets is what l7m_eval(_ids) takes.
 * rec_conn[i] is the connection of record i and src_identities[i] =
 * conn_identity[rec_conn[i]] (src_identities NULL: not written;
 * conn_identity NULL: zeros).  conn_status, conn_consumed, *n_recs and
 * *arena_bytes are always complete.  When *n_recs > cap_recs or
 * *arena_bytes > cap_bytes the per-record arrays and the arena are untouched
 * and the call returns L7M_ENOMEM (zero capacities with NULL arrays are the
 * sizing call).  L7M_EINVAL as above. */
int l7m_kafka_stream_frame(const uint8_t* wire, size_t wire_bytes, const uint64_t* conn_offs, size_t n_conns,
                           const uint32_t* conn_identity /* NULL or n_conns */, uint8_t* arena, size_t cap_bytes,
                           uint64_t* rec_offsets, uint32_t* rec_conn, uint32_t* src_identities /* NULL or cap_recs */,
                           size_t cap_recs, int32_t* conn_status, uint64_t* conn_consumed, size_t* n_recs,
                           size_t* arena_bytes);
/* The same on device buffers (d_arena 16-byte aligned), enqueued without
 * synchronising: count pass, two scans, emit pass and a copy kernel balanced
 * over the arena.  *d_n_recs and *d_arena_bytes are u64. */
int l7m_kafka_stream_frame_device(const void* d_wire, size_t wire_bytes, const void* d_conn_offs, size_t n_conns,
                                  const void* d_conn_identity, void* d_arena, size_t cap_bytes, void* d_rec_offsets,
                                  void* d_rec_conn, void* d_src_identities, size_t cap_recs, void* d_conn_status,
                                  void* d_conn_consumed, void* d_n_recs /* u64 */, void* d_arena_bytes /* u64 */,
                                  void* hip_stream);

/* ---- streaming across calls (DESIGN.md "Streaming across calls") ----------
 * A proxy frames the same connections round after round as bytes arrive.  The
 * HTTP framer below keeps 16 bytes of state per connection between rounds, and
 * l7m_stream_carry(_device) builds the next round's wire from this round's
 * unconsumed tails and the newly arrived bytes, so that the loop frame ->
 * decode -> eval -> side effects -> carry -> frame never leaves the device.
 * The Kafka framer needs no state (conn_consumed stops at a frame boundary):
 * the one-shot framer and the carry with conn_state = NULL are its loop. */
typedef struct l7m_stream_state { /* 16 bytes; all zero = a fresh connection */
  uint64_t left;   /* BODY / CHUNK_DATA: bytes of the body or chunk still to skip */
  int32_t mode;    /* L7M_STREAM_MODE_* */
  int32_t status;  /* CLOSED: the L7M_STREAM_* code that ended the connection */
} l7m_stream_state;
#define L7M_STREAM_MODE_HEAD 0       /* at a request boundary */
#define L7M_STREAM_MODE_BODY 1       /* inside a counted body, `left` bytes to go, then HEAD */
#define L7M_STREAM_MODE_CHUNK_DATA 2 /* `left` bytes of chunk data to go (0: at the CRLF behind them) */
#define L7M_STREAM_MODE_CHUNK_LINE 3 /* at the first byte of a chunk-size line */
#define L7M_STREAM_MODE_TRAILER 4    /* at the first byte of a trailer line or of the closing empty line */
#define L7M_STREAM_MODE_CLOSED 5     /* ended with `status`; yields nothing more */

/* The resumable HTTP framer: l7m_http_stream_frame's arguments and capacity
 * contract, plus the state each connection enters with (conn_state_in, NULL =
 * all fresh) and leaves with (conn_state_out, always complete like
 * conn_status; may alias conn_state_in).  The byte rules are the one-shot's;
 * what differs is where a walk stops and starts again:
 *   - a complete head is consumed when it is emitted (conn_consumed is the end
 *     of the head, then moves through the body as it is skipped), so no head
 *     is ever emitted twice, and a body larger than any wire is framed in
 *     pieces: L7M_STREAM_EPARTIAL_BODY with the position kept in the state;
 *   - an incomplete trailing head is NOT a slice: L7M_STREAM_EPARTIAL_HEAD
 *     with conn_consumed in front of it;
 *   - EBADHEAD, TUNNEL, EAMBIGUOUS, EBADTE, EBADLENGTH and EBADCHUNK close the
 *     connection: state {0, CLOSED, status}.  A connection that enters CLOSED
 *     (or with a mode outside 0..5) yields no slice, conn_consumed = its whole
 *     length, conn_status = the state's status, and keeps its state.
 * A slice exists only for a head the decoder accepts or refuses, so slices no
 * longer tile the connections: head_offs[i] is the start of head i,
 * head_offs[n_heads] = conn_offs[n_conns] (head_offs[0] with no heads), and
 * slice i as the decoder sees it, [head_offs[i], head_offs[i+1]), may carry
 * trailing bytes that are not its own (its body, later connections' chunk
 * lines, an incomplete head).  That is sound because the decoder reads a head
 * in one pass from left to right and its code for a complete or refused head
 * is decided at or before the head's last examined byte: bytes behind it
 * change neither the status nor the record (prefix stability).
 * l7m_http_stream_heads_bound still bounds n_heads. */
int l7m_http_stream_frame_resume(const uint8_t* wire, size_t wire_bytes, const uint64_t* conn_offs, size_t n_conns,
                                 const l7m_http_wire_meta* conn_meta, uint64_t* head_offs, uint32_t* head_conn,
                                 l7m_http_wire_meta* head_meta, size_t cap_heads, int32_t* conn_status,
                                 uint64_t* conn_consumed, size_t* n_heads,
                                 const l7m_stream_state* conn_state_in /* NULL or n_conns */,
                                 l7m_stream_state* conn_state_out /* n_conns */);
/* The same on device buffers: a count pass, a scan and an emit pass, one
 * connection per lane, enqueued without synchronising. */
int l7m_http_stream_frame_resume_device(const void* d_wire, size_t wire_bytes, const void* d_conn_offs,
                                        size_t n_conns, const void* d_conn_meta, void* d_head_offs,
                                        void* d_head_conn, void* d_head_meta, size_t cap_heads, void* d_conn_status,
                                        void* d_conn_consumed, void* d_n_heads /* u64 */,
                                        const void* d_conn_state_in, void* d_conn_state_out, void* hip_stream);

/* The next round's wire (both protocols).  Connections keep their index;
 * indices n_prev .. n_conns-1 are connections opened this round (no tail; the
 * caller zeroes their state).  With T = wire[conn_offs[c] + conn_consumed[c],
 * conn_offs[c+1]) (empty for c >= n_prev) and N = seg[seg_offs[c],
 * seg_offs[c+1]), the next round's connection c is
 *   - empty when conn_status[c] is not one of OK, EPARTIAL_HEAD,
 *     EPARTIAL_BODY, EPARTIAL_FRAME, or its state's mode is CLOSED (the
 *     connection has ended; the caller saw its status and closes it);
 *   - N[k:] when its state's mode is BODY or CHUNK_DATA with left > 0, where
 *     k = min(left, |N|) (T is empty then by the framer's contract); the state
 *     gets left -= k, and a BODY that reaches 0 becomes HEAD: body bytes are
 *     never copied into the next wire;
 *   - T followed by N otherwise.
 * *next_bytes (at most l7m_stream_carry_bound) is always written.  When it
 * exceeds cap_bytes nothing else is written, the state included, and the call
 * returns L7M_ENOMEM; a call with next_conn_offs == NULL is the sizing call and
 * writes *next_bytes only.  L7M_EINVAL for offsets that do not ascend or that
 * pass their buffer, conn_consumed[c] beyond its connection and
 * n_prev > n_conns.
 * With conn_state == NULL (Kafka) nothing remembers that a connection has
 * ended: it is empty in the next round, where the framer reports OK for it,
 * and bytes supplied for it after that would be framed from mid-stream.  The
 * caller closes a connection in the round that reports its end and supplies
 * no more bytes for its index (an empty segment).  With a state the CLOSED
 * mode keeps an HTTP connection empty whatever arrives. */
size_t l7m_stream_carry_bound(size_t wire_bytes, size_t seg_bytes); /* wire_bytes + seg_bytes */
int l7m_stream_carry(const uint8_t* wire, size_t wire_bytes, const uint64_t* conn_offs /* n_prev + 1 */,
                     size_t n_prev, const int32_t* conn_status, const uint64_t* conn_consumed /* n_prev each */,
                     const uint8_t* seg, size_t seg_bytes, const uint64_t* seg_offs /* n_conns + 1 */,
                     size_t n_conns /* >= n_prev */, l7m_stream_state* conn_state /* NULL or n_conns, in and out */,
                     uint8_t* next_wire, size_t cap_bytes, uint64_t* next_conn_offs /* n_conns + 1 */,
                     uint64_t* next_bytes);
/* The same on device buffers, enqueued without synchronising: a measure pass,
 * a scan, an emit pass (offsets and state) and a copy kernel balanced over the
 * destination in 16-byte units.  d_wire and d_seg need byte alignment only;
 * d_next_wire must be 16-byte aligned and writable up to round_up(cap_bytes,
 * 16), since whole units are stored 16 bytes at a time; nothing at or past
 * round_up(*d_next_bytes, 16) is written.  *d_next_bytes is a u64; when it
 * ends up above cap_bytes nothing else was written.  Input that the host
 * function refuses gives unspecified output, without a load outside d_wire /
 * d_seg or a store outside the outputs. */
int l7m_stream_carry_device(const void* d_wire, size_t wire_bytes, const void* d_conn_offs, size_t n_prev,
                            const void* d_conn_status, const void* d_conn_consumed, const void* d_seg,
                            size_t seg_bytes, const void* d_seg_offs, size_t n_conns, void* d_conn_state,
                            void* d_next_wire, size_t cap_bytes, void* d_next_conn_offs,
                            void* d_next_bytes /* u64 */, void* hip_stream);

/* ---- evaluation flags ------------------------------------------------------
 * 0 for normal use. The DIAG flags select profiling ablations of the HTTP
 * kernel whose verdicts are NOT valid (used by bench.py --diag).  HTTP
 * programs with more than 8 value automata, RE2-dialect search automata,
 * dense automata (L7M_OPT_DENSE_DFA) or slow-path rules have no ablation
 * build: the call returns L7M_EDEVICE. */
#define L7M_FLAG_DIAG_WALK_ONLY 0x40000000u  /* stop after the DFA walks       */
#define L7M_FLAG_DIAG_COPY_ONLY 0x80000000u  /* stop after staging/validation  */

/* ---- evaluation (hot path) ----------------------------------------------
 * verdicts: int32[n].  rule_hits: NULL or uint64[n_rules + 2], ACCUMULATED
 * (not cleared): [0] denies, [1] parse errors + unsupported, [2 + i] requests
 * allowed by rule i.  flags: 0 (or L7M_FLAG_DIAG_* for profiling).
 */
int l7m_eval(const l7m_ruleset* rs, const uint8_t* arena, size_t arena_bytes,
             const uint64_t* rec_offsets, size_t n, int32_t* verdicts, uint64_t* rule_hits,
             uint32_t flags);

/* l7m_eval with the source identity of every request (u32 per request; the
 * redirect's srcIdentity, pkg/proxy/kafka.go:245).  Kafka rule sets only;
 * src_identities == NULL is every request from identity 0.  HTTP records
 * carry their remote identity themselves: L7M_EINVAL for HTTP rule sets. */
int l7m_eval_ids(const l7m_ruleset* rs, const uint8_t* arena, size_t arena_bytes,
                 const uint64_t* rec_offsets, size_t n, const uint32_t* src_identities,
                 int32_t* verdicts, uint64_t* rule_hits, uint32_t flags);

/* Device-resident variant: all pointers are device pointers on the current HIP
 * device; the work is enqueued on `hip_stream` (NULL = default stream) and the
 * call returns without synchronising.  d_arena must be 16-byte aligned and
 * readable up to round_up(arena_bytes, 16) (records are streamed with aligned
 * 16-byte loads); L7M_EINVAL otherwise. */
int l7m_eval_device(const l7m_ruleset* rs, const void* d_arena, size_t arena_bytes,
                    const void* d_rec_offsets, size_t n, void* d_verdicts, void* d_rule_hits,
                    void* hip_stream, uint32_t flags);
/* ... with device-resident source identities (see l7m_eval_ids). */
int l7m_eval_device_ids(const l7m_ruleset* rs, const void* d_arena, size_t arena_bytes,
                        const void* d_rec_offsets, size_t n, const void* d_src_identities,
                        void* d_verdicts, void* d_rule_hits, void* hip_stream, uint32_t flags);

/* ---- several GPUs from one process ----------------
 * Requests are independent, so a batch is cut into contiguous byte-balanced
 * shards, one per device, evaluated concurrently (one HIP stream per device,
 * the program replicated on each), and the per-rule counters are summed with
 * ONE RCCL all-reduce (ncclAllReduce, uint64 sum) over a single-process
 * communicator of the devices (ncclCommInitAll).  This is the in-library
 * form of bench.py's process-per-GPU sharding, for a caller that is one
 * process: cilium-agent's Kafka proxy calling canAccess
 * (pkg/proxy/kafka.go:116-152) through cgo, or one Envoy filter instance.
 * A device may appear more than once (several shards on one GPU); RCCL needs
 * distinct devices, so such sets (and L7M_MULTI_NO_RCCL=1) sum the counters
 * on the host instead.  Verdicts and counters equal one l7m_eval over the
 * whole batch.  Calls on one device set are serialised; distinct sets run
 * concurrently. */
typedef struct l7m_multi l7m_multi;
int l7m_multi_create(const int* devices, uint32_t n_devices, l7m_multi** out);
void l7m_multi_destroy(l7m_multi* m);
/* 1 when the set's counters are reduced by RCCL, 0 when on the host. */
int l7m_multi_uses_rccl(const l7m_multi* m);
/* Byte-balanced contiguous shards of a packed batch: bounds[0..parts] record
 * indices (bounds[0] = 0, bounds[parts] = n); shard k = [bounds[k],
 * bounds[k+1]) holds the records whose arena bytes are closest to k / parts
 * of the total (cilium_amd/dist.py byte_balanced_bounds).  Offsets must
 * ascend (what every packer produces): L7M_EINVAL otherwise. */
int l7m_shard_bounds(const uint64_t* rec_offsets, size_t n, size_t arena_bytes, uint32_t parts,
                     uint64_t* bounds);
/* l7m_eval_ids over the device set: host arena cut by l7m_shard_bounds,
 * each shard copied to its device, verdicts gathered, counters reduced. */
int l7m_multi_eval(l7m_multi* m, const l7m_ruleset* rs, const uint8_t* arena, size_t arena_bytes,
                   const uint64_t* rec_offsets, size_t n, const uint32_t* src_identities,
                   int32_t* verdicts, uint64_t* rule_hits, uint32_t flags);
/* Device-resident shards (HBM): shard k lives on device k of the set (its
 * pointers are device pointers there; rec_offsets relative to its arena).
 * Synchronous: returns after every device's kernels and the counter
 * all-reduce; rule_hits (host, n_rules + 2) accumulates the job's sum.
 * The set evaluates on its own (non-blocking) streams and takes no caller
 * stream: the shards' contents must be complete on their devices when this
 * is called (synchronise the stream or device that produced them first, e.g.
 * hipStreamSynchronize / torch.cuda.synchronize()); nothing orders the
 * kernels after a producer still in flight. */
typedef struct {
  const void* arena;
  size_t arena_bytes;
  const void* rec_offsets;
  size_t n;
  const void* src_identities; /* Kafka L7DataMap rule sets, or NULL */
  void* verdicts;
} l7m_shard;
int l7m_multi_eval_device(l7m_multi* m, const l7m_ruleset* rs, const l7m_shard* shards,
                          uint64_t* rule_hits, uint32_t flags);

/* ---- batching front-end (the call-site shape of the reference) ------------
 * canAccess (pkg/proxy/kafka.go:116-152) and AccessFilter::decodeHeaders
 * (envoy/cilium_l7policy.cc:126-186) decide one request per call on the
 * connection's goroutine / worker thread.  l7m_batcher keeps that blocking
 * per-request call: any number of threads call l7m_batcher_eval; their
 * records share one evaluation, flushed when max_batch requests are pending
 * (or the batch's arena is full) or the first has waited max_delay_us, while
 * the next batch fills.  Callers reserve their slot with one atomic
 * compare-and-swap (no lock); batches live in pinned, device-mapped host
 * memory that the kernels read and write in place (no copies); up to
 * in_flight batches are evaluated at once, each flusher on its own stream,
 * polling for completion; callers spin briefly, then sleep.  Destroying a
 * batcher with calls in flight is safe: pending batches are still decided,
 * later calls get L7M_EINVAL, and the memory is freed after the last caller
 * has returned.
 * l7m_batcher_set_ruleset swaps the rules for later batches (the
 * Redirect.updateRules policy update, pkg/proxy/redirect.go:68-74). */
typedef struct l7m_batcher l7m_batcher;
typedef struct {
  uint32_t struct_size;  /* sizeof(l7m_batcher_opts); 0 = defaults          */
  uint32_t max_batch;    /* requests per evaluation (0 = 65536)             */
  uint32_t max_delay_us; /* longest wait of a batch's first request (0 = 200) */
  int32_t device;        /* HIP device the batches run on                   */
  uint32_t in_flight;    /* batches evaluated concurrently (0 = 4, max 8)   */
  uint32_t eager;        /* 1: a free flusher takes the pending requests at
                            once (batch size follows the load; max_delay_us
                            unused); 0: wait for max_batch / max_delay_us  */
} l7m_batcher_opts;
int l7m_batcher_create(l7m_ruleset* rs, const l7m_batcher_opts* opts, l7m_batcher** out);
int l7m_batcher_set_ruleset(l7m_batcher* b, l7m_ruleset* rs);
/* One request (a record as in the arena); blocks until its batch is decided. */
int l7m_batcher_eval(l7m_batcher* b, const uint8_t* record, size_t len, int32_t* verdict);
/* ... from source identity src_identity (canAccess's srcIdentity; Kafka rule
 * sets compiled from an L7DataMap, see l7m_eval_ids; ignored for HTTP). */
int l7m_batcher_eval_from(l7m_batcher* b, const uint8_t* record, size_t len, uint32_t src_identity,
                          int32_t* verdict);
int l7m_batcher_eval_http(l7m_batcher* b, const l7m_http_request* req, int32_t* verdict);
/* One request head as received (l7m_http_wire_decode's grammar), decoded on
 * the calling thread into the batch.  *status as there; a refused head is not
 * submitted: *verdict = L7M_VERDICT_PARSE_ERROR and the call returns L7M_OK.
 * meta NULL: zeros, ingress. */
int l7m_batcher_eval_http_wire(l7m_batcher* b, const uint8_t* head, size_t len,
                               const l7m_http_wire_meta* meta, int32_t* verdict, int32_t* status);
int l7m_batcher_stats(l7m_batcher* b, uint64_t* batches, uint64_t* requests);
/* Where a batch's time goes (means since creation): fill = first request
 * appended -> batch closed by a flusher; launch = closed -> kernels enqueued
 * (l7m_eval_device on the batch's pinned, device-mapped buffers: records read
 * and verdicts written in place); gpu = enqueued -> completion observed by the
 * flusher (event polling); wake = completion -> the caller has its verdict
 * (mean per request). */
typedef struct {
  uint64_t batches, requests;
  double fill_us, launch_us, gpu_us, wake_us;
  /* batches served by the resident workgroup, and its mean time per batch
   * reading the slot (incl. cache invalidation), evaluating, and writing the
   * verdicts back (device clock) */
  uint64_t resident_batches, resident_rounds; /* rounds: one or more batches evaluated together */
  double resident_read_us, resident_eval_us, resident_sync_us;
} l7m_batcher_profile;
int l7m_batcher_get_profile(l7m_batcher* b, l7m_batcher_profile* out);
void l7m_batcher_destroy(l7m_batcher* b);

/* ---- verdict side effects (host; for requests the GPU decided) ------------
 * l7m_http_deny_body: the 403 body AccessFilter sends on deny: the configured
 * denied_403_body, "Access denied" when empty, CRLF-terminated
 * (envoy/cilium_l7policy.cc:89-95, 169-181).  Returns its length; writes up
 * to cap-1 bytes + NUL.
 * l7m_kafka_deny_response: the bytes handleRequest enqueues for a denied
 * Kafka request, CreateResponse(ErrTopicAuthorizationFailed)
 * (pkg/proxy/kafka.go:245-259, pkg/kafka/request.go:158-182,
 * pkg/kafka/response.go) as optiopay's Resp.Bytes(version): every topic /
 * partition of the request with error 29.  *out_len = the response size
 * (L7M_ENOMEM when cap is smaller); L7M_EUNSUPPORTED for kinds ReadRequest
 * leaves untyped ("unsupported request API key"); L7M_EINVAL if the request
 * does not decode.
 * l7m_proxy_stats_add: per-endpoint proxy counters of a batch
 * (Endpoint.UpdateProxyStatistics, pkg/endpoint/endpoint.go:2099-2122):
 * received, forwarded (allowed), denied, error (ReadRequest failed /
 * unsupported). */
typedef struct {
  uint64_t received, forwarded, denied, error;
} l7m_proxy_stats;
size_t l7m_http_deny_body(const char* configured, char* out, size_t cap);
int l7m_kafka_deny_response(const uint8_t* req, size_t len, uint8_t* out, size_t cap, size_t* out_len);
int l7m_proxy_stats_add(const int32_t* verdicts, size_t n, l7m_proxy_stats* stats);

/* Per-endpoint proxy statistics keyed as the endpoint keeps them
 * (Endpoint.UpdateProxyStatistics(l7Protocol, port, ingress, request,
 * verdict), pkg/endpoint/endpoint.go:2060-2122): one entry per (protocol,
 * port, direction, request/response).  l7m_proxy_stats_update counts each
 * request of a decided batch once, as the reference's call sites do:
 *   HTTP  - port and direction from each record (the access-log entry's
 *           DestinationEndpoint.Port / is_ingress, pkg/envoy/
 *           accesslog_server.go:165-169); `port`, `ingress` unused;
 *   Kafka - the redirect's port and direction (`port`, `ingress`); port 0
 *           is not counted, nor a request ReadRequest rejected (the proxy
 *           closes the connection) (pkg/proxy/kafka.go:213-229, 349-354).
 * Verdicts: allowed -> forwarded, L7M_VERDICT_DENY -> denied, others ->
 * error; a denied Kafka request of a kind ReadRequest leaves untyped counts
 * as error (its deny response cannot be built, pkg/proxy/kafka.go:246-252,
 * pkg/kafka/request.go:174-175).  The records are read for both protocols
 * (arena / rec_offsets required).  Thread-safe.  l7m_proxy_stats_get copies up to cap entries in key
 * order and returns the number of entries. */
typedef struct l7m_proxy_stats_table l7m_proxy_stats_table;
typedef struct {
  uint32_t proto;    /* L7M_PROTO_HTTP ("http") / L7M_PROTO_KAFKA ("kafka") */
  uint16_t port;
  uint8_t ingress;
  uint8_t request;   /* 1: Statistics.Requests (verdicts are request-side)  */
  l7m_proxy_stats stats;
} l7m_proxy_stats_entry;
l7m_proxy_stats_table* l7m_proxy_stats_table_create(void);
void l7m_proxy_stats_table_destroy(l7m_proxy_stats_table* t);
int l7m_proxy_stats_update(l7m_proxy_stats_table* t, uint32_t proto, const uint8_t* arena, size_t arena_bytes,
                           const uint64_t* rec_offsets, const int32_t* verdicts, size_t n, uint16_t port,
                           int ingress);
size_t l7m_proxy_stats_get(l7m_proxy_stats_table* t, l7m_proxy_stats_entry* out, size_t cap);
/* l7m_proxy_stats_update for an HTTP batch in device memory (d_arena with the
 * contract of l7m_eval_device, d_rec_offsets u64[n], d_verdicts i32[n]): a
 * kernel on hip_stream counts the requests per (port, direction, verdict
 * class) -- the record's own port and direction when it validates, the
 * caller's `port` and `ingress` when it does not, every request counted --
 * and the counters are added to the table, which lives on the host: the call
 * SYNCHRONISES hip_stream before it merges and returns.  proto must be
 * L7M_PROTO_HTTP.  L7M_PROTO_KAFKA answers L7M_EINVAL: a Kafka batch is keyed
 * by the caller's own (port, ingress), not by its records, so a device path
 * would amount to copying four bytes of verdict per request; use
 * l7m_proxy_stats_update.  L7M_EINVAL also for a NULL table, NULL inputs with
 * n > 0 and a d_arena that is not 16-byte aligned; L7M_EDEVICE without a
 * device. */
int l7m_proxy_stats_update_device(l7m_proxy_stats_table* t, uint32_t proto, const void* d_arena, size_t arena_bytes,
                                  const void* d_rec_offsets, const void* d_verdicts, size_t n, uint16_t port,
                                  int ingress, void* hip_stream);

/* ---- access-log records of a decided batch ---------------------------------
 * HTTP: the HttpLogEntry protobuf (envoy/cilium/accesslog.proto) Envoy's
 * filter sends over the access-log socket for each request
 * (AccessLog::Entry::InitFromRequest / UpdateFromResponse / AccessLog::Log,
 * envoy/accesslog.cc:59-170; AccessFilter::decodeHeaders / encodeHeaders,
 * envoy/cilium_l7policy.cc:166-191): EntryType Request for an allowed request,
 * Denied with status 403 for a denied one; timestamp, http_protocol,
 * policy_name, source_security_id (ingress: the record's remote identity,
 * egress: opts->local_identity), addresses (when given), scheme (the
 * x-forwarded-proto header), host / path / method, the other headers in
 * request order, is_ingress.  Messages are written back to back into out;
 * entry_offs[i] .. entry_offs[i+1] is request i's message (n + 1 entries;
 * empty for records that do not parse).  Returns the total size (out == NULL:
 * the size needed; L7M_ENOMEM when cap is too small). */
typedef struct {
  uint32_t struct_size;          /* sizeof(l7m_access_log_opts); 0 = defaults */
  uint32_t http_protocol;        /* accesslog.proto Protocol: 0 HTTP10, 1 HTTP11 (default), 2 HTTP2 */
  uint64_t timestamp_ns;         /* RequestInfo::startTime of the batch's requests */
  const char* policy_name;       /* the filter's policy_name */
  uint32_t local_identity;       /* egress: the local (source) endpoint's identity */
  uint32_t reserved;
  const char* source_address;    /* NULL: unset */
  const char* destination_address;
} l7m_access_log_opts;
int64_t l7m_http_access_log(const uint8_t* arena, size_t arena_bytes, const uint64_t* rec_offsets, size_t n,
                            const int32_t* verdicts, const l7m_access_log_opts* opts, uint8_t* out, size_t cap,
                            uint64_t* entry_offs);
/* The same entries for a batch that stayed in device memory, where
 * l7m_http_wire_decode_device / l7m_eval_device left it: three kernels
 * (measure, scan, emit) enqueued on hip_stream; the call does not synchronise
 * and the host reads no byte of the batch.  Every pointer but opts is device
 * memory.  d_arena as for l7m_eval_device: 16-byte aligned and readable up to
 * arena_bytes rounded up to 16 (L7M_EINVAL otherwise); record offsets are
 * arbitrary, as for the host function.  d_out needs no alignment.
 *   select      L7M_LOG_FORWARDED | L7M_LOG_DENIED: which requests get an
 *               entry; 0 means both.  A request outside the selection gets an
 *               empty entry, like a record that does not parse.
 *   d_entry_offs  u64[n + 1]: entry i is d_out[entry_offs[i], entry_offs[i+1]),
 *               entries back to back, byte for byte those of the host function
 *   d_total     one u64: entry_offs[n]
 * When the total exceeds cap (d_out == NULL with cap == 0 is the sizing call)
 * no byte of d_out is written, d_entry_offs and *d_total are complete all the
 * same; otherwise no byte of d_out at or past the total is written.  (The host
 * function instead writes the entries that still fit.)
 * opts is host memory, read during the call with the struct_size rule above;
 * its constant fields travel to the kernels as arguments, so policy_name,
 * source_address and destination_address are limited to 255 bytes each here
 * (L7M_EINVAL; the host function takes any length).  L7M_EINVAL also for a
 * NULL d_total, NULL inputs or d_entry_offs with n > 0, cap > 0 without d_out,
 * bits in select other than the two; L7M_EDEVICE without a device. */
#define L7M_LOG_FORWARDED 1u   /* entries for allowed requests  */
#define L7M_LOG_DENIED    2u   /* entries for denied requests   */
int l7m_http_access_log_device(const void* d_arena, size_t arena_bytes, const void* d_rec_offsets, size_t n,
                               const void* d_verdicts, const l7m_access_log_opts* opts /* host */,
                               uint32_t select /* 0 = both */, void* d_out, size_t cap,
                               void* d_entry_offs /* u64[n+1] */, void* d_total /* u64 */, void* hip_stream);
/* Kafka: the proxy's log records (kafkaLogRecord.log, pkg/proxy/kafka.go
 * :168-230; LogRecordKafka, pkg/proxy/accesslog/record.go:220-241): one
 * record per topic of GetTopics() (none for requests without topics), verdict
 * Forwarded / ErrorCode 0 for allowed requests, Denied / 29
 * (ErrTopicAuthorizationFailed) for denied ones; requests ReadRequest rejects
 * log nothing.  Topic names point into the arena.  Returns the number of
 * records (out == NULL: the number needed; L7M_ENOMEM when cap is too small).
 * l7m_kafka_api_key_name: apiKeyToString (pkg/proxy/kafka.go:161-166). */
typedef struct {
  uint64_t request;        /* index in the batch */
  uint32_t verdict;        /* accesslog.FlowVerdict: 0 Forwarded, 1 Denied, 2 Error */
  int32_t error_code;      /* Kafka.ErrorCode */
  int16_t api_key;
  int16_t api_version;
  int32_t correlation_id;
  uint64_t topic_off;      /* Kafka.Topic.Topic = arena[topic_off, topic_off + topic_len) */
  uint32_t topic_len;
  uint32_t pad;
} l7m_kafka_log_record;
int64_t l7m_kafka_access_log(const uint8_t* arena, size_t arena_bytes, const uint64_t* rec_offsets, size_t n,
                             const int32_t* verdicts, l7m_kafka_log_record* out, size_t cap);
size_t l7m_kafka_api_key_name(int16_t api_key, char* out, size_t cap);
/* l7m_kafka_deny_response for a decided batch: responses written back to back
 * into out, resp_offs[i] .. resp_offs[i+1] is request i's response (n + 1
 * entries).  Request i gets the bytes l7m_kafka_deny_response gives for its
 * record when verdicts[i] is L7M_VERDICT_DENY, the record (the size-prefixed
 * request at rec_offsets[i]) lies inside the arena and that function answers
 * L7M_OK; an empty response otherwise (an allowed request, a parse error, a
 * kind ReadRequest leaves untyped, a record that does not decode).  Returns
 * the total size (out == NULL: the size needed; L7M_ENOMEM when cap is too
 * small, the responses that still fit written and resp_offs complete).
 * L7M_EINVAL for NULL inputs or resp_offs with n > 0. */
int64_t l7m_kafka_deny_responses(const uint8_t* arena, size_t arena_bytes, const uint64_t* rec_offsets, size_t n,
                                 const int32_t* verdicts, uint8_t* out, size_t cap, uint64_t* resp_offs /* n+1 */);
/* The two for a batch that stayed in device memory, where l7m_eval_device
 * left it: three kernels each (measure, scan, emit) enqueued on hip_stream;
 * the calls do not synchronise and the host reads no byte of the batch.  Every
 * pointer is device memory.  d_arena as for l7m_eval_device: 16-byte aligned
 * and readable up to arena_bytes rounded up to 16 (L7M_EINVAL otherwise);
 * record offsets are arbitrary, unaligned ones included, as for the host
 * functions.
 * l7m_kafka_deny_responses_device: d_resp_offs u64[n + 1] and the bytes of
 *   d_out (any alignment) are those of l7m_kafka_deny_responses; d_total one
 *   u64, resp_offs[n].
 * l7m_kafka_access_log_device: d_out l7m_kafka_log_record[cap], 8-byte aligned
 *   (L7M_EINVAL otherwise); cap and *d_total count records; d_first u64[n + 1],
 *   request i's records are d_out[first[i], first[i+1]).  The records are, in
 *   order and byte for byte (pad = 0 included), those l7m_kafka_access_log
 *   fills; with select = L7M_LOG_FORWARDED | L7M_LOG_DENIED (their HTTP
 *   meaning) only those of that array whose `verdict` is in the selection, 0
 *   means all of them.  topic_off is an arena offset, valid on either side.
 * When the total exceeds cap (d_out == NULL with cap == 0 is the sizing call)
 * nothing of d_out is written, the offsets and *d_total are complete all the
 * same; otherwise no byte or record of d_out at or past the total is written.
 * (The host functions instead write what still fits.)  L7M_EINVAL also for a
 * NULL d_total, NULL inputs or offsets with n > 0, cap > 0 without d_out, bits
 * in select other than the two; L7M_EDEVICE without a device.  Proxy
 * statistics of a Kafka batch have no device twin: see
 * l7m_proxy_stats_update_device. */
int l7m_kafka_deny_responses_device(const void* d_arena, size_t arena_bytes, const void* d_rec_offsets, size_t n,
                                    const void* d_verdicts, void* d_out, size_t cap,
                                    void* d_resp_offs /* u64[n+1] */, void* d_total /* u64 */, void* hip_stream);
int l7m_kafka_access_log_device(const void* d_arena, size_t arena_bytes, const void* d_rec_offsets, size_t n,
                                const void* d_verdicts, uint32_t select /* 0 = all */,
                                void* d_out /* l7m_kafka_log_record[cap] */, size_t cap,
                                void* d_first /* u64[n+1]: index of request i's first record */,
                                void* d_total /* u64: number of records */, void* hip_stream);

/* Pinned host memory helpers (cgo may not retain Go pointers across calls).
 * l7m_eval on an arena in pinned, device-mapped memory whose padded range
 * [arena, arena + arena_bytes + 64) lies inside one such allocation (16-byte
 * aligned) runs the kernels on it in place over PCIe, with no staging copy
 * (zero-copy; L7M_ZERO_COPY=0 in the environment disables it); other arenas
 * are copied.  The 64 bytes past arena_bytes are readable slack only: the
 * kernels may read them but never use their contents as record data (the
 * copying path zero-fills them, the zero-copy path leaves them as they are).  l7m_host_mapped(p, bytes) = 1 when [p, p + bytes) qualifies. */
int l7m_alloc_pinned(size_t bytes, void** out);
void l7m_free_pinned(void* p);
int l7m_host_mapped(const void* p, size_t bytes);

/* Library / device information. */
int l7m_abi_version(void);
int l7m_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* L7MATCH_H */
