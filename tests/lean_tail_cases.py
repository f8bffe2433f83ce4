"""Records and rule sets for the lean HTTP kernel's field tails and header
directory (l7m_http_impl.h: LdsChain::run kTailWord, eval_walk kScan); needs
no GPU.  tests/test_http_lean_tails_gpu.py evaluates them on the device,
tests/test_lean_tail_cases.py checks the conditions below with the oracle.

Four families, each with its own rule set; one shared batch holds the records
of the first, second and fourth (every rule set is evaluated on the whole
batch), the third is a set of small batches of its own:

  tails      every field x length x start alignment, matching / last byte
             flipped / first byte flipped
  after      the byte behind a field completes a longer literal (no match),
             and the mirror (field one byte longer than the literal)
  last       the batch's last record: its last field ends at the arena's end
             and the slack behind it would complete a longer literal
  directory  where and how often the referenced header stands in the directory

Conditions (asserted by expectations()): in each family at least a quarter of
the cases are allowed and at least a quarter denied; every rule set is of the
lean class; the arena's last record is staged in the one form and read from
HBM in the other (last_wave_tile restates the kernel's partition).
"""
import struct

import numpy as np

from cilium_amd import l7match as L
from oracle import HttpOracle

K = 1  # directory candidates the validation pass keeps in registers (eval_walk kScan)
LENGTHS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 16, 17)
FIELDS = ("method", "path", "host", "value")
BASE = {"method": b"ABCDEFGHIJKLMNOPQRS", "path": b"/abcdefghijklmnopqr", "host": b"hijklmnopqrstuvwxyz",
        "value": b"0123456789abcdefghi"}
RULE_KEY = {"method": "Method", "path": "Path", "host": "Host"}
NAME = b"x-val"  # the referenced header of the tail families
# A batch of n < 2048 records runs in one workgroup of 16 waves, wave g taking records [n g / 16,
# n (g + 1) / 16) (l7m_kernels.hip launch_http, l7m_http_impl.h http_eval_body): the cuts at 1 ... 65
# records give every wave a few records, the cuts at 16 times as many give every wave a share of
# exactly 55, 56, 64 and 65 -- one tile, and a tile of 64 plus one record.
CUTS = (1, 55, 56, 64, 65, 16 * 55, 16 * 56, 16 * 64, 16 * 65)
WAVES, WG_RECORDS, STAGE, MIN_STAGED_TAKE = 16, 2048, 8192, 32  # program.h, kMinStagedTake


def last_wave_tile(offs, arena_bytes):
    """(k, lane of the batch's last record, records of the tile) for the first
    tile of the last wave, as http_eval_body plans it: the wave's share, and
    the leading run of k records inside a window of one record stage (STAGE is
    the largest a program gets, so k is an upper bound).  Lanes < k read the
    stage; when k < MIN_STAGED_TAKE the tile takes the whole share and the
    lanes from k on read their records from HBM."""
    n = len(offs)
    nw = WAVES * -(-n // WG_RECORDS)
    start, end = n * (nw - 1) // nw, n
    m = min(end - start, 64)
    o = [int(x) for x in offs[start:start + m]]
    onext = o[1:] + [int(offs[start + m]) if start + m < n else arena_bytes]
    base = o[0] & ~15
    k = 0
    while k < m and o[k] % 4 == 0 and o[k] >= o[0] and o[k] <= onext[k] <= arena_bytes and onext[k] - base <= STAGE:
        k += 1
    return k, n - 1 - start, m


def record(method=b"ZZZZ", path=b"/zzz", host=b"zzzz", hdrs=(), rec_len=None, dir_add=0, pad=True):
    """One raw record (include/l7match.h); None = the field is absent.  rec_len:
    the length word written (default: the true one); dir_add: added to the
    first directory entry's value length; pad=False: no padding to 4 bytes."""
    flags = (1 if method is not None else 0) | (2 if path is not None else 0) | (4 if host is not None else 0) | 8
    method, path, host = method or b"", path or b"", host or b""
    ents = [len(n) | len(v) << 16 for n, v in hdrs]
    if dir_add:
        ents[0] += dir_add << 16
    body = b"".join(struct.pack("<I", e) for e in ents) + method + path + host + b"".join(n + v for n, v in hdrs)
    size = 20 + len(body)
    rec = struct.pack("<5I", size if rec_len is None else rec_len, 0, 80 | flags << 16 | len(hdrs) << 24,
                      len(method) | len(path) << 16, len(host)) + body
    return rec + (b"\0" * (-len(rec) % 4) if pad else b"")


def flip(b, at):
    return b[:at] + b"~" + b[at + 1:]


def rule(field, value):
    if field == "value":
        return L.PortRuleHTTP(Headers=[NAME.decode() + ": " + value.decode()])
    return L.PortRuleHTTP(**{RULE_KEY[field]: value.decode()})


def with_field(field, value, shift=0, tail_hdrs=(), fill=0):
    """A record whose `field` holds `value`, starting at byte offset `shift`
    (mod 4) of its word; every other field matches no rule.  The start is
    shifted with the lengths of the fields in front; a record's method always
    starts on a word (the directory in front of it is made of words), so for
    the method `shift` only adds directory entries.  fill: unreferenced
    4-byte headers in front; tail_hdrs: headers behind the field's own."""
    filler = [(b"ua", b"vv")] * fill
    if field == "method":
        return record(value, b"/zzz", b"zzzz", filler + [(b"ua", b"vv")] * shift + list(tail_hdrs))
    if field == "path":
        return record(b"Z" * (4 + shift), value, b"zzzz", filler + list(tail_hdrs))
    if field == "host":
        return record(b"ZZZZ", b"/" + b"z" * (3 + shift), value, filler + list(tail_hdrs))
    # the value starts len(NAME) = 5 bytes behind the authority's end
    return record(b"ZZZZ", b"/zzz", b"z" * (4 + (shift - len(NAME)) % 4), filler + [(NAME, value)] + list(tail_hdrs))


# ---- family 1: tail x alignment ---------------------------------------------------
def tail_rules():
    return [rule(f, BASE[f][:n]) for f in FIELDS for n in LENGTHS if n]


def tail_units():
    out = []
    for f in FIELDS:
        for n in LENGTHS:
            v = BASE[f][:n]
            for shift in range(4):
                for x in ([v, flip(v, n - 1), flip(v, 0)] if n else [v]):
                    out.append([with_field(f, x, shift, fill=n % 3)])
    return out


# ---- family 2: bytes after the end ------------------------------------------------
AFTER_T = (1, 2, 3, 5, 6, 7)  # tails of 1, 2 and 3 bytes, alone and behind a 4-byte block
C = b"c"


def lit_x(t):  # the rules want lit_x(t) + C
    return bytes([ord("d") + t]) * t


def lit_y(t):  # the rules want lit_y(t)
    return bytes([ord("m") + t]) * t


def after_rules():
    return [rule(f, v) for f in FIELDS for t in AFTER_T for v in (lit_x(t) + C, lit_y(t))]


FILLER99 = record(b"ZZZZ", b"/" + b"z" * 74, None)  # its first byte (the length word's low byte) is 'c'
assert len(FILLER99) == 100 and FILLER99[:1] == C


def ends_record(field, value):
    """`value` as the record's last bytes, the record ending on a word, so the
    byte behind the field is the next record's first."""
    for m in range(4, 8):
        if field == "host":
            rec = record(b"Z" * m, b"/zzz", value, pad=False)
        else:
            rec = record(b"Z" * m, b"/zzz", b"zzzz", [(NAME, value)], pad=False)
        if len(rec) % 4 == 0:
            return rec
    raise AssertionError


def after_units():
    """Per field and tail: X with 'c' behind it (rule X + c: no match), X + c
    (match), Y + c (rule Y: no match), Y with 'c' behind it (match)."""
    out = []
    nxt = [(b"cx", b"v")]  # an unreferenced header whose name starts with 'c'
    for t in AFTER_T:
        x, y = lit_x(t), lit_y(t)
        for v in (x, x + C, y + C, y):
            out.append([record(v, b"c/zz", b"zzzz")])                      # method, then the path
            out.append([record(b"ZZZZ", v, b"czzz")])                      # path, then the authority
            out.append([record(b"ZZZZ", b"/zzz", v, nxt)])                 # authority, then a header name
            out.append([ends_record("host", v), FILLER99])                 # authority, then the next record
            out.append([with_field("value", v, t & 3, tail_hdrs=nxt)])     # value, then the next header's name
            out.append([ends_record("value", v), FILLER99])                # value, then the next record
    return out


# ---- family 3: the last record of the arena ----------------------------------------
BIG = record(b"ZZZZ", b"/zzz", b"zzzz", [(b"bulk", b"b" * 9000)])  # larger than a record stage: read from HBM


def last_batches():
    """(records, arena_bytes, slack, staged) per case.  The last field of the
    last record is X (rule X + c) or Y (rule Y), tails 1-3, and everything from
    its end to round_up(arena_bytes, 16) is 'c'.  arena_bytes % 16 = 0: the
    field ends at arena_bytes.  1, 5, 15: in the form "whole" the record ends
    on the last word boundary and the arena's remaining 1 or 3 bytes are 'c'
    (a record is valid only when its length rounded up to 4 lies inside the
    arena); in the form "cut" the unpadded record ends at arena_bytes itself,
    which the format rejects -- the oracle says what both kernels must say.
    staged: a few small records in front, and the last record is staged; else
    the > 8 KiB record leads the last wave's tile, nothing of which is then
    staged, and the last record is read from HBM (expectations() asserts both
    from the kernel's partition of the batch)."""
    out = []
    for field in ("host", "value"):
        for t in (1, 2, 3):
            for v in (lit_x(t), lit_y(t)):
                for mod in (0, 1, 5, 15):
                    for form in (("whole",) if mod == 0 else ("whole", "cut")):
                        for staged in (True, False):
                            last = ends_record(field, v)
                            extra = b""
                            if form == "cut":  # the record's own end at arena_bytes, mod 4 = mod & 3
                                last = None
                                for m in range(4, 8):
                                    r = record(b"Z" * m, b"/zzz", v, pad=False) if field == "host" else \
                                        record(b"Z" * m, b"/zzz", b"zzzz", [(NAME, v)], pad=False)
                                    if len(r) % 4 == (mod & 3):
                                        last = r
                                assert last is not None
                            elif mod:
                                extra = C * (mod & 3)
                            # not staged: 48 records, so the last of the 16 waves takes records 45-47,
                            # BIG, the filler and the last record, as one tile (last_wave_tile)
                            front = [with_field("path", b"/front")] * (3 if staged else 45) + ([] if staged else [BIG])
                            # a filler record in front moves the arena's end to `mod` (mod 16)
                            used = sum(len(r) for r in front) + len(last) + len(extra) + len(record())
                            gap = (mod - used) % 16
                            assert gap % 4 == 0
                            front = front + [record(path=b"/zzz" + b"z" * gap)]
                            recs = front + [last]
                            arena_bytes = sum(len(r) for r in recs) + len(extra)
                            assert arena_bytes % 16 == mod
                            out.append((recs, arena_bytes, extra, staged, form))
    return out


def last_arena(recs, arena_bytes, extra):
    """(buffer of exactly round_up(arena_bytes, 16) bytes, offsets): the arena
    and, behind arena_bytes, 'c' up to the buffer's end."""
    offs = np.cumsum([0] + [len(r) for r in recs[:-1]]).astype(np.uint64)
    buf = np.frombuffer(b"".join(recs) + extra, dtype=np.uint8)
    assert buf.nbytes == arena_bytes
    full = np.full((arena_bytes + 15) & ~15, C[0], dtype=np.uint8)
    full[:arena_bytes] = buf
    return full, offs


# ---- family 4: the header directory ------------------------------------------------
def directory_rules():
    # (the lean class: method, path and authority have an automaton each, and at most four values
    # have one, so x-val is the only header with a value matcher; x-flag and x-tenant are presence matchers)
    return [L.PortRuleHTTP(Headers=["x-val: 0123"]),
            L.PortRuleHTTP(Path="/flag", Headers=["x-flag"]),
            L.PortRuleHTTP(Headers=["x-val: 01234567", "x-tenant"]),
            L.PortRuleHTTP(Method="QQ", Host="never\\.host")]


def directory_units():
    good, bad, empty = (b"x-val", b"0123"), (b"x-val", b"0124"), (b"x-val", b"")
    look, look2 = (b"y-val", b"0123"), (b"x-vaL", b"0123")  # a referenced length, another name
    unref = (b"accept", b"*/*")  # (6 bytes: the length of x-flag, another name) -- referenced length too
    plain = (b"ua", b"curl/8")
    ten, flag = (b"x-tenant", b"t12"), (b"x-flag", b"")
    out = []
    for host in (b"z", b"zz", b"zzz", b"zzzz"):  # the directory's names at every alignment
        def rec(hdrs, path=b"/zzz", **kw):
            return [record(b"ZZZZ", path, host, hdrs, **kw)]
        out += [
            rec([]),                                               # 0 headers
            rec([good]), rec([bad]), rec([look]),                   # 1 = K
            rec([look, good]), rec([look, bad]), rec([good, look]),  # K + 1
            rec([plain, good]), rec([plain, look, plain, good]),
            rec([look, look2, unref, good]), rec([look, look2, unref, bad]), rec([look, look2, look, look2]),  # K + 3
            rec([good, bad]), rec([bad, good]),                     # a repeated name: the first occurrence wins
            rec([look, good, bad]), rec([look, bad, good]),
            rec([empty]), rec([empty, good]), rec([flag], b"/flag"), rec([flag]), rec([plain, flag], b"/flag"),
            rec([ten]), rec([plain, ten]), rec([look, ten, good]), rec([ten, bad]),  # two referenced names
            rec([(b"x-val", b"01234567"), ten]), rec([ten, plain, (b"x-val", b"01234567")]),
            rec([(b"x-val", b"01234567")]), rec([(b"x-val", b"01234567"), (b"x-tenanu", b"t12")]),
            rec([(b"x-val", b"0123456"), ten]), rec([look, (b"x-val", b"01234567"), look2, ten, flag]),
            # bad records between good ones
            rec([good]) + rec([good], rec_len=struct.unpack_from("<I", rec([good])[0])[0] + 4) + rec([good])
            + rec([plain, good], dir_add=1) + rec([good]),
        ]
    fill = [(b"h%d" % k, b"v") for k in range(254)]      # names of 2-4 bytes: no rule references these lengths
    fill5 = [(b"q%04d" % k, b"v") for k in range(254)]   # 5 bytes: every one is a candidate
    for hit in (good, bad):
        out += [[record(b"ZZZZ", b"/zzz", b"zz", [hit] + fill)],                          # first of 255
                [record(b"ZZZZ", b"/zzz", b"zz", fill[:127] + [hit] + fill[127:])],       # in the middle
                [record(b"ZZZZ", b"/zzz", b"zz", fill + [hit])],                          # last
                [record(b"ZZZZ", b"/zzz", b"zz", fill5[:40] + [hit] + fill[:214])]]
    # A referenced header behind 70,000 bytes of unreferenced values: past byte 65,535 of a record read
    # from HBM (a directory entry's value length has 16 bits, so the bytes are two values of 35,000).
    for name in (b"bulk", b"y-val"):
        for hit in (good, bad):
            out.append([record(b"ZZZZ", b"/zzz", b"zz", [(name, b"b" * 35000), (name, b"b" * 35000), hit])])
    return out


# ---- the shared batch ---------------------------------------------------------------
FAMILY_RULES = {"tails": tail_rules, "after": after_rules, "directory": directory_rules}
FAMILY_UNITS = {"tails": tail_units, "after": after_units, "directory": directory_units}


def batch():
    """(arena, offsets, {family: indices of its records}): the units of the
    three batch families in a seeded shuffled order (a unit's records stay
    adjacent), so bad and large records land inside ordinary tiles."""
    units = [(fam, u) for fam in FAMILY_UNITS for u in FAMILY_UNITS[fam]()]
    order = np.random.default_rng(14).permutation(len(units))
    recs, where = [], {fam: [] for fam in FAMILY_UNITS}
    for i in order:
        fam, u = units[i]
        where[fam] += range(len(recs), len(recs) + len(u))
        recs += u
    assert len(recs) <= 4096
    arena, offs = L.pack_records(recs)
    return arena, offs, {fam: np.array(ix) for fam, ix in where.items()}


def cut(arena, offs, n):
    """The batch's first n records as a batch of their own."""
    end = int(offs[n]) if n < len(offs) else arena.nbytes
    return arena[:end], offs[:n]


def quarter_each(exp, what):
    exp = np.asarray(exp)
    allowed, denied = (exp >= 0).sum(), (exp == L.VERDICT_DENY).sum()
    assert 4 * allowed >= len(exp) and 4 * denied >= len(exp), (what, int(allowed), int(denied), len(exp))


def expectations():
    """{family: oracle verdicts of the whole batch under the family's rules},
    the batch, and the last-record cases with their verdicts; the conditions
    are asserted on the way."""
    arena, offs, where = batch()
    exp = {}
    for fam, mk in FAMILY_RULES.items():
        assert L.RuleSet.compile_http(mk()).http_lean, fam  # (l7m_ruleset_http_lean: compiled on the host)
        exp[fam] = HttpOracle(mk()).eval(arena, offs, threads=8)
        quarter_each(exp[fam][where[fam]], fam)
    oracle = HttpOracle(after_rules())
    last, final = [], []
    for recs, arena_bytes, extra, staged, form in last_batches():
        full, loffs = last_arena(recs, arena_bytes, extra)
        k, lane, m = last_wave_tile(loffs, arena_bytes)
        if staged:
            assert lane < k, (k, lane, m)
        else:  # the tile starts with BIG: no record of it is staged and it takes its whole share
            assert recs[len(recs) - m] is BIG and k == 0 < MIN_STAGED_TAKE and k <= lane < m == 3, (k, lane, m)
        v = oracle.eval(full[:arena_bytes], loffs)
        last.append((full, arena_bytes, loffs, v, staged, form))
        final.append(int(v[-1]))
    quarter_each(final, "last")
    return (arena, offs, where), exp, last
