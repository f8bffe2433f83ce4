#!/usr/bin/env python3
"""Throughput of the HTTP/1.x wire path on one config's requests.

Generates the config's requests with the workload generator, encodes them to
request heads (l7m_http_wire_encode) and times
  - l7m_pack_http and l7m_http_wire_decode on one host thread,
  - l7m_http_wire_decode_device on HBM-resident input (HIP events, warm,
    median), reported as bytes moved (the wire read twice, the arena written)
    over time, beside l7m_eval_device on the arena it produced,
and checks that the decoded arena equals the generated one byte for byte.
Prints one JSON line; --out also writes it to a file.

    python tools/bench_http_wire.py --config 2 --n 8388608 --out profiles/r08/http_wire_cfg2.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cilium_amd import l7match as L  # noqa: E402
from cilium_amd import workloads as W  # noqa: E402

HBM_PEAK_TBS = 8.0  # MI355X HBM3E


def metas_of(arena, offs):
    """l7m_http_wire_meta of every record, from its fixed words."""
    a32 = arena[:arena.nbytes & ~3].view("<u4")
    w = (offs // 4).astype(np.int64)
    w2 = a32[w + 2]
    m = np.zeros(len(offs), dtype=L.WIRE_META_DTYPE)
    m["remote_id"] = a32[w + 1]
    m["dport"] = w2 & 0xFFFF
    m["policy"] = a32[w + 4] >> 16
    m["ingress"] = (w2 >> 16 & L.F_INGRESS) != 0
    return m


def keep_records(arena, offs, keep):
    """The arena of the records with keep[i], in order."""
    ends = np.append(offs[1:], np.uint64(arena.nbytes))
    drop = np.flatnonzero(~keep)
    parts, lo = [], 0
    for i in drop:  # the runs between dropped records
        parts.append(arena[lo:int(offs[i])])
        lo = int(ends[i])
    parts.append(arena[lo:])
    sizes = (ends - offs)[keep]
    new_offs = np.zeros(len(sizes), dtype=np.uint64)
    new_offs[1:] = np.cumsum(sizes[:-1], dtype=np.uint64)
    return np.concatenate(parts), new_offs


def requests_of(arena, offs, count):
    """The first `count` records as l7m_http_request structs (for l7m_pack_http)."""
    keep = []
    arr = (L._HttpReq * count)()
    buf = arena.tobytes()
    for i in range(count):
        o = int(offs[i])
        w = np.frombuffer(buf, dtype="<u4", count=5, offset=o)
        flags, nhdr = int(w[2]) >> 16 & 0xFF, int(w[2]) >> 24
        ml, pl, al = int(w[3]) & 0xFFFF, int(w[3]) >> 16, int(w[4]) & 0xFFFF
        d = np.frombuffer(buf, dtype="<u4", count=nhdr, offset=o + 20)
        p = o + 20 + 4 * nhdr
        method, path, auth = buf[p:p + ml], buf[p + ml:p + ml + pl], buf[p + ml + pl:p + ml + pl + al]
        p += ml + pl + al
        hdrs = []
        for e in d:
            nl, vl = int(e) & 0xFFFF, int(e) >> 16
            hdrs.append((buf[p:p + nl], buf[p + nl:p + nl + vl]))
            p += nl + vl
        q = L.HTTPRequest(method if flags & L.F_METHOD else None, path if flags & L.F_PATH else None,
                          auth if flags & L.F_AUTHORITY else None, hdrs, int(w[1]), int(w[2]) & 0xFFFF,
                          bool(flags & L.F_INGRESS), int(w[4]) >> 16)
        arr[i] = L._http_req_struct(q, keep)
    return arr, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--n", type=int, default=8 << 20)
    ap.add_argument("--pack-n", type=int, default=200000, help="requests of the l7m_pack_http leg")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true", help="one untimed device decode (for a profiler run)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("bench_http_wire: no HIP device (there is no CPU path for the device legs)")

    n = args.n
    arena, offs = W.requests(args.config, 0, n)
    arena_bytes = int(arena.nbytes) - 64  # the generator's slack
    arena = arena[:arena_bytes]
    wire, hoffs, est = L.encode_http_wire(arena, offs)
    accepted = int((est >= 0).sum())
    res = {"what": "http_wire", "config": args.config, "n_generated": n, "encoder_accepted": accepted,
           "encoder_accepted_share": accepted / n}
    if accepted != n:
        # the generator's byte mutations put bytes into a method, path or header the
        # grammar cannot carry: the legs below run on the records the encoder accepts
        res["encoder_refused_codes"] = {str(c): int((est == c).sum()) for c in np.unique(est[est < 0])}
        arena, offs = keep_records(arena, offs, est >= 0)
        arena_bytes = int(arena.nbytes)
        n = accepted
        wire, hoffs, est = L.encode_http_wire(arena, offs)
        assert int((est >= 0).sum()) == n
    res.update({"n": n, "wire_bytes": int(wire.nbytes), "arena_bytes": arena_bytes})
    meta = metas_of(arena, offs)

    # ---- host, one thread ------------------------------------------------
    cap = L.http_wire_arena_bound(wire.nbytes, n)
    host_s = None
    if not args.once:
        pn = min(args.pack_n, n)
        reqs, keep = requests_of(arena, offs, pn)
        pack_bytes = int(offs[pn]) if pn < n else arena_bytes
        out = np.zeros(pack_bytes + 64, dtype=np.uint8)
        poffs = np.zeros(pn, dtype=np.uint64)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            used = L.lib().l7m_pack_http(reqs, pn, out.ctypes.data, out.nbytes, poffs.ctypes.data)
            ts.append(time.perf_counter() - t0)
        assert used == pack_bytes
        res["host_pack_http_req_s"] = pn / statistics.median(ts)
        res["host_pack_http_n"] = pn
        del reqs, keep

        h_arena = np.zeros(cap, dtype=np.uint8)
        h_offs = np.zeros(n, dtype=np.uint64)
        h_status = np.zeros(n, dtype=np.int32)
        used = ctypes.c_size_t(0)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            rc = L.lib().l7m_http_wire_decode(wire.ctypes.data, wire.nbytes, hoffs.ctypes.data, n, meta.ctypes.data,
                                              h_arena.ctypes.data, cap, h_offs.ctypes.data, h_status.ctypes.data,
                                              ctypes.byref(used))
            ts.append(time.perf_counter() - t0)
        assert rc == L.L7M_OK
        host_s = statistics.median(ts)
        res["host_wire_decode_req_s"] = n / host_s
        res["host_wire_decode_GBs"] = wire.nbytes / host_s / 1e9
        res["host_decode_equals_generated"] = bool(
            used.value == arena_bytes and np.array_equal(h_offs, offs)
            and np.array_equal(h_arena[:arena_bytes], arena))
        del h_arena

    # ---- device ------------------------------------------------------------
    d_wire = torch.from_numpy(wire).cuda()
    d_hoffs = torch.from_numpy(hoffs.view(np.int64)).cuda()
    d_meta = torch.from_numpy(meta.view(np.uint8)).cuda()
    dcap = (cap + 15) // 16 * 16
    d_arena = torch.zeros(dcap, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def decode():
        L.decode_http_wire_device(d_wire, wire.nbytes, d_hoffs, n, d_meta, d_arena, dcap, d_offs, d_status, d_total,
                                  stream)

    if args.once:
        decode()
        torch.cuda.synchronize()
        return

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    med, lo, hi = timed(decode)
    total = int(d_total.item())
    moved = 2 * wire.nbytes + total
    res.update({"device_decode_ms_median": med, "device_decode_ms_min": lo, "device_decode_ms_max": hi,
                "device_decode_req_s": n / (med / 1e3), "device_decode_bytes_moved": moved,
                "device_decode_TBs": moved / (med / 1e3) / 1e12,
                "device_decode_share_of_hbm_peak": moved / (med / 1e3) / 1e12 / HBM_PEAK_TBS,
                "device_over_host_one_thread": (n / (med / 1e3)) / (n / host_s)})
    res["device_slower_than_16_host_threads"] = bool(res["device_over_host_one_thread"] < 16)
    same = (total == arena_bytes and np.array_equal(d_offs.cpu().numpy().view(np.uint64), offs)
            and np.array_equal(d_status.cpu().numpy(), est)
            and np.array_equal(d_arena[:arena_bytes].cpu().numpy(), arena))
    res["device_decode_equals_generated"] = bool(same)

    rs = L.RuleSet.compile_http(W.rules(args.config))
    d_verd = torch.zeros(n, dtype=torch.int32, device="cuda")
    emed, elo, ehi = timed(lambda: rs.eval_device(d_arena, total, d_offs, n, d_verd, None, stream))
    res.update({"eval_device_ms_median": emed, "eval_device_ms_min": elo, "eval_device_ms_max": ehi,
                "eval_device_req_s": n / (emed / 1e3), "decode_over_eval_time": med / emed})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
