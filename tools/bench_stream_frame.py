#!/usr/bin/env python3
"""Throughput of stream framing on connection byte streams built from the
workload generator's requests.

HTTP leg: config 2's first --n generated records, turned into request heads by
l7m_http_wire_encode, grouped into connections whose request count is drawn
from a geometric distribution with mean 4 capped at 32 (numpy default_rng(17));
BODY_SHARE of the requests carry a body of 16, 64, 256 or 1024 bytes, half of
them counted (Content-Length), half chunked (one chunk and the last chunk).
Kafka leg: config 3's first --n requests with an honest size field,
concatenated with no padding into connections of the same distribution.
Skewed case: the same requests with the first 1 % of them in ONE connection.

Times l7m_http_stream_frame_device / l7m_kafka_stream_frame_device on
HBM-resident input (HIP events, warm, median) and the host functions on one
thread (wall clock, median) in the same run, and checks the device outputs
against the host's on the whole batch.  Needs a HIP device.  Prints one JSON
line; --out also writes it to a file.

    python tools/bench_stream_frame.py --n 8388608 --out profiles/r13/stream_frame.json
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

SEED = 17
BODY_SHARE = 0.10
BODY_SIZES = (16, 64, 256, 1024)
MEAN_REQUESTS, MAX_REQUESTS = 4, 32


def group(n, rng, skew):
    """Request index where each connection starts (and n at the end)."""
    first = n // 100 if skew else 0
    counts = np.minimum(rng.geometric(1.0 / MEAN_REQUESTS, size=n), MAX_REQUESTS)
    ends = first + np.cumsum(counts)
    ends = ends[:np.searchsorted(ends, n)]
    return np.concatenate(([0] if not first else [0, first], ends, [n])).astype(np.int64)


def http_requests(n):
    """-> (wire, request starts int64[n + 1]): the heads of config 2 with bodies behind BODY_SHARE of them."""
    arena, offs = W.requests(2, 0, n)
    arena = arena[:arena.nbytes - 64]
    wire, hoffs, est = L.encode_http_wire(arena, offs)
    ends = hoffs[1:].astype(np.int64)
    ok = est > 0  # a record the grammar cannot carry has an empty head
    rng = np.random.default_rng(SEED)
    with_body = np.flatnonzero(ok & (rng.random(n) < BODY_SHARE))
    sizes = rng.choice(BODY_SIZES, size=len(with_body))
    chunked = rng.random(len(with_body)) < 0.5
    filler = bytes(range(256)) * 4
    buf = wire.tobytes()
    parts, grow, prev = [], np.zeros(n, dtype=np.int64), 0
    for i, size, ch in zip(with_body.tolist(), sizes.tolist(), chunked.tolist()):
        cut = int(ends[i]) - 2  # in front of the empty line
        if ch:
            extra = b"Transfer-Encoding: chunked\r\n\r\n%x\r\n" % size + filler[:size] + b"\r\n0\r\n\r\n"
        else:
            extra = b"Content-Length: %d\r\n\r\n" % size + filler[:size]
        parts += [buf[prev:cut], extra]
        grow[i] = len(extra) - 2
        prev = cut + 2
    parts.append(buf[prev:])
    out = np.frombuffer(b"".join(parts), dtype=np.uint8)
    starts = np.zeros(n + 1, dtype=np.int64)
    starts[1:] = ends + np.cumsum(grow)
    keep = np.append(ok, True)  # empty heads vanish: their start equals the next one's
    return out, starts[keep], int(len(with_body)), int(chunked.sum())


def kafka_requests(n):
    """-> (wire, request starts int64[m + 1]): config 3's requests with an honest size field, unpadded."""
    arena, offs = W.requests(3, 0, n)
    arena = arena[:(arena.nbytes - 64) & ~3]  # without the generator's slack
    o = offs.astype(np.int64)
    slot = np.append(o[1:], arena.nbytes) - o
    size = arena.view(">i4")[o // 4].astype(np.int64)
    honest = (size >= 8) & (((size + 4 + 3) & ~3) == slot)
    flen = np.where(honest, size + 4, 0)
    # mark [o, o + flen): +1 at the start, -1 at the end, running sum
    d = np.zeros(arena.nbytes + 1, dtype=np.int8)
    np.add.at(d, o[honest], 1)
    np.add.at(d, (o + flen)[honest], -1)
    keep = np.cumsum(d[:-1], dtype=np.int8) > 0
    starts = np.zeros(int(honest.sum()) + 1, dtype=np.int64)
    starts[1:] = np.cumsum(flen[honest])
    return np.ascontiguousarray(arena[keep]), starts


def median_wall(fn, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8 << 20)
    ap.add_argument("--iters", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true", help="one untimed device call per leg (for a profiler run)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("bench_stream_frame: no HIP device (there is no CPU path for the device legs)")
    stream = torch.cuda.current_stream().cuda_stream
    lib = L.lib()

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

    res = {"what": "stream_frame", "n_generated": args.n, "seed": SEED, "body_share": BODY_SHARE,
           "requests_per_connection": "geometric, mean %d, capped at %d" % (MEAN_REQUESTS, MAX_REQUESTS)}

    def http_leg(wire, starts, skew, tag):
        n = len(starts) - 1
        coffs = starts[group(n, np.random.default_rng(SEED + 1), skew)].astype(np.uint64)
        nc = len(coffs) - 1
        cap = L.http_stream_heads_bound(wire.nbytes, nc)
        h_offs, h_conn = np.zeros(cap + 1, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
        h_status, h_consumed = np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.uint64)
        got = ctypes.c_size_t(0)

        def host():
            rc = lib.l7m_http_stream_frame(wire.ctypes.data, wire.nbytes, coffs.ctypes.data, nc, None,
                                           h_offs.ctypes.data, h_conn.ctypes.data, None, cap, h_status.ctypes.data,
                                           h_consumed.ctypes.data, ctypes.byref(got))
            assert rc == L.L7M_OK
        d_wire = torch.from_numpy(wire).cuda()
        d_coffs = torch.from_numpy(coffs.view(np.int64)).cuda()
        d_offs = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
        d_conn = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_status = torch.zeros(nc, dtype=torch.int32, device="cuda")
        d_consumed = torch.zeros(nc, dtype=torch.int64, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int64, device="cuda")

        def dev():
            L.frame_http_streams_device(d_wire, wire.nbytes, d_coffs, nc, None, d_offs, d_conn, None, cap, d_status,
                                        d_consumed, d_n, stream)
        if args.once:
            dev()
            torch.cuda.synchronize()
            return
        host_s = median_wall(host)
        med, lo, hi = timed(dev)
        heads = got.value
        same = (int(d_n.item()) == heads and np.array_equal(d_offs.cpu().numpy().view(np.uint64)[:heads + 1], h_offs[:heads + 1])
                and np.array_equal(d_conn.cpu().numpy().view(np.uint32)[:heads], h_conn[:heads])
                and np.array_equal(d_status.cpu().numpy(), h_status)
                and np.array_equal(d_consumed.cpu().numpy().view(np.uint64), h_consumed))
        res[tag] = {"requests": n, "connections": nc, "heads": heads, "wire_bytes": int(wire.nbytes),
                    "largest_connection_heads": int(np.bincount(h_conn[:heads], minlength=1).max()),
                    "connections_ok": int((h_status == 0).sum()),
                    "host_one_thread_s": host_s, "host_heads_s": heads / host_s, "host_GBs": wire.nbytes / host_s / 1e9,
                    "device_ms_median": med, "device_ms_min": lo, "device_ms_max": hi,
                    "device_heads_s": heads / (med / 1e3), "device_GBs": wire.nbytes / (med / 1e3) / 1e9,
                    "device_over_host_one_thread": host_s / (med / 1e3),
                    "device_slower_than_16_host_threads": bool(host_s / (med / 1e3) < 16),
                    "device_equals_host": bool(same)}

    def kafka_leg(wire, starts, skew, tag):
        n = len(starts) - 1
        coffs = starts[group(n, np.random.default_rng(SEED + 2), skew)].astype(np.uint64)
        nc = len(coffs) - 1
        ids = np.random.default_rng(SEED + 3).integers(1, 1 << 20, size=nc, dtype=np.uint32)
        cap_recs, cap_bytes = L.kafka_stream_bounds(wire.nbytes)
        cap_bytes = (cap_bytes + 15) // 16 * 16
        h_arena = np.zeros(cap_bytes, dtype=np.uint8)
        h_offs, h_conn = np.zeros(cap_recs, dtype=np.uint64), np.zeros(cap_recs, dtype=np.uint32)
        h_ids = np.zeros(cap_recs, dtype=np.uint32)
        h_status, h_consumed = np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.uint64)
        got, gotb = ctypes.c_size_t(0), ctypes.c_size_t(0)

        def host():
            rc = lib.l7m_kafka_stream_frame(wire.ctypes.data, wire.nbytes, coffs.ctypes.data, nc, ids.ctypes.data,
                                            h_arena.ctypes.data, cap_bytes, h_offs.ctypes.data, h_conn.ctypes.data,
                                            h_ids.ctypes.data, cap_recs, h_status.ctypes.data, h_consumed.ctypes.data,
                                            ctypes.byref(got), ctypes.byref(gotb))
            assert rc == L.L7M_OK
        d_wire = torch.from_numpy(wire).cuda()
        d_coffs = torch.from_numpy(coffs.view(np.int64)).cuda()
        d_cids = torch.from_numpy(ids.view(np.int32)).cuda()
        d_arena = torch.zeros(cap_bytes, dtype=torch.uint8, device="cuda")
        d_offs = torch.zeros(cap_recs, dtype=torch.int64, device="cuda")
        d_conn = torch.zeros(cap_recs, dtype=torch.int32, device="cuda")
        d_ids = torch.zeros(cap_recs, dtype=torch.int32, device="cuda")
        d_status = torch.zeros(nc, dtype=torch.int32, device="cuda")
        d_consumed = torch.zeros(nc, dtype=torch.int64, device="cuda")
        d_n, d_nb = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

        def dev():
            L.frame_kafka_streams_device(d_wire, wire.nbytes, d_coffs, nc, d_cids, d_arena, cap_bytes, d_offs, d_conn,
                                         d_ids, cap_recs, d_status, d_consumed, d_n, d_nb, stream)
        if args.once:
            dev()
            torch.cuda.synchronize()
            return
        host_s = median_wall(host)
        med, lo, hi = timed(dev)
        recs, nb = got.value, gotb.value
        same = (int(d_n.item()) == recs and int(d_nb.item()) == nb
                and np.array_equal(d_offs.cpu().numpy().view(np.uint64)[:recs], h_offs[:recs])
                and np.array_equal(d_conn.cpu().numpy().view(np.uint32)[:recs], h_conn[:recs])
                and np.array_equal(d_ids.cpu().numpy().view(np.uint32)[:recs], h_ids[:recs])
                and np.array_equal(d_arena[:nb].cpu().numpy(), h_arena[:nb])
                and np.array_equal(d_status.cpu().numpy(), h_status)
                and np.array_equal(d_consumed.cpu().numpy().view(np.uint64), h_consumed))
        moved = 2 * wire.nbytes + 2 * nb  # the wire walked twice and read once more by the copy; the arena written
        res[tag] = {"requests": n, "connections": nc, "records": recs, "wire_bytes": int(wire.nbytes), "arena_bytes": nb,
                    "largest_connection_records": int(np.bincount(h_conn[:recs], minlength=1).max()),
                    "host_one_thread_s": host_s, "host_records_s": recs / host_s, "host_GBs": wire.nbytes / host_s / 1e9,
                    "device_ms_median": med, "device_ms_min": lo, "device_ms_max": hi,
                    "device_records_s": recs / (med / 1e3), "device_GBs": wire.nbytes / (med / 1e3) / 1e9,
                    "device_bytes_moved": moved, "device_moved_TBs": moved / (med / 1e3) / 1e12,
                    "device_over_host_one_thread": host_s / (med / 1e3),
                    "device_slower_than_16_host_threads": bool(host_s / (med / 1e3) < 16),
                    "device_equals_host": bool(same)}

    wire, starts, with_body, chunked = http_requests(args.n)
    res.update({"http_requests_with_body": with_body, "http_requests_chunked": chunked})
    http_leg(wire, starts, False, "http")
    http_leg(wire, starts, True, "http_skewed")
    del wire, starts
    wire, starts = kafka_requests(args.n)
    res["kafka_requests_kept"] = len(starts) - 1
    kafka_leg(wire, starts, False, "kafka")
    kafka_leg(wire, starts, True, "kafka_skewed")
    if args.once:
        return
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
