#!/usr/bin/env python3
"""Throughput of streaming across calls: the resumable HTTP framer and the
stream carry over connections whose bytes arrive in rounds.

The wires are those of tools/bench_stream_frame.py (same generator seeds, the
unskewed grouping); each connection's bytes are cut at three uniformly random
points (numpy default_rng(19)) into ROUNDS = 4 segments.  Round 1 frames the
first segments; every later round frames what l7m_stream_carry(_device) built
from the tails and the next segments.  HTTP runs l7m_http_stream_frame_resume
with its per-connection state, Kafka the one-shot framer with conn_state = NULL.

Per round: HIP-event medians of the device framer and the device carry on
HBM-resident input, the one-thread host functions of the same run (wall clock,
median), and a check of every device output against the host's.  The sum of
the resume framer's rounds is set against the one-shot l7m_http_stream_frame_device
on the uncut wire, and the carry's copy traffic (the next wire read and
written once) against the 8 TB/s peak; the carry's time is that of the whole
call: measure, scan, emit and copy.  Needs a HIP device.  Prints one JSON line;
--out also writes it to a file.

    python tools/bench_stream_carry.py --n 2097152 --out profiles/r15/stream_carry.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import bench_stream_frame as B  # noqa: E402
from cilium_amd import l7match as L  # noqa: E402

ROUNDS = 4
CUT_SEED = 19
PEAK_TBS = 8.0


def cut(wire, coffs, rng):
    """-> per round (segment bytes uint8[], seg_offs uint64[nc + 1]) of the connections cut into ROUNDS."""
    nc = len(coffs) - 1
    lens = (coffs[1:] - coffs[:-1]).astype(np.int64)
    cuts = np.sort((rng.random((nc, ROUNDS - 1)) * (lens[:, None] + 1)).astype(np.int64), axis=1)
    edges = np.concatenate((np.zeros((nc, 1), dtype=np.int64), cuts, lens[:, None]), axis=1) + coffs[:-1, None].astype(np.int64)
    buf = wire.tobytes()
    out = []
    for r in range(ROUNDS):
        lo, hi = edges[:, r].tolist(), edges[:, r + 1].tolist()
        seg = np.frombuffer(b"".join([buf[a:b] for a, b in zip(lo, hi)]), dtype=np.uint8)
        offs = np.zeros(nc + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(edges[:, r + 1] - edges[:, r])
        out.append((seg, offs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2 << 20)
    ap.add_argument("--iters", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("bench_stream_carry: no HIP device (there is no CPU path for the device legs)")
    stream = torch.cuda.current_stream().cuda_stream
    lib = L.lib()

    def timed(fn, pre=None):
        """Median HIP-event milliseconds of fn(); pre() runs before each call, outside the events."""
        ms = []
        for i in range(args.warmup + args.iters):
            if pre:
                pre()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()

    def call(ms, host_s):
        x = host_s / (ms / 1e3)
        return {"device_ms": ms, "host_one_thread_s": host_s, "device_over_host_one_thread": x,
                "exceeds_16_host_threads": bool(x > 16)}

    res = {"what": "stream_carry", "n_generated": args.n, "rounds": ROUNDS, "cut_seed": CUT_SEED,
           "peak_TBs": PEAK_TBS}

    def leg(wire, starts, http, tag):
        n = len(starts) - 1
        coffs = starts[B.group(n, np.random.default_rng(B.SEED + (1 if http else 2)), False)].astype(np.uint64)
        nc = len(coffs) - 1
        segs = cut(wire, coffs, np.random.default_rng(CUT_SEED))
        out = {"requests": n, "connections": nc, "wire_bytes": int(wire.nbytes), "rounds": []}
        same = True
        # this round's wire: host copy and device copy
        h_wire, h_coffs = segs[0]
        d_wire, d_coffs = torch.from_numpy(h_wire.copy()).cuda(), i64(h_coffs)
        h_state = np.zeros(nc, dtype=L.STREAM_STATE_DTYPE)
        d_state = torch.zeros(16 * nc, dtype=torch.uint8, device="cuda")
        h_status, h_consumed = np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.uint64)
        d_status = torch.zeros(nc, dtype=torch.int32, device="cuda")
        d_consumed = torch.zeros(nc, dtype=torch.int64, device="cuda")
        units = 0
        for r in range(ROUNDS):
            wb = int(h_wire.nbytes)
            rnd = {"wire_bytes": wb}
            if http:
                cap = L.http_stream_heads_bound(wb, nc)
                h_offs, h_conn = np.zeros(cap + 1, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
                h_out = np.zeros(nc, dtype=L.STREAM_STATE_DTYPE)
                got = ctypes.c_size_t(0)

                def host_frame():
                    rc = lib.l7m_http_stream_frame_resume(
                        h_wire.ctypes.data, wb, h_coffs.ctypes.data, nc, None, h_offs.ctypes.data, h_conn.ctypes.data,
                        None, cap, h_status.ctypes.data, h_consumed.ctypes.data, ctypes.byref(got),
                        h_state.ctypes.data, h_out.ctypes.data)
                    assert rc == L.L7M_OK
                d_offs = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
                d_conn = torch.zeros(cap, dtype=torch.int32, device="cuda")
                d_out = torch.zeros(16 * nc, dtype=torch.uint8, device="cuda")
                d_n = torch.zeros(1, dtype=torch.int64, device="cuda")

                def dev_frame():
                    L.frame_http_streams_resume_device(d_wire, wb, d_coffs, nc, None, d_offs, d_conn, None, cap,
                                                       d_status, d_consumed, d_n, d_state, d_out, stream)
                host_s = B.median_wall(host_frame)
                ms = timed(dev_frame)
                k = got.value
                same &= (int(d_n.item()) == k
                         and np.array_equal(d_offs.cpu().numpy().view(np.uint64)[:k + 1], h_offs[:k + 1])
                         and np.array_equal(d_conn.cpu().numpy().view(np.uint32)[:k], h_conn[:k])
                         and d_out.cpu().numpy().tobytes() == h_out.tobytes())
                h_state, d_state = h_out, d_out
            else:
                cap_recs, cap_bytes = L.kafka_stream_bounds(wb)
                cap_bytes = (cap_bytes + 15) // 16 * 16
                h_arena = np.zeros(cap_bytes, dtype=np.uint8)
                h_offs, h_conn = np.zeros(cap_recs, dtype=np.uint64), np.zeros(cap_recs, dtype=np.uint32)
                got, gotb = ctypes.c_size_t(0), ctypes.c_size_t(0)

                def host_frame():
                    rc = lib.l7m_kafka_stream_frame(
                        h_wire.ctypes.data, wb, h_coffs.ctypes.data, nc, None, h_arena.ctypes.data, cap_bytes,
                        h_offs.ctypes.data, h_conn.ctypes.data, None, cap_recs, h_status.ctypes.data,
                        h_consumed.ctypes.data, ctypes.byref(got), ctypes.byref(gotb))
                    assert rc == L.L7M_OK
                d_arena = torch.zeros(cap_bytes, dtype=torch.uint8, device="cuda")
                d_offs = torch.zeros(cap_recs, dtype=torch.int64, device="cuda")
                d_conn = torch.zeros(cap_recs, dtype=torch.int32, device="cuda")
                d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
                d_nb = torch.zeros(1, dtype=torch.int64, device="cuda")

                def dev_frame():
                    L.frame_kafka_streams_device(d_wire, wb, d_coffs, nc, None, d_arena, cap_bytes, d_offs, d_conn,
                                                 None, cap_recs, d_status, d_consumed, d_n, d_nb, stream)
                host_s = B.median_wall(host_frame)
                ms = timed(dev_frame)
                k = got.value
                same &= (int(d_n.item()) == k and int(d_nb.item()) == gotb.value
                         and np.array_equal(d_arena[:gotb.value].cpu().numpy(), h_arena[:gotb.value]))
            same &= (np.array_equal(d_status.cpu().numpy(), h_status)
                     and np.array_equal(d_consumed.cpu().numpy().view(np.uint64), h_consumed))
            units += k
            rnd.update({"heads" if http else "records": k, "frame": call(ms, host_s)})
            if r + 1 < ROUNDS:
                seg, soffs = segs[r + 1]
                capb = L.stream_carry_bound(wb, seg.nbytes)
                h_next, h_noffs = np.zeros(max(1, capb), dtype=np.uint8), np.zeros(nc + 1, dtype=np.uint64)
                need = ctypes.c_uint64(0)
                h_keep = h_state.copy()

                def host_restore():
                    h_state[:] = h_keep

                def host_carry():
                    rc = lib.l7m_stream_carry(
                        h_wire.ctypes.data, wb, h_coffs.ctypes.data, nc, h_status.ctypes.data, h_consumed.ctypes.data,
                        seg.ctypes.data, seg.nbytes, soffs.ctypes.data, nc, h_state.ctypes.data if http else None,
                        h_next.ctypes.data, capb, h_noffs.ctypes.data, ctypes.byref(need))
                    assert rc == L.L7M_OK
                d_seg, d_soffs = torch.from_numpy(seg.copy()).cuda(), i64(soffs)
                d_next = torch.zeros((capb + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
                d_noffs = torch.zeros(nc + 1, dtype=torch.int64, device="cuda")
                d_need = torch.zeros(1, dtype=torch.int64, device="cuda")
                d_keep = d_state.clone()

                def dev_restore():
                    d_state.copy_(d_keep)

                def dev_carry():
                    L.carry_streams_device(d_wire, wb, d_coffs, nc, d_status, d_consumed, d_seg, seg.nbytes, d_soffs, nc,
                                           d_state if http else None, d_next, capb, d_noffs, d_need, stream)
                ts = []
                for _ in range(3):
                    host_restore()
                    ts.append(B.median_wall(host_carry, reps=1))
                ms = timed(dev_carry, dev_restore)
                total = int(need.value)
                same &= (int(d_need.item()) == total
                         and np.array_equal(d_noffs.cpu().numpy().view(np.uint64), h_noffs)
                         and np.array_equal(d_next[:total].cpu().numpy(), h_next[:total])
                         and (not http or d_state.cpu().numpy().tobytes() == h_state.tobytes()))
                c = call(ms, statistics.median(ts))
                c.update({"segment_bytes": int(seg.nbytes), "next_bytes": total,
                          "copy_GBs": 2 * total / (ms / 1e3) / 1e9,
                          "copy_share_of_peak": 2 * total / (ms / 1e3) / 1e12 / PEAK_TBS})
                rnd["carry"] = c
                h_wire, h_coffs = h_next[:total], h_noffs
                d_wire, d_coffs = d_next, d_noffs
            out["rounds"].append(rnd)
        out["heads" if http else "records"] = units
        out["frame_device_ms_sum"] = sum(x["frame"]["device_ms"] for x in out["rounds"])
        out["carry_device_ms_sum"] = sum(x["carry"]["device_ms"] for x in out["rounds"] if "carry" in x)
        out["device_equals_host"] = bool(same)
        if http:  # the parent's one-shot framer on the uncut wire
            cap = L.http_stream_heads_bound(wire.nbytes, nc)
            d_w, d_c = torch.from_numpy(wire).cuda(), i64(coffs)
            d_offs = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
            d_conn = torch.zeros(cap, dtype=torch.int32, device="cuda")
            d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
            ms = timed(lambda: L.frame_http_streams_device(d_w, wire.nbytes, d_c, nc, None, d_offs, d_conn, None, cap,
                                                           d_status, d_consumed, d_n, stream))
            out["one_shot_device_ms"] = ms
            out["one_shot_heads"] = int(d_n.item())
            out["resume_rounds_over_one_shot"] = out["frame_device_ms_sum"] / ms
        res[tag] = out

    wire, starts, with_body, chunked = B.http_requests(args.n)
    res.update({"http_requests_with_body": with_body, "http_requests_chunked": chunked})
    leg(wire, starts, True, "http")
    del wire, starts
    wire, starts = B.kafka_requests(args.n)
    leg(wire, starts, False, "kafka")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
