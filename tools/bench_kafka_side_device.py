#!/usr/bin/env python3
"""Verdict side effects of an HBM-resident Kafka batch: the device deny-response
and log-record encoders against the path they replace.

Generates the config's requests with the workload generator, decides them with
l7m_eval_device and times
  - l7m_kafka_deny_responses_device, l7m_kafka_access_log_device for select =
    both and for denied only (HIP events, warm, median), each reported as bytes
    moved (computed here from counts: the per-request arrays of both passes,
    the requests that are walked read twice, the output written) over time,
  - the replaced path on the same box: the copy of arena, offsets and verdicts
    to pinned host memory, l7m_kafka_access_log and l7m_kafka_deny_responses on
    one host thread; l7m_kafka_access_log also from a second build of the
    library (--baseline-lib, the parent commit's), and the faster of the two
    host rates is the baseline of the log calls,
  - l7m_eval_device on the same arena, for scale,
and checks that the device output equals the host's for the whole batch.
A device call is worth having when it runs at more than 16 x the one-thread
host rate (what sharding the host function over the box's 16 cores could
reach).  Prints one JSON line; --out also writes it to a file.

    python tools/bench_kafka_side_device.py --baseline-lib variants/parent/libl7match.so \\
        --out profiles/r12/kafka_side_device_cfg3.json
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
REC = L.KAFKA_LOG_RECORD_DTYPE.itemsize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--n", type=int, default=8 << 20)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None, help="another build of libl7match.so for the host baseline")
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true", help="one untimed call of each device function (for a profiler run)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("bench_kafka_side_device: no HIP device (there is no CPU path for the device legs)")

    n = args.n
    arena, offs = W.requests(args.config, 0, n, threads=16)
    arena_bytes = int(arena.nbytes) - 64  # the generator's slack
    arena = arena[:arena_bytes]
    rs = L.RuleSet.compile_kafka(W.rules(args.config))
    stream = torch.cuda.current_stream().cuda_stream

    d_arena = torch.zeros((arena_bytes + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    d_arena[:arena_bytes].copy_(torch.from_numpy(arena))
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    d_verd = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ro = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_first = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    rs.eval_device(d_arena, arena_bytes, d_offs, n, d_verd, None, stream)
    torch.cuda.synchronize()

    def resp(d_out, cap):
        L.kafka_deny_responses_device(d_arena, arena_bytes, d_offs, n, d_verd, d_out, cap, d_ro, d_total, stream)

    def log(select, d_out, cap):
        L.kafka_access_log_device(d_arena, arena_bytes, d_offs, n, d_verd, d_out, cap, d_first, d_total, stream,
                                  select=select)

    # the sizing calls, then buffers of exactly those sizes
    resp(None, 0)
    resp_total = int(d_total.item())
    log(0, None, 0)
    log_total = int(d_total.item())
    d_resp = torch.zeros(max(1, resp_total), dtype=torch.uint8, device="cuda")
    d_recs = torch.zeros(max(1, log_total) * REC, dtype=torch.uint8, device="cuda")
    if args.once:
        resp(d_resp, resp_total)
        log(0, d_recs, log_total)
        log(L.LOG_DENIED, d_recs, log_total)
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

    def wall(fn, iters):
        ts = []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    verdicts = d_verd.cpu().numpy()
    o = offs.astype(np.int64)
    rec_bytes = 4 + ((arena[o].astype(np.int64) << 24) | (arena[o + 1].astype(np.int64) << 16) |
                     (arena[o + 2].astype(np.int64) << 8) | arena[o + 3].astype(np.int64))
    denied = verdicts == L.VERDICT_DENY
    logged = (verdicts != L.VERDICT_PARSE_ERROR) & (verdicts != L.VERDICT_UNSUPPORTED)
    res = {"what": "kafka_side_device", "config": args.config, "n": n, "arena_bytes": arena_bytes,
           "denied": int(denied.sum()), "forwarded": int((verdicts >= 0).sum()),
           "parse_error_or_unsupported": int((~logged).sum()), "response_bytes": resp_total,
           "log_records_both": log_total, "iters": args.iters, "warmup": args.warmup}

    def moved(walked, out_bytes, emit_reads_verdict):
        # measure: offsets and verdicts read, sizes written; emit: sizes read, offsets written, and per
        # request that has output its offset (and verdict) again; a walked request is read in both passes
        k = int(walked.sum())
        return n * (8 + 4 + 8) + n * (8 + 8) + k * (8 + (4 if emit_reads_verdict else 0)) + \
            2 * int(rec_bytes[walked].sum()) + out_bytes

    legs = [("resp", lambda: resp(d_resp, resp_total), denied, 1, False),
            ("log_both", lambda: log(0, d_recs, log_total), logged, REC, True),
            ("log_denied", lambda: log(L.LOG_DENIED, d_recs, log_total), denied, REC, True)]
    for name, fn, walked, unit, rv in legs:
        med, lo, hi = timed(fn)
        out_units = int(d_total.item())
        b = moved(walked, out_units * unit, rv)
        res.update({f"{name}_ms_median": med, f"{name}_ms_min": lo, f"{name}_ms_max": hi, f"{name}_output": out_units,
                    f"{name}_req_s": n / (med / 1e3), f"{name}_bytes_moved": b, f"{name}_TBs": b / (med / 1e3) / 1e12,
                    f"{name}_share_of_hbm_peak": b / (med / 1e3) / 1e12 / HBM_PEAK_TBS})

    emed, elo, ehi = timed(lambda: rs.eval_device(d_arena, arena_bytes, d_offs, n, d_verd, None, stream))
    res.update({"eval_device_ms_median": emed, "eval_device_ms_min": elo, "eval_device_ms_max": ehi})

    # ---- the replaced path, same box ----------------------------------------
    h_arena = torch.empty(d_arena.shape[0], dtype=torch.uint8).pin_memory()
    h_offs = torch.empty(n, dtype=torch.int64).pin_memory()
    h_verd = torch.empty(n, dtype=torch.int32).pin_memory()

    def d2h():
        h_arena.copy_(d_arena, non_blocking=True)
        h_offs.copy_(d_offs, non_blocking=True)
        h_verd.copy_(d_verd, non_blocking=True)
        torch.cuda.synchronize()

    d2h()
    med, lo, hi = wall(d2h, 5)
    copied = d_arena.shape[0] + 12 * n
    res.update({"d2h_ms_median": med * 1e3, "d2h_bytes": copied, "d2h_GBs": copied / med / 1e9,
                "d2h_destination": "pinned host memory"})

    a_np, o_np, v_np = h_arena.numpy()[:arena_bytes], h_offs.numpy().view(np.uint64), h_verd.numpy()
    h_recs = np.zeros(max(1, log_total), dtype=L.KAFKA_LOG_RECORD_DTYPE)
    h_ro = np.zeros(n + 1, dtype=np.uint64)
    h_resp = np.zeros(max(1, resp_total), dtype=np.uint8)

    def host_log_with(lib):
        f = lib.l7m_kafka_access_log
        f.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_size_t]
        f.restype = ctypes.c_int64

        def run():
            got = f(a_np.ctypes.data, arena_bytes, o_np.ctypes.data, n, v_np.ctypes.data, h_recs.ctypes.data, log_total)
            assert got == log_total, got
        return run

    def host_resp():
        got = L.lib().l7m_kafka_deny_responses(a_np.ctypes.data, arena_bytes, o_np.ctypes.data, n, v_np.ctypes.data,
                                               h_resp.ctypes.data, resp_total, h_ro.ctypes.data)
        assert got == resp_total, got

    host_log = host_log_with(L.lib())
    host_log()
    med, lo, hi = wall(host_log, args.host_iters)
    res.update({"host_log_one_thread_s_median": med, "host_log_one_thread_s_min": lo, "host_log_one_thread_s_max": hi})
    best_log = med
    if args.baseline_lib:
        base_log = host_log_with(ctypes.CDLL(os.path.abspath(args.baseline_lib)))
        base_log()
        bmed, blo, bhi = wall(base_log, args.host_iters)
        res.update({"baseline_lib": args.baseline_lib, "baseline_host_log_one_thread_s_median": bmed,
                    "baseline_host_log_one_thread_s_min": blo, "baseline_host_log_one_thread_s_max": bhi})
        best_log = min(best_log, bmed)
        host_log()  # h_recs from the library under test again, for the comparison below
    host_resp()
    rmed, rlo, rhi = wall(host_resp, args.host_iters)
    res.update({"host_resp_one_thread_s_median": rmed, "host_resp_one_thread_s_min": rlo,
                "host_resp_one_thread_s_max": rhi, "host_log_baseline_s": best_log,
                "host_log_baseline_req_s": n / best_log, "host_resp_req_s": n / rmed,
                "replaced_path_s": res["d2h_ms_median"] / 1e3 + best_log + rmed})
    # the denied-only log call against the host function, which has no selection: the same baseline
    for name, base in (("resp", rmed), ("log_both", best_log), ("log_denied", best_log)):
        ratio = base / (res[f"{name}_ms_median"] / 1e3)
        res[f"{name}_device_over_host_one_thread"] = ratio
        res[f"{name}_faster_than_16_host_threads"] = bool(ratio > 16)
    res["device_faster_than_16_host_threads"] = all(res[f"{k}_faster_than_16_host_threads"]
                                                    for k in ("resp", "log_both", "log_denied"))

    # ---- equality over the whole batch ---------------------------------------
    resp(d_resp, resp_total)
    torch.cuda.synchronize()
    same_resp = (int(d_total.item()) == resp_total and np.array_equal(d_ro.cpu().numpy().view(np.uint64), h_ro)
                 and np.array_equal(d_resp.cpu().numpy()[:resp_total], h_resp[:resp_total]))
    log(0, d_recs, log_total)
    torch.cuda.synchronize()
    first = np.zeros(n + 1, dtype=np.uint64)
    first[1:] = np.cumsum(np.bincount(h_recs[:log_total]["request"].astype(np.int64), minlength=n)[:n])
    same_log = (int(d_total.item()) == log_total and np.array_equal(d_first.cpu().numpy().view(np.uint64), first)
                and d_recs.cpu().numpy()[:log_total * REC].tobytes() == h_recs[:log_total].tobytes())
    res.update({"device_equals_host": bool(same_resp and same_log), "device_resp_equals_host": bool(same_resp),
                "device_log_equals_host": bool(same_log)})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
