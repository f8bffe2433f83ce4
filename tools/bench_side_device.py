#!/usr/bin/env python3
"""Verdict side effects of an HBM-resident HTTP batch: the device access-log
encoder and proxy-statistics update against the path they replace.

Generates the config's requests with the workload generator, decides them with
l7m_eval_device and times
  - l7m_http_access_log_device for select = both and for denied only (HIP
    events, warm, median), reported as bytes moved (the arena read, the
    directory words and the per-request arrays read twice, the entries
    written) over time,
  - l7m_proxy_stats_update_device, its synchronisation and merge included
    (wall clock),
  - the replaced path on the same box: the copy of arena, offsets and verdicts
    to pinned host memory, l7m_http_access_log on one host thread and
    l7m_proxy_stats_update,
  - l7m_eval_device on the same arena, for scale,
and checks that the device entries and statistics equal the host's for the
whole batch.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_side_device.py --config 2 --n 8388608 --out profiles/r11/side_device_cfg2.json
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
OPTS = dict(policy_name="ep-7", timestamp_ns=1_700_000_000_000_000_000, local_identity=99,
            source_address="10.1.2.3:41000", destination_address="10.9.8.7:80")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--n", type=int, default=8 << 20)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true", help="one untimed device log and statistics call (for a profiler run)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("bench_side_device: no HIP device (there is no CPU path for the device legs)")

    n = args.n
    arena, offs = W.requests(args.config, 0, n)
    arena_bytes = int(arena.nbytes) - 64  # the generator's slack
    arena = arena[:arena_bytes]
    rs = L.RuleSet.compile_http(W.rules(args.config))
    stream = torch.cuda.current_stream().cuda_stream

    d_arena = torch.zeros((arena_bytes + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    d_arena[:arena_bytes].copy_(torch.from_numpy(arena))
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    d_verd = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_eo = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    rs.eval_device(d_arena, arena_bytes, d_offs, n, d_verd, None, stream)
    torch.cuda.synchronize()

    def log(select, d_out, cap):
        L.http_access_log_device(d_arena, arena_bytes, d_offs, n, d_verd, d_out, cap, d_eo, d_total, stream,
                                 select=select, **OPTS)

    # the sizing call, then a buffer of exactly that size
    log(0, None, 0)
    total = int(d_total.item())
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    if args.once:
        log(0, d_out, total)
        L.ProxyStatsTable().update_device(L.PROTO_HTTP, d_arena, arena_bytes, d_offs, d_verd, n, stream=stream)
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
    n_hdr = int((arena[:arena_bytes & ~3].view("<u4")[(offs // 4).astype(np.int64) + 2] >> 24).sum())
    res = {"what": "side_device", "config": args.config, "n": n, "arena_bytes": arena_bytes,
           "denied": int((verdicts == L.VERDICT_DENY).sum()), "forwarded": int((verdicts >= 0).sum()),
           "entry_bytes_both": total, "iters": args.iters, "warmup": args.warmup}

    def moved(entry_bytes):
        # measure: offsets, verdicts, 20 fixed bytes and the directory of every record, sizes written;
        # emit: sizes read and offsets written, offsets and verdicts again, the arena staged, entries written
        per_req = (8 + 4) * 2 + 20 + 8 * 3
        return n * per_req + 4 * n_hdr + arena_bytes + entry_bytes

    for name, select in (("both", 0), ("denied", L.LOG_DENIED)):
        med, lo, hi = timed(lambda: log(select, d_out, total))
        out_bytes = int(d_total.item())
        b = moved(out_bytes)
        res.update({f"log_{name}_ms_median": med, f"log_{name}_ms_min": lo, f"log_{name}_ms_max": hi,
                    f"log_{name}_entry_bytes": out_bytes, f"log_{name}_req_s": n / (med / 1e3),
                    f"log_{name}_bytes_moved": b, f"log_{name}_TBs": b / (med / 1e3) / 1e12,
                    f"log_{name}_share_of_hbm_peak": b / (med / 1e3) / 1e12 / HBM_PEAK_TBS})

    t_dev = L.ProxyStatsTable()
    calls = [0]

    def stats_dev():
        calls[0] += 1
        t_dev.update_device(L.PROTO_HTTP, d_arena, arena_bytes, d_offs, d_verd, n, stream=stream)

    for _ in range(args.warmup):
        stats_dev()
    med, lo, hi = wall(stats_dev, args.iters)
    res.update({"stats_device_ms_median": med * 1e3, "stats_device_ms_min": lo * 1e3, "stats_device_ms_max": hi * 1e3,
                "stats_device_includes": "memset, kernel, D2H of the counters, synchronise, host merge"})

    emed, elo, ehi = timed(lambda: rs.eval_device(d_arena, arena_bytes, d_offs, n, d_verd, None, stream))
    res.update({"eval_device_ms_median": emed, "eval_device_ms_min": elo, "eval_device_ms_max": ehi,
                "log_both_over_eval_time": res["log_both_ms_median"] / emed})

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
    o = L._AccessLogOpts(ctypes.sizeof(L._AccessLogOpts), 1, OPTS["timestamp_ns"], L._b(OPTS["policy_name"]), OPTS["local_identity"], 0,
                         L._b(OPTS["source_address"]), L._b(OPTS["destination_address"]))
    h_eo = np.zeros(n + 1, dtype=np.uint64)
    h_out = np.zeros(total, dtype=np.uint8)

    def host_log():
        got = L.lib().l7m_http_access_log(a_np.ctypes.data, arena_bytes, o_np.ctypes.data, n, v_np.ctypes.data,
                                          ctypes.byref(o), h_out.ctypes.data, total, h_eo.ctypes.data)
        assert got == total, got

    host_log()
    med, lo, hi = wall(host_log, args.host_iters)
    res.update({"host_log_one_thread_s_median": med, "host_log_one_thread_s_min": lo, "host_log_one_thread_s_max": hi,
                "host_log_one_thread_req_s": n / med,
                "device_over_host_one_thread": (n / (res["log_both_ms_median"] / 1e3)) / (n / med)})
    res["device_faster_than_16_host_threads"] = bool(res["device_over_host_one_thread"] > 16)

    t_host = L.ProxyStatsTable()

    def stats_host():
        rc = L.lib().l7m_proxy_stats_update(t_host._h, L.PROTO_HTTP, a_np.ctypes.data, arena_bytes, o_np.ctypes.data,
                                            v_np.ctypes.data, n, 0, 1)
        assert rc == L.L7M_OK

    med, lo, hi = wall(stats_host, args.host_iters)
    res.update({"host_stats_s_median": med, "replaced_path_s": res["d2h_ms_median"] / 1e3 + res["host_log_one_thread_s_median"] + med})

    # ---- equality over the whole batch ---------------------------------------
    log(0, d_out, total)
    torch.cuda.synchronize()
    same_log = (int(d_total.item()) == total and np.array_equal(d_eo.cpu().numpy().view(np.uint64), h_eo)
                and np.array_equal(d_out.cpu().numpy(), h_out))
    e_dev, e_host = t_dev.entries(), t_host.entries()
    scale = calls[0] / args.host_iters  # both tables saw the same batch, a different number of times
    same_stats = set(e_dev) == set(e_host) and all(
        e_dev[k][c] * args.host_iters == e_host[k][c] * calls[0] for k in e_dev for c in e_dev[k])
    res.update({"device_equals_host": bool(same_log and same_stats), "device_log_equals_host": bool(same_log),
                "device_stats_equal_host": bool(same_stats), "stats_rows": len(e_dev), "stats_calls_ratio": scale})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
