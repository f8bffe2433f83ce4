"""bench.py's parity leg (the oracle sample of the timed batch's verdicts),
exercised on CPU with verdicts the oracle itself produced; its options for a
plain / --full run and the --dump-outputs writer."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from cilium_amd import l7match as L  # noqa: E402
from cilium_amd import workloads as W  # noqa: E402
from oracle import HttpOracle, KafkaOracle  # noqa: E402


def _verdicts(cfg, lo, n, rules):
    a, o = W.requests(cfg, lo, n, n_rules=len(rules))
    orc = HttpOracle(rules) if cfg != 3 else KafkaOracle(rules)
    return orc.eval(a, o, threads=4)


def test_parity_leg_http_strided_sample_and_mismatch():
    rules = W.rules(2)
    lo, n = 123_456, 20_000
    v = _verdicts(2, lo, n, rules)
    r = bench.parity_leg(2, rules, v, lo, n, threads=4, n_sample=3000, blocks=16)
    assert r["mismatches"] == 0 and r["runs"] == 16 and r["sampled"] == 16 * 188
    bad = v.copy()
    bad[n - 1] = -7  # the last run ends at the shard's last request
    r = bench.parity_leg(2, rules, bad, lo, n, threads=4, n_sample=3000, blocks=16)
    assert r["mismatches"] == 1 and r["first_mismatch"] == {"request": lo + n - 1, "gpu": -7,
                                                            "oracle": int(v[n - 1])}


def test_plain_run_has_no_extra_legs_and_full_restores_them(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.no_parity and a.no_e2e and a.no_batcher and a.no_cpu_baseline
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-batcher", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.no_batcher
    assert not (a.no_parity or a.no_e2e or a.no_cpu_baseline)


def test_dump_outputs_exact_float64_and_fixed_sample(tmp_path, monkeypatch):
    import torch
    # the real cap keeps a dump under 64 MB: float64 verdicts + counters at config 5's 100k rules
    assert bench.DUMP_MAX_VERDICTS * 8 + 8 * 100_002 + 1024 < 64e6
    monkeypatch.setattr(bench, "DUMP_MAX_VERDICTS", 1000)
    v = torch.arange(5000, dtype=torch.int32)
    v[:3] = torch.tensor([L.VERDICT_ALLOW_NO_L7, L.VERDICT_DENY, L.VERDICT_ALLOW_NO_PORT_POLICY], dtype=torch.int32)
    small = v[:400]
    hits = np.array([2**40 + 1, 0, 7], dtype=np.uint64)
    bench.dump_outputs(str(tmp_path / "a"), {"verdicts": v, "small": small}, hits)
    bench.dump_outputs(str(tmp_path / "b"), {"verdicts": v, "small": small}, None)
    assert sorted(os.listdir(tmp_path / "a")) == ["hits.npy", "small.npy", "verdicts.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == ["small.npy", "verdicts.npy"]
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("hits", "small", "verdicts")}
    assert all(x.dtype == np.float64 for x in got.values())
    assert np.array_equal(got["hits"], [2**40 + 1, 0, 7])
    assert np.array_equal(got["small"], v[:400].numpy())  # whole: under its share (500) of the cap
    idx = bench.sample_index(5000, 500)
    assert len(idx) == 500 and (np.diff(idx) >= 0).all() and idx.min() >= 0 and idx.max() < 5000
    assert np.array_equal(got["verdicts"], v.numpy()[idx])  # the sample is a function of (n, cap) alone
    assert np.array_equal(got["verdicts"], np.load(tmp_path / "b" / "verdicts.npy"))
    assert bench.sample_index(500, 500) is None


def test_parity_leg_kafka_whole_small_shard():
    rules = W.rules(3, n_rules=500)
    v = _verdicts(3, 0, 1000, rules)
    r = bench.parity_leg(3, rules, v, 0, 1000, threads=4, n_sample=5000, n_rules=500)
    assert r == {**r, "sampled": 1000, "mismatches": 0, "runs": 1}
