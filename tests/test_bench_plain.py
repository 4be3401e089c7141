"""bench.py's plain run on CPU, one rank: only what `value` / `ms_per_step` need (no pass without pre-roll, no roofline
leg), and --dump-outputs writing a fixed sample of what the last timed step computed, exactly, as float64 .npy files."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for extra in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd")):
    if extra not in sys.path:
        sys.path.insert(0, extra)

MODULUS = (1 << 55) - 55  # words wider than a float64 holds exactly


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


class CpuJob:
    """The workload interface of bench.py on a CPU tensor: each step maps every word x to (3 x + 1) mod q."""

    def __init__(self, units, words):
        import torch

        rng = np.random.default_rng(11)
        self.x = torch.from_numpy(rng.integers(0, MODULUS, size=(units, 2, words), dtype=np.uint64).view(np.int64))
        self.units = units
        self.steps_run = 0
        self.out = None

    def step(self):
        self.out = (self.x * 3 + 1) % MODULUS  # 3 x + 1 < 2^63: no overflow in int64
        self.steps_run += 1

    def result(self):
        return self.out, self.units

    def describe(self, world):
        return {"metric": "m", "unit": "u", "dtype": "u64", "config": {"workload": "cpu dry run"}}

    def roofline(self, steps, rank):
        raise AssertionError("a plain run has no roofline leg")


def _run(bench, tmp_path, units, words, steps=3, warmup=2):
    jobs = []

    def make_job():
        jobs.append(CpuJob(units, words))
        return jobs[-1]

    args = argparse.Namespace(steps=steps, warmup=warmup, skip_gather=False, full=False, dump_outputs=str(tmp_path))
    return bench.run_benchmark(args, make_job, 0, 1, device="cpu"), jobs[0]


def test_plain_run_times_exactly_the_steps_and_dumps_the_last_output(tmp_path):
    bench = _bench()
    line, job = _run(bench, tmp_path, units=7, words=64)
    assert job.steps_run == 2 + 3  # W warm-ups + K timed steps, nothing else (no pre-roll on CPU)
    assert line["steps"] == 3 and line["warmup"] == 2 and line["full"] is False
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 7) < 1e-6
    assert line["higher_is_better"] is True and line["unit"] == "u" and line["dtype"] == "u64"
    assert "value_without_pre_roll" not in line and line["roofline"] is None
    split = np.load(tmp_path / "result.npy")
    rows = np.load(tmp_path / "result_rows.npy")
    assert split.dtype == np.float64 and rows.dtype == np.float64
    assert split.shape == (7, 2, 64, 2) and list(rows) == list(range(7))  # small: every unit
    words = split[..., 0].astype(np.uint64) << np.uint64(32) | split[..., 1].astype(np.uint64)
    assert np.array_equal(words, job.out.numpy().view(np.uint64))


def test_dump_is_a_fixed_bounded_sample(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BYTES_PER_OUTPUT", 10 * 2 * 64 * 16)  # room for 10 of the 50 units
    _run(bench, tmp_path / "a", units=50, words=64)
    _run(bench, tmp_path / "b", units=50, words=64)
    rows = np.load(tmp_path / "a" / "result_rows.npy")
    assert len(rows) == 10 and len(set(rows)) == 10 and list(rows) == sorted(rows)
    assert os.path.getsize(tmp_path / "a" / "result.npy") < 10 * 2 * 64 * 16 + 256
    for name in ("result.npy", "result_rows.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))


def test_steps_must_be_positive(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()
