"""SimplePirServer on the device: computeResponse and process at the reference's two parameter pairs (7 / 28 bits in 4-byte
words, 14 / 42 bits in 8-byte words, lattice dimension 1024).  One JSON line:

    python bench_tools/simple_pir_bench.py [--config big-u32|big-u64|small-u32|all] [--steps K] [--warmup W] [--cpu-rows R]
                                           [--process-only] [--stats kernel_stats.csv]

big: 32768 entries of 32768 scalars (a square database of 2^30 elements); small: 4096 x 4096.  Per configuration: the bytes
of the database as stored; for query_count 1, 4, 16 the median and max / median of --steps (>= 30) timed compute_response
calls by events, the implied GB/s on the stored bytes and its fraction of 8 TB/s; the same for the wide layout (one word per
element, the reference's, packed from ours with unpack and answered by the same kernel family) as the A/B that shows what
the narrow layout buys; process by events -- the entry alone, with the server's context kept and the seed on the device
(--process-steps calls); and the numpy restatement's time for the query_count 1 reply on the host, measured on --cpu-rows
rows and scaled to the whole database.

The split of process into database and hint: the C ABI has no entry for one half, so events cannot give it.  It comes from
kernel time: --stats names the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats --output-format csv` run of this tool
alone with ONE --config and --process-only (every process call of that run counted: 1 + warm-up + --process-steps), and adds
process_database_kernel_ms / process_hint_kernel_ms per call to the line."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd"), os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

CONFIGS = {  # name: (plaintext_bits, ciphertext_bits, word_bits, entries = scalars per entry)
    "big-u32": (7, 28, 32, 32768),
    "big-u64": (14, 42, 64, 32768),
    "small-u32": (7, 28, 32, 4096),
}
QUERY_COUNTS = (1, 4, 16)


def timed(call, steps, warmup):
    import torch

    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(steps):
        begin.record()
        call()
        end.record()
        end.synchronize()
        times.append(begin.elapsed_time(end))
    median = float(np.median(times))
    return median, float(max(times)) / median


PROCESS_WARMUP = 2


def process_split(stats_path, calls):
    """Kernel time per process call from a rocprofv3 kernel_stats.csv: (database kernel, everything the hint launches)."""
    database = hint = 0.0
    hint_kernels = ("simple_pir_widen", "simple_pir_hint_mac", "simple_pir_replicate", "ntt_", "seeded_", "coeff_permute",
                    "narrow_kernel")
    with open(stats_path) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "simple_pir_database_kernel" in name:
                database += float(row["TotalDurationNs"])
            elif "heamd" in name and any(k in name for k in hint_kernels):
                hint += float(row["TotalDurationNs"])
    return database / calls / 1e6, hint / calls / 1e6


def run(name, steps, warmup, cpu_rows, process_steps, process_only, stats):
    import torch

    import heamd
    import simple_pir_reference as restated

    pbits, cbits, word_bits, side = CONFIGS[name]
    entry_size = side * pbits // 8
    cls = heamd.SimplePirServer if word_bits == 64 else heamd.SimplePirServer32
    rng = np.random.default_rng(1)
    entries = torch.from_numpy(rng.integers(0, 256, size=(side, entry_size), dtype=np.uint8)).cuda()
    seed = torch.arange(32, dtype=torch.uint8, device="cuda")
    server = cls.process(entries, pbits, cbits, 1024, seed)
    outputs = (server.database, server.hint)
    process_ms, process_spread = timed(lambda: server.reprocess(entries, seed, out=outputs), process_steps, PROCESS_WARMUP)
    p = server.params
    elements = p["column_size"] * p["database_columns"]
    stored = elements * p["element_bytes"]
    wide_bytes = elements * word_bits // 8
    # the wide layout: one word per element; a plaintext_bits just below ciphertext_bits selects word-sized elements
    wide = cls(server.wide_database(), server.hint, dict(p, plaintext_bits=cbits - 1))
    out = {"config": name, "plaintext_bits": pbits, "ciphertext_bits": cbits, "word_bits": word_bits, "lattice_dimension": 1024,
           "column_size": p["column_size"], "database_columns": p["database_columns"], "element_bytes": p["element_bytes"],
           "database_bytes_stored": stored, "database_bytes_wide": wide_bytes, "process_ms": process_ms, "process_max_over_median": process_spread,
           "process_calls_timed": process_steps, "replies": {}}
    if stats:
        database_ms, hint_ms = process_split(stats, 1 + PROCESS_WARMUP + process_steps)
        out.update({"process_database_kernel_ms": database_ms, "process_hint_kernel_ms": hint_ms})
    if process_only:
        return out
    to_device = heamd.to_device if word_bits == 64 else heamd.to_device32
    for q in QUERY_COUNTS:
        requests = to_device(rng.integers(0, 1 << cbits, size=(q, p["database_columns"]), dtype=np.uint64))
        row = {}
        for label, target, nbytes in (("narrow", server, stored), ("wide", wide, wide_bytes)):
            ms, spread = timed(lambda: target.compute_response(requests), steps, warmup)
            row[label] = {"ms_median": ms, "max_over_median": spread, "GBps": nbytes / ms / 1e6,
                          "fraction_of_8TBps": nbytes / (ms / 1e3) / 8e12}
        assert torch.equal(server.compute_response(requests), wide.compute_response(requests))
        row["narrow_speedup"] = row["wide"]["ms_median"] / row["narrow"]["ms_median"]
        out["replies"][str(q)] = row
    if cpu_rows:
        rows = min(cpu_rows, p["column_size"])
        block = server.database[:rows].cpu().numpy().astype(np.uint64)
        request = rng.integers(0, 1 << cbits, size=(1, p["database_columns"]), dtype=np.uint64)
        start = time.perf_counter()
        restated.compute_response(p, block, request, word_bits)
        out["cpu_numpy_reply_ms_scaled"] = (time.perf_counter() - start) * 1e3 * p["column_size"] / rows
        out["cpu_rows_measured"] = rows
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", default="all", choices=sorted(CONFIGS) + ["all"])
    parser.add_argument("--steps", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--cpu-rows", type=int, default=1024)
    parser.add_argument("--process-steps", type=int, default=10)
    parser.add_argument("--process-only", action="store_true")
    parser.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 run of this tool with one --config and --process-only")
    args = parser.parse_args()
    names = sorted(CONFIGS) if args.config == "all" else [args.config]
    print(json.dumps({"tool": "simple_pir_bench", "steps": args.steps,
                      "configs": [run(name, args.steps, args.warmup, args.cpu_rows, args.process_steps, args.process_only, args.stats)
                                  for name in names]}))


if __name__ == "__main__":
    main()
