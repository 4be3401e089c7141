"""MulPirServer.process on the device (he_pir_process_database_device) at the PIR benchmark's ring: N = 8192, L = 4 x 55-bit
moduli (as c5), a 17-bit t, about 16 384 plaintexts out (4.3 GB Eval).  One JSON line per mode:

    python bench_tools/pir_database_bench.py --mode pack|split [--steps K] [--warmup W] [--stats kernel_stats.csv]
                                             [--cpu-plaintexts M]

pack: 120-byte entries with a size prefix (135 per plaintext); split: 40 000-byte entries (three chunks each).  Reports
plaintexts/s by events around the call (entries already on the device, enqueue-only form), the bytes the algorithm moves
(raw entries in + Eval database out + the staging slab written and read + the present mask) and, with --stats (the
kernel_stats.csv of a `rocprofv3 --kernel-trace --stats --output-format csv` run of this tool alone, whose calls are
--warmup + --steps), the kernel time per call and those bytes over it against 8 TB/s.  --cpu-plaintexts: the CPU composition (oracle unpack + plaintext_to_eval) on that many plaintexts
on the host threads the affinity mask allows."""
import argparse
import csv
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd"), os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

DEGREE, PLAINTEXTS = 8192, 16384
SHAPES = {  # mode: (dimensions, entry_size_in_bytes, entry_count)
    "pack": ([128, 128], 120, 135 * PLAINTEXTS),
    "split": ([128, 43], 40000, 5461),  # 3 chunks x 5504 slots = 16 512 plaintexts
}


def kernel_ns_per_call(stats_path, calls):
    """Sum of the library's kernels (names in namespace heamd) in a rocprofv3 kernel_stats.csv, per call."""
    total = 0
    with open(stats_path) as f:
        for row in csv.DictReader(f):
            if "heamd" in row["Name"]:
                total += int(float(row["TotalDurationNs"]))
    return total / calls


def cpu_composition(oracle, ref, mode, count):
    import pir_database_reference as refdb

    dims, entry_size, _ = SHAPES[mode]
    rng = np.random.default_rng(2)
    bits = ref.t.bit_length() - 1
    bpp = DEGREE * bits // 8
    slices = [rng.integers(0, 256, size=bpp, dtype=np.uint8).tobytes() for _ in range(count)]
    threads = len(os.sched_getaffinity(0))

    def one(batch):
        coefficients = np.stack([refdb.unpack(oracle, s, bits, DEGREE) for s in batch])
        ref.plaintext_to_eval(coefficients)

    batches = [slices[i:i + 8] for i in range(0, count, 8)]
    start = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, batches))
    seconds = time.perf_counter() - start
    return {"cpu_plaintexts": count, "cpu_threads": threads, "cpu_plaintexts_per_s": count / seconds}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--mode", choices=sorted(SHAPES), default="pack")
    parser.add_argument("--steps", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    parser.add_argument("--cpu-plaintexts", type=int, default=0)
    args = parser.parse_args()

    import heamd
    import oracle

    dims, entry_size, count = SHAPES[args.mode]
    t = heamd.generate_primes([17], True, DEGREE)[0]
    q = heamd.generate_primes([55] * 5, False, DEGREE)
    result = {"tool": "pir_database_bench", "mode": args.mode, "degree": DEGREE, "L": 4, "t_bits": 17,
              "dimensions": dims, "entry_size_in_bytes": entry_size, "entry_count": count}
    if args.cpu_plaintexts:
        oracle.build()
        result.update(cpu_composition(oracle, oracle.BfvContext(DEGREE, t, q), args.mode, args.cpu_plaintexts))
    import torch

    ctx = heamd.BfvContext(DEGREE, t, q)
    shape = ctx.pir_database_shape(dims, count, entry_size, True)
    slots = shape["chunk_count"] * shape["plaintexts_per_chunk"]
    rng = np.random.default_rng(1)
    entries = torch.from_numpy(rng.integers(0, 256, size=(count, entry_size), dtype=np.uint8)).cuda()
    database = torch.empty((slots, ctx.L, DEGREE), dtype=torch.int64, device="cuda")
    present = torch.empty(slots, dtype=torch.uint8, device="cuda")
    for _ in range(args.warmup):
        ctx.pir_process_database(entries, dims, entry_size, True, out=(database, present))
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(args.steps):
        begin.record()
        ctx.pir_process_database(entries, dims, entry_size, True, out=(database, present))
        end.record()
        end.synchronize()
        times.append(begin.elapsed_time(end))
    ms = float(np.median(times))
    bytes_in = count * entry_size
    bytes_out = slots * ctx.L * DEGREE * 8 + slots
    staging = 2 * slots * DEGREE * 8
    moved = bytes_in + bytes_out + staging
    result.update({"chunk_count": shape["chunk_count"], "plaintexts": slots, "ms_median": ms, "ms_all": times,
                   "plaintexts_per_s": slots / (ms / 1e3), "bytes_moved": moved, "bytes_raw_in": bytes_in,
                   "bytes_eval_out": bytes_out, "bytes_staging": staging,
                   "floor_ms_at_8TBps": moved / 8e12 * 1e3,
                   "fraction_of_8TBps_wall": moved / (ms / 1e3) / 8e12})
    if args.stats:
        kernel_ns = kernel_ns_per_call(args.stats, args.steps + args.warmup)
        result.update({"kernel_ms_per_call": kernel_ns / 1e6, "fraction_of_8TBps_kernel": moved / (kernel_ns / 1e9) / 8e12})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
