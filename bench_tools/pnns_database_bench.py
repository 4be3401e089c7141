"""Database.process for one context on the device (heamd.PnnsContext.process_database: he_pnns_quantize_rows_device +
he_pnns_diagonal_matrix_device) at 2^20 rows x 128 columns, N = 8192, L = 4 x 55-bit moduli, a 20-bit t: 16 384 plaintexts out
(4.3 GB Eval).  One JSON line, also written to --out:

    python bench_tools/pnns_database_bench.py [--steps K] [--warmup W] [--stats kernel_stats.csv] [--cpu-plaintexts M]
                                              [--out profiles/pnns_database.json]

Reports plaintexts/s by events around the call (vectors already on the device, enqueue-only form), the bytes the algorithm
must move (float vectors in, int64 values out and in again, the staging slab written, transformed in place and read, the Eval
matrix out) against 8 TB/s and, with --stats (the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats --output-format csv`
run of this tool alone, whose calls are --warmup + --steps), the time of every library kernel per call and the pack kernel's
share.  --cpu-plaintexts: the same build through the CPU restatement (tests/pnns_reference.py over the oracle) on that many
plaintexts -- whole diagonals -- on the host threads the affinity mask allows."""
import argparse
import csv
import json
import os
import re
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd"), os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

DEGREE, ROWS, COLS, SCALE = 8192, 1 << 20, 128, 4096.0


def kernels_per_call(stats_path, calls):
    """{short kernel name: ms per call} of the library's kernels (namespace heamd) in a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(stats_path) as f:
        for row in csv.DictReader(f):
            if "heamd" not in row["Name"]:
                continue
            name = row["Name"].replace("(anonymous namespace)::", "").replace("heamd::", "")
            match = re.search(r"(\w+<[^(]*>|\w+)\(", name)
            short = match.group(1) if match else name
            out[short] = out.get(short, 0.0) + float(row["TotalDurationNs"]) / calls / 1e6
    return out


def cpu_composition(oracle, ref, t, count):
    import pnns_reference as pnns

    per_column = ROWS // DEGREE
    diagonals = max(1, count // per_column)
    rng = np.random.default_rng(2)
    vectors = rng.standard_normal((ROWS, COLS), dtype=np.float32)
    threads = len(os.sched_getaffinity(0))
    baby_step = pnns.baby_step_giant_step(COLS)[0]
    start = time.perf_counter()
    rounded = pnns.normalized_scaled_and_rounded(vectors, SCALE)
    quantize_seconds = time.perf_counter() - start

    def one(diagonal):
        encoder = pnns.SimdEncoder(oracle, DEGREE, t)
        pnns.diagonal_matrix(ref, encoder, rounded, ROWS, COLS, baby_step, False, first_diagonal=diagonal, diagonal_count=1)

    start = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(one, range(diagonals)))
    seconds = time.perf_counter() - start
    built = diagonals * per_column
    # the quantisation is paid once for the whole matrix: its share for `built` plaintexts
    total = seconds + quantize_seconds * built / (COLS * per_column)
    return {"cpu_plaintexts": built, "cpu_threads": threads, "cpu_plaintexts_per_s": built / total,
            "cpu_quantize_s_whole_matrix": quantize_seconds}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--steps", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    parser.add_argument("--stats-calls", type=int, default=0, help="calls of the traced run (default: --warmup + --steps)")
    parser.add_argument("--cpu-plaintexts", type=int, default=0)
    parser.add_argument("--out", help="also write the JSON line to this file")
    args = parser.parse_args()

    import heamd
    import oracle

    t = heamd.generate_primes([20], False, DEGREE)[0]
    q = heamd.generate_primes([55] * 5, False, DEGREE)
    result = {"tool": "pnns_database_bench", "degree": DEGREE, "L": 4, "t_bits": 20, "rows": ROWS, "cols": COLS,
              "scaling_factor": SCALE}
    if args.cpu_plaintexts:
        oracle.build()
        result.update(cpu_composition(oracle, oracle.BfvContext(DEGREE, t, q), t, args.cpu_plaintexts))
    import torch

    bfv = heamd.BfvContext(DEGREE, t, q)
    ctx = heamd.PnnsContext(bfv)
    shape = ctx.matrix_shape(ROWS, COLS)
    plaintexts = shape["plaintext_count"]
    vectors = torch.randn((ROWS, COLS), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    for _ in range(args.warmup):
        matrix, flag = ctx.process_database(vectors, SCALE)
        del matrix
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(args.steps):
        begin.record()
        matrix, flag = ctx.process_database(vectors, SCALE)
        end.record()
        end.synchronize()
        times.append(begin.elapsed_time(end))
        assert int(flag.item()) == 0
        del matrix
    ms = float(np.median(times))
    elements = ROWS * COLS
    bytes_vectors = 4 * elements + 4 * elements  # read for the norm, read again for the quotient
    bytes_values = 2 * 8 * elements              # int64 written, then read by the pack kernel
    bytes_staging = 4 * plaintexts * DEGREE * 8  # written by the pack, read and written by the inverse NTT, read by the lift
    bytes_out = plaintexts * bfv.L * DEGREE * 8
    moved = bytes_vectors + bytes_values + bytes_staging + bytes_out
    result.update({"plaintexts": plaintexts, "baby_step": shape["baby_step"], "giant_step": shape["giant_step"],
                   "ms_median": ms, "ms_all": times, "plaintexts_per_s": plaintexts / (ms / 1e3), "bytes_moved": moved,
                   "bytes_vectors": bytes_vectors, "bytes_values": bytes_values, "bytes_staging": bytes_staging,
                   "bytes_eval_out": bytes_out, "floor_ms_at_8TBps": moved / 8e12 * 1e3,
                   "fraction_of_8TBps_wall": moved / (ms / 1e3) / 8e12})
    if "cpu_plaintexts_per_s" in result:
        result["device_over_cpu"] = result["plaintexts_per_s"] / result["cpu_plaintexts_per_s"]
    if args.stats:
        per_kernel = kernels_per_call(args.stats, args.stats_calls or args.steps + args.warmup)
        kernel_ms = sum(per_kernel.values())
        pack_ms = sum(v for k, v in per_kernel.items() if k.startswith("pnns_diagonal_pack_kernel"))
        result.update({"kernel_ms_per_call": kernel_ms, "kernels_ms_per_call": per_kernel, "pack_kernel_ms_per_call": pack_ms,
                       "pack_kernel_share": pack_ms / kernel_ms if kernel_ms else None,
                       "fraction_of_8TBps_kernel": moved / (kernel_ms / 1e3) / 8e12 if kernel_ms else None})
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
