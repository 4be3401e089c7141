"""The PNNS client on the device (he_pnns_generate_query_device, he_pnns_decrypt_response_device) against what a
caller had before them, at N = 8192, L = 4 x 55-bit moduli, a 17-bit t, one context.  One JSON line:

    python bench_tools/pnns_client_bench.py [--query-rows 1024] [--cols 128] [--database-rows 1048576]
                                            [--host-query-rows 64] [--steps K] [--warmup W]

Query side, both at the full shape: `generate_query` against quantise on the device, copy to the host, numpy dense-row packing
and SIMD encoding (the transform over [t] is the CPU oracle's, on the threads this process may use), copy back,
he_bfv_encrypt_device on the same seeds.  The two give the same words (checked before anything is timed).

Response side: `decrypt_response` on the response of `query_rows` query rows against a `database_rows`-row database (M
ciphertexts over q_0), and its mirror image -- he_bfv_decrypt_device, copy to the host, the oracle's forward transform, numpy
decoding, dense-column unpacking, centring and scaling, copy back.  The host path moves N words and runs a CPU transform per
ciphertext, so it is timed on the response of --host-query-rows query rows, and `decrypt_response` is timed at that size too:
the ratio is of two measurements at one size.  The two give the same floats (checked first).

Times are device events around the device calls and a host clock around the paths that end on the host (each ends in a copy that
synchronises); medians over --steps, alternating."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd"), os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

DEGREE, MODULI = 8192, 4


def next_power_of_two(x):
    return 1 if x <= 1 else 1 << (int(x) - 1).bit_length()


def dense_row_slots(residues, n):
    """denseRowPlaintexts up to encodeSimd in array form: [rows][cols] residues -> [K][N] slot values"""
    rows, cols = residues.shape
    padded, half = next_power_of_two(cols), n // 2
    per_plaintext = n // padded
    count = -(-rows // per_plaintext)
    k = np.arange(n, dtype=np.int64)
    out = np.zeros((count, n), dtype=np.uint64)
    for p in range(count):
        held = min(rows - p * per_plaintext, per_plaintext)
        length = held * padded
        if held == per_plaintext:
            element = k
        elif length <= half:
            element = k % next_power_of_two(length)
        else:
            element = np.where(k < half, k, half + (k - half) % next_power_of_two(length - half))
        row, column = p * per_plaintext + element // padded, element % padded
        live = (row < rows) & (column < cols)
        out[p] = np.where(live, residues[np.where(live, row, 0), np.where(live, column, 0)], np.uint64(0))
    return out


def unpack_dense_column(decoded, rows, cols, n):
    """unpackDenseColumn in array form: decoded [M][N] slots -> [rows][cols]"""
    j = np.arange(rows * cols, dtype=np.int64)
    half = n // 2
    if rows <= half:
        per_simd_row = rows * (half // rows)
        plaintext, within = j // (2 * per_simd_row), j % (2 * per_simd_row)
        slot = np.where(within < per_simd_row, within, half + within - per_simd_row)
    else:
        per_column = -(-rows // n)
        column, row = j // rows, j % rows
        plaintext, slot = column * per_column + row // n, row % n
    return decoded[plaintext, slot].reshape(cols, rows).T


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--query-rows", type=int, default=1024)
    parser.add_argument("--cols", type=int, default=128)
    parser.add_argument("--database-rows", type=int, default=1 << 20)
    parser.add_argument("--host-query-rows", type=int, default=64)
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--warmup", type=int, default=2)
    args = parser.parse_args()

    import torch

    import heamd
    import oracle
    import pnns_reference as pnns

    assert torch.cuda.is_available(), "pnns_client_bench.py measures on a GPU"
    oracle.build()
    n, L = DEGREE, MODULI
    threads = len(os.sched_getaffinity(0))
    t = heamd.generate_primes([17], True, n)[0]
    q = heamd.generate_primes([55] * (L + 1), False, n)
    bfv = heamd.BfvContext(n, t, q)
    ctx = heamd.PnnsContext(bfv)
    encoder = pnns.SimdEncoder(oracle, n, t, threads=threads)
    rng = np.random.default_rng(8)
    scaling_factor = 100.0

    def seeds(*shape):
        return torch.from_numpy(rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)).cuda()

    key = bfv.generate_secret_key(seeds(1))[0].contiguous()

    # ---- the query ---------------------------------------------------------------------------------------------------------
    query_rows, cols = args.query_rows, args.cols
    count = ctx.matrix_shape(query_rows, cols, "denseRow")["plaintext_count"]
    vectors = torch.from_numpy(rng.standard_normal((query_rows, cols)).astype(np.float32)).cuda()
    a_seeds, error_seeds = seeds(1, count), seeds(1, count)
    query_workspace = torch.empty(heamd.pnns_generate_query_workspace_bytes([ctx], query_rows, cols), dtype=torch.uint8, device="cuda")

    def query_device():
        return heamd.pnns_generate_query([ctx], vectors, scaling_factor, key, a_seeds, error_seeds, workspace=query_workspace)[0]

    def query_host():
        rounded = ctx.quantize_rows(vectors, scaling_factor).cpu().numpy()
        residues = np.where(rounded < 0, rounded + t, rounded).astype(np.uint64)
        plaintexts = heamd.to_device(np.ascontiguousarray(encoder.encode(dense_row_slots(residues, n))))
        return bfv.encrypt(plaintexts, key, a_seeds[0], error_seeds[0])

    same_query = bool(torch.equal(query_device()[0], query_host()))
    assert same_query, "generate_query and the host path differ"

    # ---- the response --------------------------------------------------------------------------------------------------------
    rows = args.database_rows

    def response_of(query_rows_of_it):
        m = ctx.matrix_shape(rows, query_rows_of_it, "denseColumn")["plaintext_count"]
        return torch.randint(0, q[0], (1, m, 2, 1, n), dtype=torch.int64, device="cuda")

    full, part = response_of(query_rows), response_of(args.host_query_rows)

    def workspace_for(query_rows_of_it):
        return torch.empty(heamd.pnns_decrypt_response_workspace_bytes([ctx], rows, query_rows_of_it), dtype=torch.uint8,
                           device="cuda")

    full_workspace, part_workspace = workspace_for(query_rows), workspace_for(args.host_query_rows)

    def response_device_full():
        return heamd.pnns_decrypt_response([ctx], full, key, rows, query_rows, scaling_factor, workspace=full_workspace)

    def response_device_part():
        return heamd.pnns_decrypt_response([ctx], part, key, rows, args.host_query_rows, scaling_factor, workspace=part_workspace)

    def response_host_part():
        plaintexts = heamd.to_host(bfv.decrypt(part[0], key))
        values = unpack_dense_column(encoder.decode(plaintexts), rows, args.host_query_rows, n).astype(np.int64)
        centred = np.where(values > (t - 1) >> 1, values - t, values)
        scale = np.float32(scaling_factor)
        return torch.from_numpy(centred.astype(np.float32) / np.float32(scale * scale)).cuda()

    same_response = bool(torch.equal(response_device_part(), response_host_part()))
    assert same_response, "decrypt_response and the host path differ"

    device_calls = {"generate_query": query_device, "decrypt_response_full": response_device_full,
                    "decrypt_response_part": response_device_part}
    host_calls = {"query_host_path": query_host, "response_host_path_part": response_host_part}
    for _ in range(args.warmup):
        for run in device_calls.values():
            run()
        query_host()
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in list(device_calls) + list(host_calls)}
    for step in range(args.steps):
        for name, run in device_calls.items():
            begin.record()
            run()
            end.record()
            end.synchronize()
            times[name].append(begin.elapsed_time(end))
        for name, run in host_calls.items():
            if name == "response_host_path_part" and step >= max(2, args.steps // 5):
                continue  # seconds per step: fewer steps
            torch.cuda.synchronize()
            start = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - start) * 1e3)
        print(f"step {step}", file=sys.stderr, flush=True)
    ms = {name: float(np.median(values)) for name, values in times.items()}
    result = {
        "tool": "pnns_client_bench", "degree": n, "L": L, "t_bits": 17, "contexts": 1, "host_threads": threads,
        "query": {"rows": query_rows, "cols": cols, "ciphertexts": count},
        "response_full": {"database_rows": rows, "query_rows": query_rows, "ciphertexts": int(full.shape[1]),
                          "bytes": int(full.numel() * 8)},
        "response_part": {"database_rows": rows, "query_rows": args.host_query_rows, "ciphertexts": int(part.shape[1])},
        "steps": {name: len(values) for name, values in times.items()}, "warmup": args.warmup,
        "same_words": same_query, "same_floats": same_response, "ms_median": ms,
        "ms_min": {name: float(min(values)) for name, values in times.items()},
        "ms_max": {name: float(max(values)) for name, values in times.items()},
        "generate_query_over_host_path": ms["generate_query"] / ms["query_host_path"],
        "decrypt_response_over_host_path_at_part": ms["decrypt_response_part"] / ms["response_host_path_part"],
        "distances_per_s_full": rows * query_rows / (ms["decrypt_response_full"] / 1e3),
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
