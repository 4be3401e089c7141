"""The MulPIR client on the device (he_pir_generate_query_device, he_pir_decrypt_response_device) against what a
caller had before them, at N = 8192, L = 4 x 55-bit moduli, a 17-bit t, dimensions [64, 32], 120-byte entries with a size prefix
(135 to a plaintext).  One JSON line:

    python bench_tools/pir_client_bench.py [--queries 1024] [--steps K] [--warmup W]

Query side: `generate_query` for --queries queries of one index against the composition a caller had: the indices copied to the
host, the selection plaintexts made there in numpy, copied back, he_bfv_encrypt_device on the same seeds.  The two give the same
words (checked before anything is timed).  `encrypt_alone` is he_bfv_encrypt_device on resident plaintexts: what the entry adds
to it is the selection kernel and the zeroization of the plaintexts.

Reply side: `decrypt_response` on --queries one-ciphertext replies over q_0 (uniform words: every plaintext coefficient below t
occurs, those at and above 2^bits too) against he_bfv_decrypt_device, the plaintexts copied to the host, the oracle's
coefficientsToBytes per reply and the entry cut out in numpy, entries and sizes copied back.  The two give the same bytes
(checked first).  `decrypt_alone` is he_bfv_decrypt_device into a resident slab; `decrypt_full` is decryptFull, whose kernel
reads every plaintext word and writes every byte.

`copy` is a device-to-device copy of the query's plaintext slab, the yardstick for the two kernels' rates (their own times come
from a kernel trace of this tool, not from it).  Times are device events around the device calls and a host clock around the
paths that end on the host; medians over --steps, alternating."""
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
DIMS, ENTRY_SIZE = [64, 32], 120


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--queries", type=int, default=1024)
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()

    import torch

    import heamd
    import oracle

    assert torch.cuda.is_available(), "pir_client_bench.py measures on a GPU"
    oracle.build()
    n, L, queries = DEGREE, MODULI, args.queries
    t = heamd.generate_primes([17], True, n)[0]
    q = heamd.generate_primes([55] * (L + 1), False, n)
    bfv = heamd.BfvContext(n, t, q)
    bits = t.bit_length() - 1
    rng = np.random.default_rng(17)

    def seeds(*shape):
        return torch.from_numpy(rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)).cuda()

    key = bfv.generate_secret_key(seeds(1))[0].contiguous()
    per = n * bits // 8 // (1 + ENTRY_SIZE)
    entry_count = per * DIMS[0] * DIMS[1] - 50
    parameter = (DIMS, entry_count, ENTRY_SIZE, True)
    plan = bfv.pir_client_plan(*parameter, 1)
    assert plan["query_ciphertext_count"] == 1 and plan["reply_ciphertext_count"] == 1 and plan["entries_per_plaintext"] == per
    indices = torch.from_numpy(rng.integers(0, entry_count, size=(queries, 1), dtype=np.int64)).cuda()

    # ---- the query ---------------------------------------------------------------------------------------------------------
    a_seeds, error_seeds = seeds(queries, 1), seeds(queries, 1)
    query_workspace = torch.empty(bfv.pir_generate_query_workspace_bytes(*parameter, 1, queries), dtype=torch.uint8, device="cuda")
    value = pow(1 << (sum(DIMS) - 1).bit_length(), -1, t)  # one index: sum(DIMS) inputs in the one ciphertext

    def query_device():
        return bfv.pir_generate_query(indices, *parameter, key, a_seeds, error_seeds, workspace=query_workspace)[0]

    def host_plaintexts():
        plaintext_index = indices.cpu().numpy()[:, 0] // per
        out = np.zeros((queries, n), dtype=np.uint64)
        rows = np.arange(queries)
        out[rows, plaintext_index // DIMS[1]] = value           # coordinate 0, most significant
        out[rows, DIMS[0] + plaintext_index % DIMS[1]] = value  # coordinate 1
        return heamd.to_device(out)

    def query_host():
        return bfv.encrypt(host_plaintexts(), key, a_seeds.view(-1, 32), error_seeds.view(-1, 32))

    resident_plaintexts = host_plaintexts()

    def encrypt_alone():
        return bfv.encrypt(resident_plaintexts, key, a_seeds.view(-1, 32), error_seeds.view(-1, 32))

    same_query = bool(torch.equal(query_device().view(queries, 2, L, n), query_host()))
    assert same_query, "generate_query and the host path differ"

    # ---- the replies ---------------------------------------------------------------------------------------------------------
    response = torch.randint(0, q[0], (queries, 1, 1, 2, 1, n), dtype=torch.int64, device="cuda")
    reply_workspace = torch.empty(bfv.pir_decrypt_response_workspace_bytes(*parameter, 1, queries, 1), dtype=torch.uint8,
                                  device="cuda")
    encoded = 1 + ENTRY_SIZE

    def reply_device():
        return bfv.pir_decrypt_response(response, indices, *parameter, key, workspace=reply_workspace)

    def reply_full():
        return bfv.pir_decrypt_response(response, None, *parameter, key, workspace=reply_workspace)[0]

    def decrypt_alone():
        return bfv.decrypt(response.view(queries, 2, 1, n), key)

    def reply_host():
        plaintexts = heamd.to_host(decrypt_alone())
        positions = indices.cpu().numpy()[:, 0] % per
        entries = np.zeros((queries, ENTRY_SIZE), dtype=np.uint8)
        sizes = np.zeros(queries, dtype=np.int64)
        for row in range(queries):
            data = oracle.coefficients_to_bytes(plaintexts[row], bits)
            record = data[positions[row] * encoded:(positions[row] + 1) * encoded]
            sizes[row] = min(int(record[0]), ENTRY_SIZE)
            entries[row, :sizes[row]] = record[1:1 + sizes[row]]
        return torch.from_numpy(entries).cuda(), torch.from_numpy(sizes).cuda()

    got, want = reply_device(), reply_host()
    same_reply = bool(torch.equal(got[0].view(queries, ENTRY_SIZE), want[0])) and bool(torch.equal(got[1].view(-1), want[1]))
    assert same_reply, "decrypt_response and the host path differ"

    copy_target = torch.empty_like(resident_plaintexts)

    def copy():
        copy_target.copy_(resident_plaintexts)

    device_calls = {"generate_query": query_device, "encrypt_alone": encrypt_alone, "decrypt_response": reply_device,
                    "decrypt_alone": decrypt_alone, "decrypt_full": reply_full, "copy": copy}
    host_calls = {"query_host_path": query_host, "reply_host_path": reply_host}
    for _ in range(args.warmup):
        for run in list(device_calls.values()) + list(host_calls.values()):
            run()
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
            torch.cuda.synchronize()
            start = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - start) * 1e3)
        print(f"step {step}", file=sys.stderr, flush=True)
    ms = {name: float(np.median(values)) for name, values in times.items()}
    slab_bytes = queries * n * 8
    result = {
        "tool": "pir_client_bench", "degree": n, "L": L, "t_bits": 17, "dimensions": DIMS, "entry_size": ENTRY_SIZE,
        "entries_per_plaintext": per, "queries": queries, "indices_per_query": 1, "host_threads": len(os.sched_getaffinity(0)),
        "steps": args.steps, "warmup": args.warmup, "same_words": same_query, "same_bytes": same_reply, "ms_median": ms,
        "ms_min": {name: float(min(values)) for name, values in times.items()},
        "ms_max": {name: float(max(values)) for name, values in times.items()},
        "generate_query_over_host_path": ms["generate_query"] / ms["query_host_path"],
        "decrypt_response_over_host_path": ms["decrypt_response"] / ms["reply_host_path"],
        "generate_query_beyond_encrypt_share": 1 - ms["encrypt_alone"] / ms["generate_query"],
        "decrypt_response_beyond_decrypt_share": 1 - ms["decrypt_alone"] / ms["decrypt_response"],
        "plaintext_slab_bytes": slab_bytes, "copy_bytes_per_s": 2 * slab_bytes / (ms["copy"] / 1e3),
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
