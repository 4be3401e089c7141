"""The keyword-PIR client on the device (he_keyword_client_generate_query_device, he_keyword_client_decrypt_response_device,
he_keyword_client_find_in_buckets_device) against what a caller had before them, at N = 8192, L = 4 x 55-bit
moduli, a 17-bit t, dimensions [64, 32], h = 2, for --queries keywords.  One JSON line, also written to
profiles/keyword_pir_client_bench.json:

    python bench_tools/keyword_pir_client_bench.py [--queries 1024] [--steps K] [--warmup W] [--out FILE]

Two shapes: bucket rows of E = 1024 bytes (sixteen to a plaintext; the staged search) and of E = 40000 bytes (three reply
ciphertexts; the direct search).  Every row is a bucket of slots with 100-byte values that fills the row; the keyword's slot is
the last of its second bucket, so the search walks both chains to their ends.

  decrypt_response  against the path a caller had: he_pir_decrypt_response_device, the bucket rows copied to the host and
                    parsed there by tests/keyword_pir_client_reference.py.  The two give the same outcome (checked first).
  find_in_buckets   alone, in the plan's form and, where the row allows it, in the other, against the library's copy kernel
                    (he_words_copy_device) over the same bucket bytes; and at E = 32768, the longest staged row, in both forms.
  generate_query    against he_pir_generate_query_device on indices already resident (E = 1024 only).

Times are device events around the device calls and a host clock around the path that ends on the host; medians over --steps,
the calls of a step alternating."""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd"), os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

DEGREE, MODULI, DIMS, H = 8192, 4, [64, 32], 2
SHAPES = {"E1024": 1024, "E40000": 40000}
VALUE = 100


def bucket_row(rng, entry_size, last_hash):
    """a bucket that fills the row with slots of VALUE bytes; the last slot's hash is last_hash"""
    slots = min((entry_size - 1) // (10 + VALUE), 255)
    body = bytearray([slots])
    for slot in range(slots):
        hash_ = last_hash if slot == slots - 1 else int(rng.integers(1, 1 << 62))
        body += struct.pack("<QH", hash_, VALUE) + rng.integers(0, 256, VALUE, dtype=np.uint8).tobytes()
    return bytes(body) + bytes(entry_size - len(body))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--queries", type=int, default=1024)
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyword_pir_client_bench.json"))
    args = parser.parse_args()

    import torch

    import heamd
    import keyword_pir_client_reference as client
    import keyword_pir_reference as kw

    assert torch.cuda.is_available(), "keyword_pir_client_bench.py measures on a GPU"
    n, L, queries = DEGREE, MODULI, args.queries
    t = heamd.generate_primes([17], True, n)[0]
    bfv = heamd.BfvContext(n, t, heamd.generate_primes([55] * (L + 1), False, n))
    bits = t.bit_length() - 1
    assert bits == 16
    bpp = n * bits // 8
    rng = np.random.default_rng(19)

    def seeds(*shape):
        return torch.from_numpy(rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)).cuda()

    key = bfv.generate_secret_key(seeds(1))[0].contiguous()
    keyword_list = [b"keyword %08d" % k for k in range(queries)]
    blob, offsets = heamd.binding._blob(keyword_list)
    keywords, keyword_offsets = torch.from_numpy(blob).cuda(), torch.from_numpy(offsets.view(np.int64)).cuda()
    hashes_host = [kw.keyword_hash(k) for k in keyword_list]
    hashes = torch.from_numpy(np.array(hashes_host, dtype=np.uint64).view(np.int64)).cuda()
    device_calls, host_calls, checks, shapes = {}, {}, {}, {}

    def time_find(name, rows, keys):
        for form in ("staged", "direct"):
            if form == "staged" and rows.shape[2] > client.STAGED_ROW_LIMIT:
                continue
            device_calls["%s.find_%s" % (name, form)] = \
                lambda rows=rows, keys=keys, form=form: heamd.BfvContext.keyword_pir_find_in_buckets(rows, keys, form=form)
        target = torch.empty_like(rows)
        words = (rows.view(-1).view(torch.int64), target.view(-1).view(torch.int64))  # the copy kernel moves 8-byte words
        device_calls[name + ".copy"] = lambda words=words: heamd.stream_copy(*words)

    for name, entry_size in SHAPES.items():
        per = bpp // entry_size if bpp >= entry_size else 1
        entry_count = per * DIMS[0] * DIMS[1] - 50 if per > 1 else DIMS[0] * DIMS[1] - 50
        parameter = (DIMS, entry_count, entry_size)
        plan = bfv.keyword_pir_client_plan(*parameter, H)
        R = plan["reply_ciphertext_count"]
        indices_host = [kw.hash_indices_of_hash(hash_, entry_count, H) for hash_ in hashes_host]
        indices = torch.from_numpy(np.array(indices_host, dtype=np.int64)).cuda()
        # the replies: each bucket row at its index's position of a reply's byte string, packed 16 bits a coefficient, MSB first
        data = np.zeros((queries, H, R * bpp), dtype=np.uint8)
        rows_host = []
        for q in range(queries):
            rows_q = [bucket_row(rng, entry_size, 1), bucket_row(rng, entry_size, hashes_host[q])]
            rows_host.append(rows_q)
            for i in range(H):
                start = (indices_host[q][i] % per) * entry_size
                data[q, i, start:start + entry_size] = np.frombuffer(rows_q[i], dtype=np.uint8)
        coefficients = (data[..., 0::2].astype(np.int64) << 8) | data[..., 1::2].astype(np.int64)
        plaintexts = torch.from_numpy(coefficients.reshape(-1, n)).cuda()
        count = queries * H * R
        response = bfv.encrypt(plaintexts, key, seeds(count), seeds(count), moduli_count=1).view(queries, H, R, 2, 1, n)
        workspace = torch.empty(bfv.keyword_pir_decrypt_response_workspace_bytes(*parameter, H, queries, 1), dtype=torch.uint8,
                                device="cuda")

        def reply_device(response=response, parameter=parameter, workspace=workspace):
            return bfv.keyword_pir_decrypt_response(response, *parameter, key, hashes=hashes, workspace=workspace)

        def rows_device(response=response, parameter=parameter, indices=indices):
            return bfv.pir_decrypt_response(response, indices, *parameter, False, key)[0]

        def reply_host(rows_device=rows_device):
            rows = rows_device().cpu().numpy()
            return [client.find_in_buckets([bytes(rows[q, i]) for i in range(H)], hashes_host[q]) for q in range(queries)]

        got, want = reply_device(), reply_host()
        same = all((int(got[2][q]), int(got[1][q])) == want[q][:2] for q in range(queries)) and \
            all(bytes(got[0][q, :VALUE].cpu().numpy()) == want[q][2] for q in range(0, queries, 97)) and \
            all(status == client.FOUND for status, _, _ in want)
        assert same, "decrypt_response and the host path differ at " + name
        checks[name] = same
        shapes[name] = {"entry_size": entry_size, "entries_per_plaintext": per, "reply_ciphertexts": R,
                        "find_form": plan["find_form"], "slots_per_bucket": rows_host[0][0][0],
                        "bucket_bytes": queries * H * entry_size, "value_capacity": plan["value_capacity"]}
        device_calls[name + ".decrypt_response"] = reply_device
        device_calls[name + ".index_decrypt_response"] = rows_device
        host_calls[name + ".host_path"] = reply_host
        time_find(name, rows_device().contiguous(), hashes)
        if name == "E1024":
            C = plan["query_ciphertext_count"]
            a_seeds, error_seeds = seeds(queries, C), seeds(queries, C)
            query_workspace = torch.empty(bfv.keyword_pir_generate_query_workspace_bytes(*parameter, H, queries), dtype=torch.uint8,
                                          device="cuda")

            def query_device(parameter=parameter, a_seeds=a_seeds, error_seeds=error_seeds, query_workspace=query_workspace):
                return bfv.keyword_pir_generate_query(keywords, keyword_offsets, *parameter, H, key, a_seeds, error_seeds,
                                                      workspace=query_workspace)[0]

            def query_index(parameter=parameter, indices=indices, a_seeds=a_seeds, error_seeds=error_seeds):
                return bfv.pir_generate_query(indices, *parameter, False, key, a_seeds, error_seeds)[0]

            checks["same_query_words"] = bool(torch.equal(query_device(), query_index()))
            assert checks["same_query_words"], "generate_query and he_pir_generate_query_device on the indices differ"
            device_calls["generate_query"], device_calls["index_generate_query"] = query_device, query_index
    # the longest staged row, both forms, bytes alone
    longest = client.STAGED_ROW_LIMIT
    rows = torch.from_numpy(np.frombuffer(b"".join(bucket_row(rng, longest, 1) + bucket_row(rng, longest, hashes_host[q])
                                                   for q in range(queries)), dtype=np.uint8).copy()).cuda().view(queries, H, longest)
    shapes["E32768"] = {"entry_size": longest, "bucket_bytes": queries * H * longest, "slots_per_bucket": int(rows[0, 0, 0])}
    time_find("E32768", rows, hashes)

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
    result = {
        "tool": "keyword_pir_client_bench", "degree": n, "L": L, "t_bits": 17, "dimensions": DIMS, "hash_function_count": H,
        "queries": queries, "value_bytes": VALUE, "host_threads": len(os.sched_getaffinity(0)), "steps": args.steps,
        "warmup": args.warmup, "checks": checks, "shapes": shapes, "ms_median": ms,
        "ms_min": {name: float(min(values)) for name, values in times.items()},
        "ms_max": {name: float(max(values)) for name, values in times.items()},
        "decrypt_response_over_host_path": {name: ms[name + ".decrypt_response"] / ms[name + ".host_path"] for name in SHAPES},
        "find_over_copy": {name: ms[name] / ms[name.split(".")[0] + ".copy"] for name in ms if ".find_" in name},
        "generate_query_over_index_generate_query": ms["generate_query"] / ms["index_generate_query"],
    }
    line = json.dumps(result)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
