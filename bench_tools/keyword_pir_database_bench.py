"""KeywordPirServer.process on the device, stage by stage, at the two shapes the reference documents:

    small   100 000 x 2-byte values on n_4096_logq_27_28_28_logt_4  (4-byte words)
    large   1000 x 60 kB values on n_8192_logq_3x55_logt_24         (the value bytes dominate)

    python bench_tools/keyword_pir_database_bench.py [--shape small|large] [--windows W] [--calls C] [--out FILE]

One JSON line per shape (and, with --out, a JSON file of both): the median over W windows of C calls each, events around a
window, for the keyword hash, the candidate indices, the bucket serialization and the index-PIR build of all sub-tables; wall
time of the host placement (all passes, expansions included); and the serialize kernel's read-plus-written bytes over its time
against he_words_copy_device moving the same number of bytes in the same run.  CuckooTableConfig.defaultKeywordPir with
defaultMaxSerializedBucketSize, two dimensions."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd")):
    if path not in sys.path:
        sys.path.insert(0, path)

SHAPES = {  # name: (degree, coefficient moduli or their bit counts, plaintext modulus bits, word bits, entries, value bytes)
    "small": (4096, [(1 << 27) - 40959, (1 << 28) - 65535, (1 << 28) - 73727], 5, 32, 100_000, 2),
    "large": (8192, [55, 55, 55], 25, 64, 1000, 60_000),
}


def median_ms(call, windows, calls):
    import torch

    call()
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(windows):
        begin.record()
        for _ in range(calls):
            call()
        end.record()
        end.synchronize()
        times.append(begin.elapsed_time(end) / calls)
    return float(np.median(times))


def run(name, windows, calls):
    import heamd
    import torch

    degree, moduli, t_bits, word_bits, count, value_bytes = SHAPES[name]
    t = heamd.generate_primes([t_bits], True, 1)[0]
    q = moduli if moduli[0] > 64 else heamd.generate_primes(moduli, False, degree)
    ctx = (heamd.BfvContext32 if word_bits == 32 else heamd.BfvContext)(degree, t, q)
    bytes_per_plaintext = degree * (t.bit_length() - 1) // 8
    single = 1 + 10 + value_bytes  # CuckooTableConfig.defaultMaxSerializedBucketSize (CuckooTable.swift:109-118)
    limit = -(-single // bytes_per_plaintext) * bytes_per_plaintext if single >= bytes_per_plaintext // 2 \
        else bytes_per_plaintext // 2
    config = heamd.CuckooTableConfig(2, 100, limit)
    rng = np.random.default_rng(1)
    keywords = [rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() for n in rng.integers(8, 17, size=count)]
    keywords = list(dict.fromkeys(keywords))
    count = len(keywords)
    values = [rng.integers(0, 256, size=value_bytes, dtype=np.uint8).tobytes() for _ in range(count)]
    keyword_blob, keyword_offsets = heamd.binding._blob(keywords, "cuda")
    offsets_device = heamd.to_device(keyword_offsets)
    result = {"tool": "keyword_pir_database_bench", "shape": name, "degree": degree, "word_bits": word_bits, "entries": count,
              "value_bytes": value_bytes, "max_serialized_bucket_size": limit, "windows": windows, "calls_per_window": calls}

    result["hash_ms"] = median_ms(lambda: heamd.keyword_pir_hash_keywords(keyword_blob, offsets_device), windows, calls)
    hashes = heamd.keyword_pir_hash_keywords(keyword_blob, offsets_device)
    sizes = [value_bytes] * count
    bucket_count = heamd.keyword_pir_bucket_count(config, sizes)
    result["indices_ms"] = median_ms(lambda: heamd.keyword_pir_hash_indices(hashes, bucket_count // 2, 2), windows, calls)

    host_hashes = heamd.to_host(hashes)
    start, passes = time.perf_counter(), 0
    while True:  # what he_keyword_pir_table_create_device does between the kernels
        indices = heamd.keyword_pir_hash_indices(hashes, bucket_count // 2, 2).cpu().numpy().view(np.uint32)
        placed = heamd.keyword_pir_cuckoo_place(config, host_hashes, indices, sizes, bucket_count, 1)
        passes += 1
        if placed["status"] == "ok":
            break
        bucket_count = placed["next_bucket_count"]
    result.update(placement_ms=(time.perf_counter() - start) * 1e3, placement_passes=passes, bucket_count=bucket_count)

    start = time.perf_counter()
    table = heamd.KeywordPirTable(config, keywords, values, seed=1)
    torch.cuda.synchronize()
    result["table_create_ms_with_upload"] = (time.perf_counter() - start) * 1e3
    assert table.bucket_count == bucket_count and table.entry_count == count
    entry_size = table.largest_bucket_size
    per_table = table.buckets_per_table
    out = torch.empty((bucket_count, entry_size), dtype=torch.uint8, device="cuda")
    result["serialize_ms"] = median_ms(lambda: table.entries(entry_size, out=out), windows, calls)
    # the values, 8 bytes of hash and 8 of offset per slot, 4 per slot start written and read, the CSR pair, and the rows
    moved = count * value_bytes + count * (8 + 8 + 4 + 4 + 4) + 4 * (bucket_count + 1) + out.numel()
    words = moved // 16  # a copy reads and writes every word: `moved` bytes in all
    source = torch.empty((words,), dtype=torch.int64, device="cuda")
    target = torch.empty_like(source)
    copy_ms = median_ms(lambda: heamd.stream_copy(source, target), windows, calls)
    result.update(entry_size_in_bytes=entry_size, serialize_bytes_moved=moved, serialize_GBps=moved / result["serialize_ms"] / 1e6,
                  words_copy_ms=copy_ms, words_copy_GBps=words * 16 / copy_ms / 1e6)
    result["serialize_over_words_copy"] = result["serialize_GBps"] / result["words_copy_GBps"]

    shape = None
    side = math.isqrt(per_table)
    for d0 in range(max(side, 1), per_table + 2):  # two dimensions that hold a sub-table
        dims = [d0, -(-per_table // d0)]
        try:
            shape = ctx.pir_database_shape(dims, per_table, entry_size, False)
            break
        except heamd.HeError:
            continue
    sub_tables = [out[t * per_table:(t + 1) * per_table] for t in range(table.table_count)]
    slots = shape["chunk_count"] * shape["plaintexts_per_chunk"]
    targets = [(heamd.binding._empty((slots, ctx.L, degree), ctx._word, "cuda"),
                torch.empty((slots,), dtype=torch.uint8, device="cuda")) for _ in sub_tables]

    def build():
        for entries, target_pair in zip(sub_tables, targets):
            ctx.pir_process_database(entries, dims, entry_size, False, out=target_pair)

    result["index_pir_build_ms"] = median_ms(build, max(windows // 2, 1), 1)
    result["process_database_ms"] = median_ms(lambda: table.process_database(ctx, dims, entry_size), max(windows // 2, 1), 1)
    result.update(dimensions=dims, chunk_count=shape["chunk_count"], plaintexts=slots * table.table_count,
                  load_factor=float(table.load_factor), expansions=table.expansion_count)
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shape", choices=sorted(SHAPES))
    parser.add_argument("--windows", type=int, default=7)
    parser.add_argument("--calls", type=int, default=5)
    parser.add_argument("--out")
    args = parser.parse_args()
    results = []
    for name in ([args.shape] if args.shape else ["small", "large"]):
        results.append(run(name, args.windows, args.calls))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
