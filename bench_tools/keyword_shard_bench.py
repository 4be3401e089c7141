"""KeywordDatabase.init on the device: he_keyword_database_partition_device, stage by stage, at the two shapes
of keyword_pir_database_bench.py and one that does not fit the Infinity Cache:

    small   100 000 x (16-byte keyword, 2-byte value), 64 shards
    large   1000 x (16-byte keyword, 60 kB value), 8 shards
    rows    4 194 304 x (16-byte keyword, 32-byte value), 1024 shards   (about 200 MB read and 200 MB written)

    python bench_tools/keyword_shard_bench.py [--shape small|large|rows] [--windows W] [--calls C] [--out FILE]

One JSON line per shape (and, with --out, a JSON file of all): the median over W windows of C calls each, events around a
window.  The entry is one call, so the stages are differences of calls that leave a stage out:
    whole      the call as it is
    no_gather  the same call with both blob sizes claimed as 0: the order passes, the shard starts, both offset scans
    one_shard  no_gather with one shard: no order pass -- the identity order, the lengths and both offset scans
    order_ms = no_gather - one_shard, offsets_ms = one_shard, gather_ms = whole - no_gather
(one_shard reads the offsets in input order where no_gather reads them through the order; the difference is charged to the
order passes.)  The gather's read-plus-written bytes over gather_ms are set against he_words_copy_device moving the same number
of bytes in the same run.  host_path_ms is the caller's former path, as wall time: the indices to the host, a numpy stable
argsort, a fancy-index gather of both blobs and their upload."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd")):
    if path not in sys.path:
        sys.path.insert(0, path)

SHAPES = {  # name: (rows, keyword bytes, value bytes, shards)
    "small": (100_000, 16, 2, 64),
    "large": (1000, 16, 60_000, 8),
    "rows": (1 << 22, 16, 32, 1024),
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
    from heamd.binding import _check, vp

    count, key_size, value_size, shard_count = SHAPES[name]
    rng = np.random.default_rng(1)
    keywords_host = rng.integers(0, 256, size=(count, key_size), dtype=np.uint8)
    values_host = rng.integers(0, 256, size=(count, value_size), dtype=np.uint8)
    keywords, values = torch.from_numpy(keywords_host).cuda().reshape(-1), torch.from_numpy(values_host).cuda().reshape(-1)
    key_offsets = heamd.to_device(np.arange(count + 1, dtype=np.uint64) * key_size)
    value_offsets = heamd.to_device(np.arange(count + 1, dtype=np.uint64) * value_size)
    indices = heamd.keyword_pir_shard_indices(heamd.keyword_pir_hash_keywords(keywords, key_offsets), shard_count)
    key_bytes, value_bytes = keywords.numel(), values.numel()
    out = {"keywords": torch.empty_like(keywords), "values": torch.empty_like(values),
           "key_offsets": torch.empty_like(key_offsets), "value_offsets": torch.empty_like(value_offsets),
           "order": torch.empty((count,), dtype=torch.int32, device="cuda"),
           "starts": torch.empty((shard_count + 1,), dtype=torch.int32, device="cuda")}
    lib = heamd.load_library()

    def partition(shards, claimed_key_bytes, claimed_value_bytes):
        _check(lib.he_keyword_database_partition_device(
            vp(keywords.data_ptr()), vp(key_offsets.data_ptr()), claimed_key_bytes, vp(values.data_ptr()),
            vp(value_offsets.data_ptr()), claimed_value_bytes, count, vp(indices.data_ptr()), shards,
            vp(out["keywords"].data_ptr()), vp(out["key_offsets"].data_ptr()), vp(out["values"].data_ptr()),
            vp(out["value_offsets"].data_ptr()), vp(out["order"].data_ptr()), vp(out["starts"].data_ptr()), None, None))

    plan = heamd.keyword_pir_partition_plan(count, shard_count, key_bytes, value_bytes)
    result = {"tool": "keyword_shard_bench", "shape": name, "rows": count, "keyword_bytes": key_size, "value_bytes": value_size,
              "shard_count": shard_count, "windows": windows, "calls_per_window": calls, "plan": plan}
    whole = median_ms(lambda: partition(shard_count, key_bytes, value_bytes), windows, calls)
    # the result of the whole call, checked against numpy before anything is timed further
    order = np.argsort(indices.cpu().numpy().view(np.uint32), kind="stable")
    assert np.array_equal(out["order"].cpu().numpy().view(np.uint32), order.astype(np.uint32))
    assert np.array_equal(out["values"].cpu().numpy().reshape(count, value_size), values_host[order])
    assert np.array_equal(out["keywords"].cpu().numpy().reshape(count, key_size), keywords_host[order])
    no_gather = median_ms(lambda: partition(shard_count, 0, 0), windows, calls)
    one_shard = median_ms(lambda: partition(1, 0, 0), windows, calls)
    gather = whole - no_gather
    # the gather reads and writes every blob byte, and reads both offset arrays and the order
    moved = 2 * (key_bytes + value_bytes) + 2 * (2 * 8 * (count + 1) + 4 * count)
    words = moved // 16  # a copy reads and writes every word: `moved` bytes in all
    source = torch.empty((words,), dtype=torch.int64, device="cuda")
    target = torch.empty_like(source)
    copy_ms = median_ms(lambda: heamd.stream_copy(source, target), windows, calls)
    result.update(whole_ms=whole, order_ms=no_gather - one_shard, offsets_ms=one_shard, gather_ms=gather,
                  gather_bytes_moved=moved, gather_GBps=moved / gather / 1e6, words_copy_ms=copy_ms,
                  words_copy_GBps=words * 16 / copy_ms / 1e6)
    result["gather_over_words_copy"] = result["gather_GBps"] / result["words_copy_GBps"]
    result["whole_GBps"] = moved / whole / 1e6

    times = []
    for _ in range(3):  # the caller's former path
        torch.cuda.synchronize()
        start = time.perf_counter()
        host_indices = indices.cpu().numpy().view(np.uint32)
        host_order = np.argsort(host_indices, kind="stable")
        sorted_keywords = torch.from_numpy(keywords_host[host_order]).cuda()
        sorted_values = torch.from_numpy(values_host[host_order]).cuda()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - start) * 1e3)
        del sorted_keywords, sorted_values
    result["host_path_ms"] = float(np.median(times))
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shape", choices=sorted(SHAPES))
    parser.add_argument("--windows", type=int, default=7)
    parser.add_argument("--calls", type=int, default=5)
    parser.add_argument("--out")
    args = parser.parse_args()
    results = []
    for name in ([args.shape] if args.shape else ["small", "large", "rows"]):
        results.append(run(name, args.windows, args.calls))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
