"""SimplePIR over sharded databases on the device: DatabaseMap.shardDatabase as he_simple_pir_shard_map_device +
he_simple_pir_shard_scatter_device, and SimplePirClientForAllShards' assembly as he_simple_pir_shard_assemble_device.

    python bench_tools/simple_pir_shard_bench.py [--count N] [--host-count N] [--windows W] [--calls C] [--out FILE]

Values of 1024 .. 4096 random bytes (2^20 of them unless --count says otherwise) into 5 shards, at two chunk sizes: 820, what SimplePIRProcessDatabase computes for this
database (ceil(4096 / 5); not a multiple of 8, so the scatter runs its byte form), and 832, the next multiple of 16 (the 16-byte
form).  One JSON line per chunk size (and, with --out, a JSON file of all): the median over W windows of C calls each, device
events around a window.
    map_ms, scatter_ms   the two entries alone; split_ms both, as a caller issues them
    scatter_GBps         (value bytes read + slab bytes written) / scatter_ms, set against he_words_copy_device moving the same
                         number of bytes in the same run (words_copy_GBps)
    host_path_ms         at --host-count values, wall time of the path the entries replace: the values to the host, the split in
                         numpy (a Python loop over the chunks with the same orders), the shards back up; device_split_ms_at_host_
                         count is the device path on the same values, whose slab must equal the host's byte for byte
    assemble_ms          1024 lookups; assemble_host_ms: the decrypted chunks and the index lists to the host and the entries
                         stitched there in numpy (wall time)."""
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

SHARDS, LARGEST, LOOKUPS = 5, 4096, 1024


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


class Database:
    def __init__(self, count, chunk_size, seed=1):
        import heamd
        import torch

        rng = np.random.default_rng(seed)
        self.count, self.chunk_size = count, chunk_size
        self.lengths = rng.integers(1024, LARGEST + 1, size=count, dtype=np.int64)
        self.offsets = np.concatenate(([0], np.cumsum(self.lengths))).astype(np.uint64)
        self.orders = np.argsort(rng.random((count, SHARDS)), axis=1).astype(np.uint8)
        generator = torch.Generator(device="cuda").manual_seed(seed)
        self.values = torch.randint(0, 256, (int(self.offsets[-1]),), dtype=torch.uint8, device="cuda", generator=generator)
        self.plan = heamd.simple_pir_shard_plan(self.offsets, SHARDS, chunk_size)
        total = self.total = self.plan["total_chunks"]
        self.offsets_device = heamd.to_device(self.offsets)
        self.orders_device = torch.from_numpy(self.orders).cuda()
        words = lambda n, dtype: torch.empty((n,), dtype=dtype, device="cuda")  # noqa: E731
        self.chunk_starts, self.row_starts = words(count + 1, torch.int64), words(SHARDS + 1, torch.int64)
        self.chunk_shard, self.chunk_index, self.row_chunk = (words(total, torch.int32) for _ in range(3))
        self.slab = words(total * chunk_size, torch.uint8)
        self.plan = heamd.simple_pir_shard_plan(self.offsets, SHARDS, chunk_size, self.slab.data_ptr())
        self.lib = heamd.load_library()

    def map(self):
        from heamd.binding import _check, vp

        p = lambda tensor: vp(tensor.data_ptr())  # noqa: E731
        _check(self.lib.he_simple_pir_shard_map_device(
            p(self.offsets_device), p(self.orders_device), self.count, SHARDS, self.chunk_size, self.total, p(self.chunk_starts),
            p(self.chunk_shard), p(self.chunk_index), p(self.row_starts), p(self.row_chunk), None, None))

    def scatter(self):
        from heamd.binding import _check, vp

        p = lambda tensor: vp(tensor.data_ptr())  # noqa: E731
        _check(self.lib.he_simple_pir_shard_scatter_device(
            p(self.values), self.values.numel(), p(self.offsets_device), self.count, self.chunk_size, self.total,
            p(self.chunk_starts), p(self.row_chunk), p(self.slab), None))

    def split(self):
        self.map()
        self.scatter()

    def host_split(self):
        """the path the entries replace: download, split in numpy with the same orders, upload -> (ms, slab on the host)"""
        import torch

        torch.cuda.synchronize()
        start = time.perf_counter()
        blob = self.values.cpu().numpy()
        S, C = SHARDS, self.chunk_size
        chunks = -(-self.lengths // C)
        position = np.argsort(self.orders, axis=1)  # order^-1
        given = chunks[:, None] // S + (position < (chunks % S)[:, None])  # rows entry e gives shard s
        base = np.cumsum(given, axis=0) - given
        shard_start = np.concatenate(([0], np.cumsum(given.sum(axis=0))))
        slab = np.zeros((int(shard_start[-1]), C), dtype=np.uint8)
        offsets = self.offsets.astype(np.int64)
        for e in range(self.count):
            order, begin, end = self.orders[e], offsets[e], offsets[e + 1]
            for k in range(int(chunks[e])):
                shard = order[k % S]
                piece = blob[begin + k * C: min(begin + (k + 1) * C, end)]
                slab[shard_start[shard] + base[e, shard] + k // S, :piece.size] = piece
        device = torch.from_numpy(slab).cuda()
        torch.cuda.synchronize()
        return (time.perf_counter() - start) * 1e3, slab, device


def run(count, host_count, chunk_size, windows, calls):
    import heamd
    import torch
    from heamd.binding import _check, vp

    result = {"tool": "simple_pir_shard_bench", "values": count, "shard_count": SHARDS, "chunk_size": chunk_size,
              "windows": windows, "calls_per_window": calls}
    small = Database(host_count, chunk_size)
    small.split()
    host_ms, host_slab, _ = small.host_split()
    assert np.array_equal(small.slab.cpu().numpy().reshape(-1, chunk_size), host_slab), "the device slab differs from the host's"
    result.update(host_count=host_count, host_path_ms=host_ms, host_value_bytes=small.values.numel(),
                  device_split_ms_at_host_count=median_ms(small.split, windows, calls))

    # the assembly, on the small database's map: decrypted chunks are the shard rows the index lists ask for
    rng = np.random.default_rng(2)
    plan = small.plan
    M, per_shard = plan["maximum_chunk_count"], plan["chunks_per_shard"]
    lookups = rng.integers(0, host_count + host_count // 8, size=LOOKUPS)  # one in nine is absent
    positions = heamd.to_device(lookups.astype(np.uint64))
    indices = torch.empty((SHARDS, LOOKUPS, per_shard), dtype=torch.int64, device="cuda")
    found = torch.empty((LOOKUPS,), dtype=torch.int32, device="cuda")
    p = lambda tensor: vp(tensor.data_ptr())  # noqa: E731
    _check(small.lib.he_simple_pir_shard_query_indices_device(
        p(positions), LOOKUPS, host_count, SHARDS, small.total, M, per_shard, p(small.chunk_starts), p(small.chunk_shard),
        p(small.chunk_index), p(indices), p(found), None))
    rows = small.row_starts[:SHARDS].reshape(SHARDS, 1, 1) + indices  # slab row of every query slot
    chunks = small.slab.reshape(-1, chunk_size)[rows.reshape(-1)].reshape(SHARDS, LOOKUPS, per_shard, chunk_size).contiguous()
    entries = torch.empty((LOOKUPS, M * chunk_size), dtype=torch.uint8, device="cuda")
    sizes = torch.empty((LOOKUPS,), dtype=torch.int64, device="cuda")

    def assemble():
        _check(small.lib.he_simple_pir_shard_assemble_device(
            p(chunks), p(indices), p(positions), LOOKUPS, p(small.offsets_device), host_count, SHARDS, chunk_size, small.total, M,
            per_shard, p(small.chunk_starts), p(small.chunk_shard), p(small.chunk_index), p(entries), p(sizes), p(found), None))

    result["assemble_ms"] = median_ms(assemble, windows, max(calls, 20))
    blob, offsets = small.values.cpu().numpy(), small.offsets.astype(np.int64)
    got, got_sizes = entries.cpu().numpy(), sizes.cpu().numpy()
    for b in range(0, LOOKUPS, 37):
        e = int(lookups[b])
        value = blob[offsets[e]:offsets[e + 1]] if e < host_count else blob[:0]
        assert got_sizes[b] == value.size and np.array_equal(got[b, :value.size], value) and not got[b, value.size:].any(), b
    chunk_starts, chunk_shard = small.chunk_starts.cpu().numpy(), small.chunk_shard.cpu().numpy()
    chunk_index = small.chunk_index.cpu().numpy()
    torch.cuda.synchronize()
    start = time.perf_counter()
    host_chunks, host_indices = chunks.cpu().numpy(), indices.cpu().numpy()
    for b in range(LOOKUPS):  # the reference's stitching, on the host
        e = int(lookups[b])
        out = np.zeros(M * chunk_size, dtype=np.uint8)
        if e < host_count:
            for k in range(int(chunk_starts[e + 1] - chunk_starts[e])):
                shard, target = chunk_shard[chunk_starts[e] + k], chunk_index[chunk_starts[e] + k]
                slot = int(np.flatnonzero(host_indices[shard, b] == target)[-1])
                out[k * chunk_size:(k + 1) * chunk_size] = host_chunks[shard, b, slot]
    result["assemble_host_ms"] = (time.perf_counter() - start) * 1e3
    del small, chunks, entries

    big = Database(count, chunk_size) if count != host_count else Database(host_count, chunk_size)
    result["plan"] = big.plan
    result["value_bytes"] = big.values.numel()
    result["slab_bytes"] = big.slab.numel()
    big.map()
    result["map_ms"] = median_ms(big.map, windows, calls)
    result["scatter_ms"] = median_ms(big.scatter, windows, calls)
    result["split_ms"] = median_ms(big.split, windows, calls)
    moved = big.values.numel() + big.slab.numel()
    words = moved // 16  # a copy reads and writes every word: `moved` bytes in all
    source = torch.empty((words,), dtype=torch.int64, device="cuda")
    target = torch.empty_like(source)
    copy_ms = median_ms(lambda: heamd.stream_copy(source, target), windows, calls)
    result.update(scatter_bytes_moved=moved, scatter_GBps=moved / result["scatter_ms"] / 1e6, words_copy_ms=copy_ms,
                  words_copy_GBps=words * 16 / copy_ms / 1e6)
    result["scatter_over_words_copy"] = result["scatter_GBps"] / result["words_copy_GBps"]
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--count", type=int, default=1 << 20)
    parser.add_argument("--host-count", type=int, default=1 << 16)
    parser.add_argument("--chunk-size", type=int, action="append")
    parser.add_argument("--windows", type=int, default=5)
    parser.add_argument("--calls", type=int, default=3)
    parser.add_argument("--out")
    args = parser.parse_args()
    results = []
    for chunk_size in args.chunk_size or [-(-LARGEST // SHARDS), 832]:
        results.append(run(args.count, args.host_count, chunk_size, args.windows, args.calls))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
