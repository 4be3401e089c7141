"""SimplePirServer.compute_response_batch (the int8 matrix kernel) beside compute_response (the existing reply kernel, the
yardstick) in one run, over a square database of random elements below 2^plaintext_bits built on the device.  One JSON line:

    python bench_tools/simple_pir_batch_bench.py [--config big-u32|big-u64|all] [--side 32768] [--queries 1,4,8,16,32,64]
                                                 [--steps 30] [--warmup 10]

Per configuration and query_count: the median and max / median of --steps calls of each entry timed by events after --warmup
calls, the batch entry's passes over the database, its stored bytes per second per pass and their fraction of 8 TB/s, and
existing / batch.  The two entries' words are compared on every query_count.  `copy_ms` is the library's copy kernel moving
the database's stored bytes once (read and write): the floor to quote beside one read of the database."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd")):
    if path not in sys.path:
        sys.path.insert(0, path)

from simple_pir_bench import timed  # noqa: E402

CONFIGS = {"big-u32": (7, 28, 32), "big-u64": (14, 42, 64)}  # name: (plaintext_bits, ciphertext_bits, word_bits)


def run(name, side, queries, steps, warmup):
    import torch

    import heamd

    pbits, cbits, word_bits = CONFIGS[name]
    element_bytes = 1 if pbits <= 8 else 2
    generator = torch.Generator(device="cuda").manual_seed(1)
    database = torch.randint(0, 1 << pbits, (side, side), device="cuda", generator=generator,
                             dtype=torch.uint8 if element_bytes == 1 else torch.int16)
    params = dict(plaintext_bits=pbits, ciphertext_bits=cbits, column_size=side, database_columns=side,
                  element_bytes=element_bytes)
    server = (heamd.SimplePirServer if word_bits == 64 else heamd.SimplePirServer32)(database, None, params)
    stored = side * side * element_bytes
    plan = heamd.simple_pir_batch_plan(pbits, cbits, side, max(queries), word_bits)
    words = database.view(-1).view(torch.int64)  # stream_copy counts 8-byte words
    assert words.numel() * 8 == stored
    spare = torch.empty_like(words)
    copy_ms, copy_spread = timed(lambda: heamd.stream_copy(words, spare), steps, warmup)
    del spare
    out = {"config": name, "plaintext_bits": pbits, "ciphertext_bits": cbits, "word_bits": word_bits, "column_size": side,
           "database_columns": side, "element_bytes": element_bytes, "database_bytes_stored": stored, "plan": plan,
           "copy_ms": copy_ms, "copy_max_over_median": copy_spread, "copy_GBps_read_plus_write": 2 * stored / copy_ms / 1e6,
           "replies": {}}
    rng = np.random.default_rng(2)
    to_device = heamd.to_device if word_bits == 64 else heamd.to_device32
    for q in queries:
        requests = to_device(rng.integers(0, 1 << cbits, size=(q, side), dtype=np.uint64))
        assert torch.equal(server.compute_response_batch(requests), server.compute_response(requests))
        batch_ms, batch_spread = timed(lambda: server.compute_response_batch(requests), steps, warmup)
        existing_ms, existing_spread = timed(lambda: server.compute_response(requests), steps, warmup)
        passes = -(-q // plan["requests_per_pass"])
        out["replies"][str(q)] = {
            "batch": {"ms_median": batch_ms, "max_over_median": batch_spread, "passes": passes,
                      "GBps_per_pass": passes * stored / batch_ms / 1e6,
                      "fraction_of_8TBps_per_pass": passes * stored / (batch_ms / 1e3) / 8e12},
            "existing": {"ms_median": existing_ms, "max_over_median": existing_spread, "passes": -(-q // 8)},
            "existing_over_batch": existing_ms / batch_ms}
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", default="all", choices=sorted(CONFIGS) + ["all"])
    parser.add_argument("--side", type=int, default=32768)
    parser.add_argument("--queries", default="1,4,8,16,32,64")
    parser.add_argument("--steps", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=10)
    args = parser.parse_args()
    names = sorted(CONFIGS) if args.config == "all" else [args.config]
    queries = [int(q) for q in args.queries.split(",")]
    print(json.dumps({"tool": "simple_pir_batch_bench", "steps": args.steps, "warmup": args.warmup,
                      "configs": [run(name, args.side, queries, args.steps, args.warmup) for name in names]}))


if __name__ == "__main__":
    main()
