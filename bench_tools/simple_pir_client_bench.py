"""The SimplePIR client on the device (he_simple_pir_precompute_queries_device and the entries around it) over
32768 x 32768 elements, N = 1024, at 7 / 28 bits in 4-byte words and 14 / 42 bits in 8-byte words (one chunk per entry, 32 seeded
polynomials, a hint of 32768 x 1024 words).  One JSON line:

    python bench_tools/simple_pir_client_bench.py [--steps 30] [--warmup 3] [--queries 1024]

Per word size and batch B in 1, 16, 128: `precompute` and its two halves on resident secrets, `encrypt_zero` and
`secret_times_hint` (the three give the same words, checked before anything is timed).  The hint product is set against the
library's copy kernel on the hint's bytes (he_words_copy_device, read + write): `hint_read_over_copy` is the rate at which the
product's passes read the hint (ceil(B / 16) passes) over the copy's rate, `add_terms_per_s` counts B x column_size x N terms.
`host_ms_per_query` is the numpy path of tests/simple_pir_reference.Client for one query -- the two int64 products and the rounded
division -- timed on 1024 rows of each matrix and scaled to 32768, as DESIGN.md 4.6 scales its host figures.  `add_indices` and
`decrypt_responses` run on --queries queries.  The hint holds uniform words mod p: its values do not change the work.
Times are device events around the calls; medians over --steps with max / median beside them."""
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

N, SIDE = 1024, 32768
CONFIGS = [(7, 28, 32), (14, 42, 64)]
BATCHES = (1, 16, 128)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--steps", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--queries", type=int, default=1024)
    args = parser.parse_args()

    import torch

    import heamd
    import simple_pir_reference as R

    assert torch.cuda.is_available(), "simple_pir_client_bench.py measures on a GPU"
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def measure(calls):
        for _ in range(args.warmup):
            for run in calls.values():
                run()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(args.steps):
            for name, run in calls.items():
                begin.record()
                run()
                end.record()
                end.synchronize()
                times[name].append(begin.elapsed_time(end))
        return ({name: float(np.median(v)) for name, v in times.items()},
                {name: float(max(v) / np.median(v)) for name, v in times.items()})

    rng = np.random.default_rng(28)

    def seeds(*shape):
        return torch.from_numpy(rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)).cuda()

    results = []
    for pbits, cbits, word_bits in CONFIGS:
        params = heamd.simple_pir_shape(pbits, cbits, N, SIDE, SIDE * pbits // 8, word_bits)
        assert (params["column_size"], params["database_columns"], params["chunks_per_entry"], params["a_poly_count"]) == \
            (SIDE, SIDE, 1, SIDE // N)
        p, dtype = params["modulus"], torch.int64 if word_bits == 64 else torch.int32
        hint = torch.randint(0, p, (SIDE, N), dtype=torch.int64, device="cuda").to(dtype)
        client = heamd.SimplePirClient(params, hint, bytes(range(32)), word_bits)
        client.a_polynomials()
        ring = heamd.PolyContext(N, [p])
        hint_bytes = hint.numel() * hint.element_size()
        words = hint.view(torch.int64)
        copy_target = torch.empty_like(words)
        row = {"plaintext_bits": pbits, "ciphertext_bits": cbits, "word_bits": word_bits, "modulus": p, "hint_bytes": hint_bytes,
               "plan": client.plan(max(BATCHES)), "batches": {}}
        copy_ms, copy_spread = measure({"copy": lambda: heamd.stream_copy(words, copy_target)})
        copy_rate = 2 * hint_bytes / (copy_ms["copy"] / 1e3)
        row["copy"] = {"ms_median": copy_ms["copy"], "max_over_median": copy_spread["copy"], "bytes_per_s": copy_rate}
        for batch in BATCHES:
            secret_seeds, error_seeds = seeds(batch, 1), seeds(batch)
            # the secrets precompute draws from these seeds, resident for the two halves
            drawn = ring.random_ternary_from_seeds(secret_seeds.view(-1, 32), word=client._word).view(batch, 1, N).contiguous()
            spaces = {op: torch.empty(client.workspace_bytes(op, batch), dtype=torch.uint8, device="cuda")
                      for op in ("precompute", "encrypt_zero", "secret_times_hint")}
            calls = {
                "precompute": lambda: client.precompute(secret_seeds, error_seeds, workspace=spaces["precompute"]),
                "encrypt_zero": lambda: client.encrypt_zero(drawn, error_seeds, workspace=spaces["encrypt_zero"]),
                "secret_times_hint": lambda: client.secret_times_hint(drawn.view(batch, N), workspace=spaces["secret_times_hint"]),
            }
            queries, products = calls["precompute"]()
            same = bool(torch.equal(queries, calls["encrypt_zero"]())) and \
                bool(torch.equal(products.view(batch, SIDE), calls["secret_times_hint"]()))
            assert same, "precompute and its halves differ"
            ms, spread = measure(calls)
            passes = -(-batch // row["plan"]["secret_rows_per_pass"])
            seconds = ms["secret_times_hint"] / 1e3
            row["batches"][str(batch)] = {
                "ms_median": ms, "max_over_median": spread, "same_words": same, "passes": passes,
                "ms_per_query": ms["precompute"] / batch,
                "hint_read_bytes_per_s": passes * hint_bytes / seconds,
                "hint_read_over_copy": passes * hint_bytes / seconds / copy_rate,
                "add_terms_per_s": batch * SIDE * N / seconds,
                "workspace_bytes": {op: int(space.numel()) for op, space in spaces.items()},
            }
            del spaces, drawn
        # the host path of one query, on 1024 rows of each matrix
        host_rows = 1024
        secret = R.ternary_secrets(params, rng)
        rows = rng.integers(0, p, size=(host_rows, N), dtype=np.uint64)
        start = time.perf_counter()
        sample = R.secret_times_matrix(params, secret, rows)
        R.mod_switch(params, sample)
        R.secret_times_matrix(params, secret, rows)
        row["host_ms_per_query"] = (time.perf_counter() - start) * 1e3 * SIDE / host_rows
        row["host_rows_timed"] = host_rows
        # add(index:) and decrypt for many queries
        count = args.queries
        slab = torch.randint(0, 1 << cbits, (count, 1, SIDE), dtype=torch.int64, device="cuda").to(dtype)
        outcome = torch.randint(0, p, (count, 1, SIDE), dtype=torch.int64, device="cuda").to(dtype)
        indices = torch.from_numpy(rng.integers(0, SIDE, size=count, dtype=np.int64)).cuda()
        space = torch.empty(client.workspace_bytes("decrypt_responses", count), dtype=torch.uint8, device="cuda")
        ms, spread = measure({"add_indices": lambda: client.add_indices(slab, indices),
                              "decrypt_responses": lambda: client.decrypt(slab, outcome, indices, workspace=space)})
        row["per_index"] = {"queries": count, "ms_median": ms, "max_over_median": spread}
        results.append(row)
        del hint, words, copy_target, slab, outcome, client
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "simple_pir_client_bench", "lattice_dimension": N, "side": SIDE, "steps": args.steps,
                      "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "configs": results}))


if __name__ == "__main__":
    main()
