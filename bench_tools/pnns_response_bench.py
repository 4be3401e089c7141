"""Server.computeResponse for one-row queries on the device (heamd.PnnsContext.compute_response:
he_pnns_compute_response_device) at 2^20 rows x 128 columns, N = 8192, L = 4 x 55-bit moduli, a 20-bit t: b = 12, G = 11,
C = 128, a 4.3 GB matrix.  One JSON line, also written to --out:

    python bench_tools/pnns_response_bench.py [--queries 1,4] [--steps K] [--warmup W] [--no-composition] [--word32]
                                              [--stats Q=kernel_stats.csv ...] [--out profiles/pnns_response.json]

--word32: the same shape on a Bfv<UInt32> context (he_pnns_compute_response_device_u32), moduli as the 4-byte tests take them
(27, 28, 28 and 29 bits, a 17-bit t; a 1.6 GB matrix); the composition is of 8-byte entry points and is not run.

Per query count: the median of --steps calls by events around the enqueue-only call, per query.  The baseline, in the same
process: the same response of ONE query composed from the entry points the library had before (the sequence of
tests/test_gpu_pnns.py's mul_transpose_vector_device, its per-result loops batched as far as those entry points allow: per
giant step one gather of the step's plaintexts into the [columns][count] order he_bfv_inner_product_plain_resident_device
reads, one launch over the C results, one inverse NTT; the sum one batched key switch per step) and the mod-switch.  Times do
not depend on the words, so queries and keys are uniform words.  --stats Q=path (the kernel_stats.csv of a `rocprofv3
--kernel-trace --stats --output-format csv` run of this tool with --queries Q --no-composition, whose calls are --warmup +
--steps): every library kernel's time per call and the inner-product kernel's fraction of 8 TB/s on the matrix bytes."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd"), os.path.join(ROOT, "bench_tools")):
    if path not in sys.path:
        sys.path.insert(0, path)

DEGREE, ROWS, COLS, SCALE = 8192, 1 << 20, 128, 4096.0


def uniform(torch, moduli, before, seed, dtype=None):
    generator = torch.Generator("cuda").manual_seed(seed)
    rows = [torch.randint(0, int(m), tuple(before) + (DEGREE,), dtype=torch.int64, device="cuda", generator=generator)
            for m in moduli]
    return torch.stack(rows, dim=len(before)).to(dtype or torch.int64).contiguous()


def composition(heamd, torch, bfv, matrix, baby_step, giant_step, results, query, key_one, key_baby):
    ring = bfv.ciphertext_context()
    L = bfv.L
    element_one = heamd.galois_element_rotating_columns(-1, DEGREE)
    element_baby = heamd.galois_element_rotating_columns(-baby_step, DEGREE)
    states, state = [], query.reshape(1, 2, L, DEGREE)
    for step in range(baby_step):
        states.append(state)
        if step != baby_step - 1:
            state = bfv.apply_galois(state, element_one, key_one)
    rotated = ring.forward_ntt_(torch.cat(states).contiguous())
    dimension = COLS
    by_step = matrix.reshape(dimension, results, L, DEGREE)
    products = []
    for giant in range(giant_step):
        count = min(baby_step, dimension - baby_step * giant)
        plaintexts = by_step[baby_step * giant:baby_step * giant + count].transpose(0, 1).contiguous()  # [C][count][L][N]
        product = bfv.inner_product_plain_resident(rotated[:count].contiguous(), plaintexts, columns=results)
        products.append(ring.inverse_ntt_(product))
    accumulator = products.pop()
    for product in reversed(products):
        accumulator = bfv.apply_galois(accumulator.reshape(results, 2, L, DEGREE), element_baby, key_baby)
        accumulator = ring.add_(accumulator, product.reshape(results, 2, L, DEGREE))
    return bfv.mod_switch_down_to_single(accumulator, 2)


def timed(torch, steps, warmup, call):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(steps):
        begin.record()
        out = call()
        end.record()
        end.synchronize()
        times.append(begin.elapsed_time(end))
        del out
    return float(np.median(times)), times


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--queries", default="1,4")
    parser.add_argument("--steps", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--no-composition", action="store_true")
    parser.add_argument("--word32", action="store_true", help="Bfv<UInt32>: packed 4-byte words through the _u32 entry")
    parser.add_argument("--stats", action="append", default=[], help="Q=kernel_stats.csv of a traced run with --queries Q")
    parser.add_argument("--out")
    args = parser.parse_args()

    import torch

    import heamd
    from pnns_database_bench import kernels_per_call

    heamd.load_library().he_set_scratch_cache(2 ** 64 - 1)  # what a server sets once: the calls are enqueue-only
    if args.word32:
        import oracle

        t = oracle.generate_primes([17], True, DEGREE)[0]
        q = oracle.generate_primes([27, 28, 28, 29], False, DEGREE, word_bits=32)
        bfv = heamd.BfvContext32(DEGREE, t, q)
        args.no_composition = True
    else:
        t = heamd.generate_primes([20], False, DEGREE)[0]
        q = heamd.generate_primes([55] * 5, False, DEGREE)
        bfv = heamd.BfvContext(DEGREE, t, q)
    word = torch.int32 if args.word32 else torch.int64
    ctx = heamd.PnnsContext(bfv)
    L = bfv.L
    shape = ctx.matrix_shape(ROWS, COLS)
    baby_step, giant_step, results = shape["baby_step"], shape["giant_step"], ROWS // DEGREE
    vectors = torch.randn((ROWS, COLS), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    matrix, flag = ctx.process_database(vectors, SCALE)
    assert int(flag.item()) == 0
    del vectors
    matrix_bytes = matrix.numel() * matrix.element_size()
    properties = torch.cuda.get_device_properties(0)
    result = {"tool": "pnns_response_bench", "word_bits": 32 if args.word32 else 64, "degree": DEGREE, "L": L, "rows": ROWS, "cols": COLS, "baby_step": baby_step,
              "giant_step": giant_step, "result_ciphertexts": results, "matrix_bytes": matrix_bytes, "steps": args.steps,
              "device": properties.name, "clock_rate_khz": getattr(properties, "clock_rate", None),
              "compute_units": properties.multi_processor_count, "entry": {}}
    most = max(int(v) for v in args.queries.split(","))
    queries = uniform(torch, q[:L], (most, 2), 2, word)
    keys = [(uniform(torch, q, (L, 2), 10 + 2 * k, word), uniform(torch, q, (L, 2), 11 + 2 * k, word)) for k in range(most)]
    for count in (int(v) for v in args.queries.split(",")):
        ms, times = timed(torch, args.steps, args.warmup,
                          lambda: ctx.compute_response(matrix, ROWS, COLS, queries[:count].contiguous(), keys[:count]))
        result["entry"][str(count)] = {"ms_median": ms, "ms_per_query": ms / count, "ms_min": min(times), "ms_max": max(times)}
    if not args.no_composition:
        ms, times = timed(torch, args.steps, args.warmup,
                          lambda: composition(heamd, torch, bfv, matrix, baby_step, giant_step, results, queries[0],
                                              keys[0][0], keys[0][1]))
        result["composition_one_query"] = {"ms_median": ms, "ms_min": min(times), "ms_max": max(times)}
        got = ctx.compute_response(matrix, ROWS, COLS, queries[:1].contiguous(), keys[:1])
        same = composition(heamd, torch, bfv, matrix, baby_step, giant_step, results, queries[0], keys[0][0], keys[0][1])
        result["composition_equals_entry"] = bool(torch.equal(got.reshape(-1), same.reshape(-1)))
        if "1" in result["entry"]:
            result["composition_over_entry_one_query"] = ms / result["entry"]["1"]["ms_median"]
    for item in args.stats:
        count, path = item.split("=", 1)
        per_kernel = kernels_per_call(path, args.steps + args.warmup)
        inner = sum(v for k, v in per_kernel.items() if k.startswith("pnns_bsgs_inner_product_kernel"))
        result.setdefault("kernels", {})[count] = {
            "kernel_ms_per_call": sum(per_kernel.values()), "kernels_ms_per_call": per_kernel,
            "inner_product_ms_per_call": inner,
            "inner_product_fraction_of_8TBps_on_matrix_bytes": matrix_bytes / (inner / 1e3) / 8e12 if inner else None}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
