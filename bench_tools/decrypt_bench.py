"""Decryption of resident ciphertexts (he_bfv_decrypt_device, he_bfv_noise_norm_device, he_bfv_is_transparent_device) at the
PIR benchmark's ring: N = 8192, L = 4 x 55-bit moduli, a 17-bit t, 1024 Coeff-form ciphertexts of two polynomials.  One JSON
line:

    python bench_tools/decrypt_bench.py [--batch B] [--steps K] [--warmup W] [--stats kernel_stats.csv]

In one run, alternating per step: `decrypt` against the composition of the entries that existed before it and yield the same
words -- forward NTT, he_poly_mul (c1 *= s), he_poly_add (c0 += c1), inverse NTT, he_rns_scale_and_round_device -- which is
timed twice: in place on slabs it may destroy (c0 and c1 already split into two contiguous slabs and the key replicated per
ciphertext, both outside the timed window), and with the copy that keeps the caller's ciphertexts as `decrypt` does (its
slab is const).  The words of the two are compared before anything is timed.  `noise_norm`, `is_transparent` and a streaming
copy of the ciphertext slab (the copy rate the kernels are held against) are timed on their own.  Times are device events
around each call, medians over --steps.

--stats: the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats --output-format csv` run of this tool alone: the time
per launch of the kernels of decrypt_kernels.hip, the bytes each moves and that rate over the copy rate of this run."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd")):
    if path not in sys.path:
        sys.path.insert(0, path)

DEGREE, MODULI = 8192, 4
KERNELS = ("secret_dot_product_kernel", "add_first_polynomial_kernel", "noise_norm_kernel", "is_transparent_kernel")


def kernel_ns_per_launch(stats_path):
    """{kernel: ns per launch} of the kernels of decrypt_kernels.hip in a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(stats_path) as f:
        for row in csv.DictReader(f):
            for kernel in KERNELS:
                if kernel in row["Name"]:
                    out[kernel] = float(row["TotalDurationNs"]) / max(int(float(row["Calls"])), 1)
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--batch", type=int, default=1024)
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    args = parser.parse_args()

    import torch

    import heamd

    assert torch.cuda.is_available(), "decrypt_bench.py measures on a GPU"
    batch, n, L = args.batch, DEGREE, MODULI
    t = heamd.generate_primes([17], True, n)[0]
    q = heamd.generate_primes([55] * (L + 1), False, n)
    ctx = heamd.BfvContext(n, t, q)
    poly = ctx.ciphertext_context()
    rng = np.random.default_rng(5)

    def uniform(prefix, moduli):
        rows = [rng.integers(0, m, size=tuple(prefix) + (n,), dtype=np.uint64) for m in moduli]
        return heamd.to_device(np.ascontiguousarray(np.stack(rows, axis=len(prefix))))

    cts = uniform((batch, 2), q[:L])  # [batch][2][L][N] Coeff
    key = uniform((), q)  # [L + 1][N] Eval
    # what the composition is handed: the polynomials split, the key once per ciphertext
    split = torch.stack([cts[:, 0], cts[:, 1]]).contiguous()  # [2][batch][L][N]
    key_per_ciphertext = key[:L].unsqueeze(0).expand(batch, L, n).contiguous()
    work = torch.empty_like(split)
    copy_target = torch.empty_like(cts)

    def composition(slabs):
        poly.forward_ntt_(slabs)
        poly.mul_(slabs[1], key_per_ciphertext)
        poly.add_(slabs[0], slabs[1])
        poly.inverse_ntt_(slabs[0])
        return ctx.scale_and_round(slabs[0])

    def composition_preserving():
        work.copy_(split)
        return composition(work)

    def composition_in_place():  # (any canonical words time alike: the slab is not restored between steps)
        return composition(work)

    workspace = torch.empty(ctx.decrypt_workspace_bytes(batch), dtype=torch.uint8, device="cuda")
    variants = {
        "decrypt": lambda: ctx.decrypt(cts, key, workspace=workspace),
        "composition_preserving": composition_preserving,
        "composition_in_place": composition_in_place,
        "noise_norm": lambda: ctx.noise_norm_device(cts, key, workspace=workspace),
        "is_transparent": lambda: ctx.is_transparent(cts),
        "stream_copy": lambda: heamd.stream_copy(cts, copy_target),
    }
    same = bool(torch.equal(variants["decrypt"](), composition_preserving()))
    assert same, "decrypt and the composition of the earlier entries differ"
    for _ in range(args.warmup):
        for run in variants.values():
            run()
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in variants}
    for _ in range(args.steps):
        for name, run in variants.items():  # alternating, so that a drift of the clock reaches every variant alike
            begin.record()
            run()
            end.record()
            end.synchronize()
            times[name].append(begin.elapsed_time(end))
    ms = {name: float(np.median(values)) for name, values in times.items()}
    slab_bytes = cts.numel() * 8
    copy_rate = 2 * slab_bytes / (ms["stream_copy"] / 1e3)
    poly_bytes = batch * L * n * 8
    moved = {  # bytes each kernel of decrypt_kernels.hip moves at this shape
        "secret_dot_product_kernel": 2 * poly_bytes + L * n * 8,  # Coeff input: c1 (Eval) in, c1 s out, the key once
        "add_first_polynomial_kernel": 3 * poly_bytes,  # c0 and the inverse transform's rows in, the dot product out
        "noise_norm_kernel": poly_bytes + batch * ctx.noise_norm_limbs() * 8,
        "is_transparent_kernel": poly_bytes + batch,
    }
    result = {"tool": "decrypt_bench", "degree": n, "L": L, "t_bits": 17, "batch": batch, "poly_count": 2, "form": "Coeff",
              "steps": args.steps, "warmup": args.warmup, "same_words": same, "ms_median": ms,
              "ms_min": {name: float(min(values)) for name, values in times.items()},
              "ms_max": {name: float(max(values)) for name, values in times.items()},
              "decrypt_over_composition_preserving": ms["decrypt"] / ms["composition_preserving"],
              "decrypt_over_composition_in_place": ms["decrypt"] / ms["composition_in_place"],
              "ciphertexts_per_s": batch / (ms["decrypt"] / 1e3), "slab_bytes": slab_bytes,
              "copy_rate_bytes_per_s": copy_rate, "kernel_bytes_moved": moved,
              # (one kernel is the whole call; the other two calls also transform: --stats has their kernels' own times)
              "is_transparent_call_fraction_of_copy_rate":
              moved["is_transparent_kernel"] / (ms["is_transparent"] / 1e3) / copy_rate}
    if args.stats:
        per_launch = kernel_ns_per_launch(args.stats)
        result["kernel_us_per_launch"] = {k: v / 1e3 for k, v in per_launch.items()}
        result["kernel_fraction_of_copy_rate"] = {k: moved[k] / (v / 1e9) / copy_rate for k, v in per_launch.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
