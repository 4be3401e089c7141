"""Encryption and key generation on the device (he_bfv_encrypt_device, he_bfv_generate_key_switch_keys_device) at two shapes:

    encrypt    N = 8192, L = 4 x 55-bit moduli (+ a 55-bit key-switching modulus), a 17-bit t: 1024 encryptions
    keys       N = 4096, moduli of 27, 28, 28 bits (L = 2): 28 key-switch keys = 56 Eval encryptions of zero over 3 moduli

    python bench_tools/encrypt_bench.py [--steps K] [--warmup W]

One JSON line.  Per shape three figures from the same run, alternating per step, device events around each call, medians:
  (a) the entry;
  (b) he_poly_random_from_seeds_device alone on the same `a` seeds over the same moduli: the AES blocks of the uniform stream,
      which the pipelines are supposed to be bound by (the error stream adds 1/m of them) -- the ratio (a)/(b) is recorded,
      not asserted;
  (c) the composition a caller had before these entries: the uniform sampler, he_poly_mul, the transforms, add / neg (and
      he_bfv_add_plain_device, or the key-switch term by he_poly_mul_scalar + add on the one row), with the error polynomials
      handed to it.  Outside the timed window it is given: the error polynomials in Coeff form as a device slab (a caller then made
      them on the host and uploaded them; here the centred binomial sampler makes them from the same error seeds, which the tests
      hold word for word to the restatement), the secret key replicated per ciphertext, and for the keys the current keys already
      multiplied by q_ks mod q_j and spread to [keys][L][N] rows.
(a) and (c) are compared word for word before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd")):
    if path not in sys.path:
        sys.path.insert(0, path)


def _time(variants, steps, warmup, torch):
    for _ in range(warmup):
        for run in variants.values():
            run()
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in variants}
    for _ in range(steps):
        for name, run in variants.items():  # alternating, so that a drift of the clock reaches every variant alike
            begin.record()
            run()
            end.record()
            end.synchronize()
            times[name].append(begin.elapsed_time(end))
    return ({name: float(np.median(v)) for name, v in times.items()}, {name: float(min(v)) for name, v in times.items()},
            {name: float(max(v)) for name, v in times.items()})


def _seeds(torch, count, salt):
    return torch.from_numpy(np.random.default_rng(salt).integers(0, 256, (count, 32), dtype=np.uint8)).cuda()


def encrypt_shape(heamd, torch, steps, warmup, batch=1024):
    n, L = 8192, 4
    t = heamd.generate_primes([17], True, n)[0]
    q = heamd.generate_primes([55] * (L + 1), False, n)
    ctx = heamd.BfvContext(n, t, q)
    poly = ctx.ciphertext_context()
    key = ctx.generate_secret_key(_seeds(torch, 1, 1))[0].contiguous()
    a_seeds, e_seeds = _seeds(torch, batch, 2), _seeds(torch, batch, 3)
    plaintexts = heamd.to_device(np.random.default_rng(4).integers(0, t, (batch, n)).astype(np.uint64))
    workspace = torch.empty(ctx.encrypt_workspace_bytes("encrypt", batch), dtype=torch.uint8, device="cuda")
    # handed to the composition
    errors = poly.random_centered_binomial_from_seeds(e_seeds)
    key_per_ciphertext = key[:L].unsqueeze(0).expand(batch, L, n).contiguous()

    def composition():
        a = poly.random_from_seeds(a_seeds)
        c0 = a.clone()
        poly.mul_(c0, key_per_ciphertext)
        poly.inverse_ntt_(c0)
        poly.inverse_ntt_(a)
        poly.add_(c0, errors)
        poly.neg_(c0)
        cts = torch.stack([c0, a], dim=1)
        ctx.add_plain_(cts, plaintexts)
        return cts

    variants = {
        "encrypt": lambda: ctx.encrypt(plaintexts, key, a_seeds, e_seeds, workspace=workspace),
        "uniform_sampler": lambda: poly.random_from_seeds(a_seeds),
        "composition": composition,
    }
    same = bool(torch.equal(variants["encrypt"](), composition()))
    assert same, "encrypt and the composition of the earlier entries differ"
    ms, low, high = _time(variants, steps, warmup, torch)
    return {"degree": n, "L": L, "moduli_bits": 55, "t_bits": 17, "batch": batch, "same_words": same, "ms_median": ms,
            "ms_min": low, "ms_max": high, "encrypt_over_uniform_sampler": ms["encrypt"] / ms["uniform_sampler"],
            "encrypt_over_composition": ms["encrypt"] / ms["composition"],
            "encryptions_per_s": batch / (ms["encrypt"] / 1e3), "a_stream_bytes": batch * L * n * 16}


def keys_shape(heamd, torch, steps, warmup, keys=28):
    n = 4096
    t = heamd.generate_primes([17], True, n)[0]
    q = heamd.generate_primes([27, 28, 28], False, n)
    ctx = heamd.BfvContext(n, t, q)
    L, m = ctx.L, len(q)
    ks = ctx.key_switching_context()
    key = ctx.generate_secret_key(_seeds(torch, 1, 11))[0].contiguous()
    count = keys * L
    a_seeds, e_seeds = _seeds(torch, count, 12), _seeds(torch, count, 13)
    current = ks.random_from_seeds(_seeds(torch, keys, 14))  # [keys][L + 1][N]: any Eval polynomials time alike
    workspace = torch.empty(ctx.encrypt_workspace_bytes("key_switch_keys", keys), dtype=torch.uint8, device="cuda")
    # handed to the composition
    errors = ks.random_centered_binomial_from_seeds(e_seeds)  # [count][L + 1][N] Coeff
    key_per_ciphertext = key.unsqueeze(0).expand(count, m, n).contiguous()
    scaled = current.clone()
    ks.mul_scalar_(scaled, [q[-1] % qi for qi in q])
    payload = torch.zeros((keys, L, m, n), dtype=torch.int64, device="cuda")
    for j in range(L):
        payload[:, j, j] = scaled[:, j]
    payload = payload.reshape(count, m, n).contiguous()

    def composition():
        a = ks.random_from_seeds(a_seeds)
        c0 = a.clone()
        ks.mul_(c0, key_per_ciphertext)
        error_eval = errors.clone()
        ks.forward_ntt_(error_eval)
        ks.add_(c0, error_eval)
        ks.neg_(c0)
        ks.add_(c0, payload)
        return torch.stack([c0, a], dim=1).reshape(keys, L, 2, m, n)

    variants = {
        "key_switch_keys": lambda: ctx.generate_key_switch_keys(key, current, a_seeds, e_seeds, workspace=workspace),
        "uniform_sampler": lambda: ks.random_from_seeds(a_seeds),
        "composition": composition,
    }
    same = bool(torch.equal(variants["key_switch_keys"](), composition()))
    assert same, "key generation and the composition of the earlier entries differ"
    ms, low, high = _time(variants, steps, warmup, torch)
    return {"degree": n, "L": L, "moduli_bits": [27, 28, 28], "keys": keys, "ciphertexts": count, "same_words": same,
            "ms_median": ms, "ms_min": low, "ms_max": high,
            "keys_over_uniform_sampler": ms["key_switch_keys"] / ms["uniform_sampler"],
            "keys_over_composition": ms["key_switch_keys"] / ms["composition"],
            "key_switch_keys_per_s": keys / (ms["key_switch_keys"] / 1e3), "a_stream_bytes": count * m * n * 16}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    args = parser.parse_args()

    import torch

    import heamd

    assert torch.cuda.is_available(), "encrypt_bench.py measures on a GPU"
    print(json.dumps({"tool": "encrypt_bench", "steps": args.steps, "warmup": args.warmup,
                      "encrypt": encrypt_shape(heamd, torch, args.steps, args.warmup),
                      "keys": keys_shape(heamd, torch, args.steps, args.warmup)}))


if __name__ == "__main__":
    main()
