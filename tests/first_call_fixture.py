"""The fixture tests/c/first_call.c reads: seeded inputs of the six workspace pipelines (footprint_cases.ORACLE_ROWS) on one
ring, and the CPU oracle's outputs for them.  The layout is stated at the top of the C file."""
import collections

import numpy as np

Ring = collections.namedtuple("Ring", "name degree batch plaintext_bits bits")
# N = 256, batch 3: the ring of tests/c/abi_scheme.c, whose relinearize call this matrix is about (log_degree < 12: the unfused
# pipelines); N = 8: fewer coefficients than a wavefront; N = 4096, batch 3, L = 3: footprint_cases.TILED (the tiled transforms).
RINGS = [Ring("N256", 256, 3, 17, (50, 50, 51)), Ring("N8", 8, 2, 17, (27, 28, 28)), Ring("N4096", 4096, 3, 17, (55, 55, 55, 55))]
ELEMENT = 3  # a Galois element valid at every N >= 4


def write(path, oracle, ring, threads=1):
    degree, batch = ring.degree, ring.batch
    t = oracle.generate_primes([ring.plaintext_bits], True, degree)[0]
    q = oracle.generate_primes(list(ring.bits), False, degree)
    ref = oracle.BfvContext(degree, t, q)
    L = ref.L
    assert L == len(q) - 1
    moduli = ref.ciphertext_context().moduli
    rng = np.random.default_rng(degree)

    def uniform(prefix, row_moduli):
        rows = [rng.integers(0, m, size=tuple(prefix) + (degree,), dtype=np.uint64) for m in row_moduli]
        return np.ascontiguousarray(np.stack(rows, axis=len(prefix)))

    lhs, rhs = uniform((batch, 2), moduli), uniform((batch, 2), moduli)
    key, key2 = (uniform((L, 2), ref.key_switching_context().moduli) for _ in range(2))
    secret = uniform((), moduli)
    product = ref.mul(lhs, rhs, L, threads=threads)
    relinearized = ref.relinearize(product, key, L, threads=threads)
    galois = ref.apply_galois(lhs, ELEMENT, key, L)
    grouped = np.stack([ref.apply_galois(lhs, ELEMENT, key, L), ref.apply_galois(rhs, ELEMENT, key2, L)])
    inner = ref.inner_product(lhs, rhs, L)
    qctx, dots = ref.ciphertext_context(L), []
    for ct in product:  # Bfv.dotProduct, as tests/test_gpu_footprint.py states it over the oracle
        ct_eval = qctx.forward_ntt(ct)
        dot, power = ct_eval[0].copy(), secret.copy()
        for index in (1, 2):
            dot = qctx.add(dot, qctx.mul(ct_eval[index], power))
            power = qctx.mul(power, secret)
        dots.append(qctx.inverse_ntt(dot))
    head = np.array([degree, t, len(q), *q, batch, ELEMENT], dtype=np.uint64)
    parts = (head, lhs, rhs, key, key2, secret, product, relinearized, galois, grouped, inner, np.stack(dots))
    shapes = [(batch, 3, L, degree), (batch, 2, L, degree), (batch, 2, L, degree), (2, batch, 2, L, degree), (3, L, degree),
              (batch, L, degree)]
    for part, expected_shape in zip(parts[6:], shapes):
        assert np.asarray(part).shape == expected_shape, (np.asarray(part).shape, expected_shape)
    with open(path, "wb") as out:
        for part in parts:
            out.write(np.ascontiguousarray(part, dtype=np.uint64).tobytes())
