"""The case table of the processed-database file tests, shared by tests/test_pir_database_file.py (no device) and
tests/test_gpu_pir_database_file.py.

Parameter sets: the moduli widths of tests/test_gpu_pir_database.py (40/40/41 and 40/40/40/41 bits under a 17-bit t, the
27/28/28-bit set of its UInt32 test) and of tests/ciphertext_wire_cases.py (55 / 40 / 62 bits), at the degrees where the
kernels can go wrong:
  N = 8    a row is w bytes (27 .. 62), a payload a few dozen: most aligned 8-byte chunks hold the end of one payload, a tag
           and the start of the next, and under a nil run a chunk holds several tags
  N = 64   rows of a whole number of 8-byte chunks, payloads that are not, so every payload starts at another residue
  N = 256  several workgroups per plaintext on load
  L = 1, 2, 3 rows per plaintext (the last modulus of a set of several is the key-switching one and has no row)
  62 bits  a field that crosses from one aligned 8-byte word of the file into the next (above 56 bits every field can)
  UInt32   the widths a Bfv<UInt32> context has; the device tests run them on packed 4-byte slabs
Presence patterns and counts rotate so that every pattern meets every parameter set."""
import collections

import numpy as np

Params = collections.namedtuple("Params", "name word_bits degree q_bits")
Case = collections.namedtuple("Case", "params pattern count")

T_BITS = 17  # the plaintext modulus of tests/test_gpu_pir_database.py; the file format does not depend on it

PARAMS = (
    Params("u64-n8-l2", 64, 8, (40, 40, 41)),
    Params("u64-n8-l3-wide", 64, 8, (55, 40, 62, 62)),
    Params("u64-n64-l3", 64, 64, (40, 40, 40, 41)),
    Params("u64-n64-l1-wide", 64, 64, (62,)),
    Params("u64-n256-l3", 64, 256, (40, 40, 40, 41)),
    Params("u32-n8-l2", 32, 8, (27, 28, 28)),
    Params("u32-n64-l1", 32, 64, (27,)),
    Params("u32-n256-l2", 32, 256, (27, 28, 28)),
)
PATTERNS = ("all", "none", "one", "edges-nil", "alternating", "run-one-nil", "random")
COUNTS = (2, 5, 13, 36)


def rows_of(params):
    """L: the moduli of the top-level ciphertext context"""
    return max(1, len(params.q_bits) - 1)


def moduli_of(params, generate_primes):
    """(plaintext modulus, coefficient moduli) as tests/test_gpu_pir_database.py draws them"""
    t = generate_primes([T_BITS], True, params.degree)[0]
    return int(t), [int(q) for q in generate_primes(list(params.q_bits), False, params.degree)]


def mask_of(case):
    """the present bytes of a case; present plaintexts carry 1, and in "random" also other non-zero bytes (any byte != 0 is
    present to the device entries)"""
    count, pattern = case.count, case.pattern
    mask = np.ones(count, dtype=np.uint8)
    if pattern == "none":
        mask[:] = 0
    elif pattern == "one":
        mask[:] = 0
        mask[count // 2] = 1
    elif pattern == "edges-nil":
        mask[0] = mask[-1] = 0
    elif pattern == "alternating":
        mask[1::2] = 0
    elif pattern == "run-one-nil":
        mask[(2 * count) // 3] = 0
    elif pattern == "random":
        rng = np.random.default_rng(1000 + count)
        mask = (rng.integers(0, 3, size=count) != 0).astype(np.uint8) * rng.integers(1, 256, size=count).astype(np.uint8)
    return mask


def cases():
    out = []
    for i, params in enumerate(PARAMS):
        out += [Case(params, "none", 0), Case(params, "all", 1), Case(params, "none", 1)]
        for j, pattern in enumerate(PATTERNS):
            out.append(Case(params, pattern, COUNTS[(i + j) % len(COUNTS)]))
    return out


ALL = cases()


def case_id(case):
    return f"{case.params.name}-{case.pattern}-c{case.count}"


def seed_of(case):
    return sum(ord(c) for c in case_id(case))
