"""Inputs for the edges of the 4-byte polynomial layer (csrc/ntt_word32.hip, csrc/poly_kernels.hip) and for key switches over many ciphertext
moduli at a tiled degree, with their expected values.

The CPU oracle decides the transforms (test_word32_cases.py holds it to a direct O(N^2) evaluation in Python integers for
N <= 64); Python integers decide the element-wise tables and the negacyclic product.  Nothing here imports the device
package: test_gpu_word32_edges.py and test_gpu_bfv.py hold the kernels to what is built here.

Slabs are numpy uint64 arrays [batch][L][N] of canonical words, as the oracle takes them; the GPU tests narrow them.
"""
import functools

import numpy as np

# ---- A1: every degree the 4-byte transforms accept -------------------------------------------------------------------------
DEGREES = [1 << k for k in range(1, 16)]
# (ntt32_kernel runs 64 lanes below N = 128 and 1024 above N = 2048; N = 4096 .. 16384 are register-tiled)
PATTERNS = ("zero", "full", "even", "odd", "last", "x", "half", "uniform")
EDGE_POLYS = 7


def bit_reverse(i, bits):
    out = 0
    for _ in range(bits):
        out, i = (out << 1) | (i & 1), i >> 1
    return out


def small_prime_bits(degree):
    """Width of the two small moduli of a degree's context: the narrowest for which two NTT primes exist at EVERY degree."""
    return degree.bit_length() + 6


def degree_moduli(oracle, degree):
    """large, small, large, small, large (period 5): the three largest 30-bit NTT primes of the degree -- 4p - 1 is within
    140 of 2^32 at N = 2 -- and its two smallest primes of small_prime_bits() bits."""
    large = oracle.generate_primes([30, 30, 30], False, degree, word_bits=32)
    small = oracle.generate_primes([small_prime_bits(degree)] * 2, True, degree, word_bits=32)
    return [large[0], small[0], large[1], small[1], large[2]]


def pattern_row(name, p, degree, rng):
    row = np.zeros(degree, dtype=np.uint64)
    if name == "full":
        row[:] = p - 1
    elif name == "even":
        row[0::2] = p - 1
    elif name == "odd":
        row[1::2] = p - 1
    elif name == "last":
        row[degree - 1] = p - 1
    elif name == "x":
        row[1] = 1
    elif name == "half":
        row[:degree // 2] = p - 1
    elif name == "uniform":
        row[:] = rng.integers(0, p, size=degree, dtype=np.uint64)
    else:
        assert name == "zero"
    return row


def pattern_of(poly, modulus_index):
    """Row (poly, modulus) of the edge slabs holds pattern (poly + modulus) mod 8: polynomials 0 .. 6 give a modulus seven
    of the eight patterns, polynomial 7 -- a slab of its own, see edge_slabs() -- the eighth."""
    return PATTERNS[(poly + modulus_index) % len(PATTERNS)]


def edge_slabs(oracle, degree):
    """-> (moduli, [slab of seven polynomials, slab of one]).  Eight patterns do not fit the seven rows a modulus has in a
    batch of seven, so the pattern each modulus misses there comes as a batch of one: between the two slabs every modulus
    meets every pattern."""
    moduli = degree_moduli(oracle, degree)
    rng = np.random.default_rng(degree)
    rows = [[pattern_row(pattern_of(poly, mi), p, degree, rng) for mi, p in enumerate(moduli)]
            for poly in range(EDGE_POLYS + 1)]
    return moduli, [np.array(rows[:EDGE_POLYS], dtype=np.uint64), np.array(rows[EDGE_POLYS:], dtype=np.uint64)]


@functools.lru_cache(maxsize=None)
def edge_case(oracle, degree):
    """-> (moduli, [(slab, forward, inverse)]) with the oracle's transforms of each slab, computed once per degree."""
    moduli, slabs = edge_slabs(oracle, degree)
    ref = oracle.PolyContext(degree, moduli)
    return moduli, [(slab, ref.forward_ntt(slab), ref.inverse_ntt(slab)) for slab in slabs]


def psi_of(tables, degree, p):
    """The primitive 2N-th root the tables are built on: root_powers is in bit-reversed order, so psi sits at index N / 2."""
    psi = int(tables["root_powers"][degree // 2])
    assert pow(psi, degree, p) == p - 1
    return psi


def direct_forward(row, p, psi):
    """X[i] = sum_j x[j] psi^((2 bitrev(i) + 1) j) mod p (PolyRq+Ntt.swift:237-319's result, without its butterflies)."""
    n = len(row)
    bits = n.bit_length() - 1
    powers = [pow(psi, e, p) for e in range(2 * n)]
    x = [int(v) for v in row]
    return [sum(x[j] * powers[(2 * bit_reverse(i, bits) + 1) * j % (2 * n)] for j in range(n)) % p for i in range(n)]


def direct_inverse(row, p, psi):
    """x[j] = N^-1 sum_i X[i] psi^(-(2 bitrev(i) + 1) j) mod p."""
    n = len(row)
    bits = n.bit_length() - 1
    powers = [pow(psi, -e, p) for e in range(2 * n)]
    X = [int(v) for v in row]
    inv_n = pow(n, -1, p)
    return [inv_n * sum(X[i] * powers[(2 * bit_reverse(i, bits) + 1) * j % (2 * n)] for i in range(n)) % p for j in range(n)]


# ---- A2: the row -> modulus map ---------------------------------------------------------------------------------------------
PERIODS = (1, 2, 3, 5, 6, 7)
PERIOD_DEGREES = (4096, 1024)  # register-tiled, generic
PERIOD_POLYS = 211             # prime, and 211 x 7 rows are more workgroups than the chip holds at once
PERIOD_BITS = 28


def _uniform(rng, batch, moduli, degree):
    return np.stack([rng.integers(0, q, size=(batch, degree), dtype=np.uint64) for q in moduli], axis=1).copy()


def period_case(oracle, degree, period, threads=1):
    """-> (moduli, slab, forward, inverse): 211 polynomials over `period` distinct 28-bit moduli; polynomial 0 is p - 1
    everywhere, polynomial 1 zero, the last one p - 1 in its first half, the rest uniform."""
    moduli = oracle.generate_primes([PERIOD_BITS] * period, False, degree, word_bits=32)
    rng = np.random.default_rng(degree + period)
    slab = _uniform(rng, PERIOD_POLYS, moduli, degree)
    top = np.array(moduli, dtype=np.uint64)[:, None] - np.uint64(1)
    slab[0] = top
    slab[1] = 0
    slab[-1] = 0
    slab[-1, :, :degree // 2] = top
    ref = oracle.PolyContext(degree, moduli)
    return moduli, slab, ref.forward_ntt(slab, threads=threads), ref.inverse_ntt(slab, threads=threads)


# ---- A3: more rows than the chip holds at once --------------------------------------------------------------------------------
CROWDED = ((8192, (30, 30, 29), 400), (16384, (30, 29), 150), (32768, (30, 30), 5))


def crowded_case(oracle, degree, bits, polys, threads=1):
    """-> (moduli, slab, forward): uniform words, the first polynomial zero, the last row p - 1."""
    moduli = oracle.generate_primes(list(bits), False, degree, word_bits=32)
    slab = _uniform(np.random.default_rng(degree + polys), polys, moduli, degree)
    slab[0] = 0
    slab[-1, -1] = moduli[-1] - 1
    return moduli, slab, oracle.PolyContext(degree, moduli).forward_ntt(slab, threads=threads)


# ---- A4: a negacyclic product on 4-byte words only ----------------------------------------------------------------------------
PRODUCT_DEGREE = 128


def negacyclic_product(x, y, p):
    n = len(x)
    out = [0] * n
    for i, xi in enumerate(x):
        for j, yj in enumerate(y):
            if i + j < n:
                out[i + j] += xi * yj
            else:
                out[i + j - n] -= xi * yj
    return [v % p for v in out]


@functools.lru_cache(maxsize=None)
def product_case(oracle):
    """-> (p, x, y, product) [3][1][128]: a uniform pair, p - 1 everywhere times itself, and x^(N-1) times a uniform row."""
    degree = PRODUCT_DEGREE
    p = oracle.generate_primes([30], False, degree, word_bits=32)[0]
    rng = np.random.default_rng(128)
    x, y = _uniform(rng, 3, [p], degree), _uniform(rng, 3, [p], degree)
    x[1], y[1] = p - 1, p - 1
    x[2] = 0
    x[2, 0, degree - 1] = 1
    product = np.array([[negacyclic_product([int(v) for v in a[0]], [int(v) for v in b[0]], p)] for a, b in zip(x, y)],
                       dtype=np.uint64)
    return p, x, y, product


# ---- A5: the element-wise operations on the edge values -----------------------------------------------------------------------
ELEMENTWISE_DEGREES = (64, 4096)


def edge_values(p):
    return [0, 1, 2, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1]


def edge_pairs(p):
    values = edge_values(p)
    return [(a, b) for a in values for b in values]


def edge_scalars(moduli):
    """-> four scalars as residue lists: 0, 1, (p - 1) / 2, p - 1."""
    return [[0] * len(moduli), [1] * len(moduli), [(p - 1) // 2 for p in moduli], [p - 1 for p in moduli]]


def elementwise_moduli(oracle, degree):
    """The largest 30-bit prime, a 20-bit prime and the smallest prime of the degree's A1 context."""
    moduli = [oracle.generate_primes([30], False, degree, word_bits=32)[0],
              oracle.generate_primes([20], True, degree, word_bits=32)[0], min(degree_moduli(oracle, degree))]
    assert len(set(moduli)) == 3
    return moduli


def elementwise_case(oracle, degree):
    """-> (moduli, lhs, rhs) [2][3][N]: polynomial 0 carries the 49 operand pairs of its row's modulus, tiled along the row
    for as many whole tables as fit; the words behind them and polynomial 1 are uniform."""
    moduli = elementwise_moduli(oracle, degree)
    rng = np.random.default_rng(degree + 49)
    lhs, rhs = _uniform(rng, 2, moduli, degree), _uniform(rng, 2, moduli, degree)
    for mi, p in enumerate(moduli):
        pairs = edge_pairs(p)
        tiled = pairs * (degree // len(pairs))
        lhs[0, mi, :len(tiled)] = [a for a, _ in tiled]
        rhs[0, mi, :len(tiled)] = [b for _, b in tiled]
    return moduli, lhs, rhs


def elementwise_expected(op, moduli, lhs, rhs=None, scalars=None):
    """add / sub / mul / neg / mul_scalar in Python integers."""
    out = np.zeros_like(lhs)
    for mi, p in enumerate(moduli):
        for poly in range(lhs.shape[0]):
            a = [int(v) for v in lhs[poly, mi]]
            b = [int(v) for v in rhs[poly, mi]] if rhs is not None else None
            if op == "add":
                row = [(x + y) % p for x, y in zip(a, b)]
            elif op == "sub":
                row = [(x - y) % p for x, y in zip(a, b)]
            elif op == "mul":
                row = [x * y % p for x, y in zip(a, b)]
            elif op == "neg":
                row = [-x % p for x in a]
            else:
                assert op == "mul_scalar"
                row = [x * scalars[mi] % p for x in a]
            out[poly, mi] = row
    return out


# ---- A6: a degree the 4-byte transforms refuse ---------------------------------------------------------------------------------
REFUSED_DEGREE, REFUSED_MODULUS = 65536, 786433  # 3 * 2^18 + 1: an NTT prime of the degree, so only the degree is at fault


# ---- B: many ciphertext moduli at a tiled degree, both word sizes -------------------------------------------------------------
MANY_MODULI_DEGREE = 4096
# (name, word bits, bits of the L ciphertext moduli + the special one, preferring_small)
MANY_MODULI_SETS = (
    ("w32_30x14", 32, [30] * 15, False),  # the most 30-bit moduli the reference admits; the largest 64-bit product sum
    ("w32_26x16", 32, [26] * 17, False),  # L > 15: the generic key MAC at a tiled degree
    ("w64_60x8", 64, [60] * 9, False),    # L <= 8 and 8 p < 2^63: the bounded reduction at its limit
    ("w64_55x9", 64, [55] * 10, False),   # L = 9: the general reduction
    ("w64_61x4", 64, [61] * 5, False),    # 4 p < 2^63 for every 61-bit p: bounded
    ("w64_61x5", 64, [61] * 6, False),    # 5 p >= 2^63 for p above 2^63 / 5: general
    ("w64_50x16", 64, [50] * 17, False),  # the widest band the BEHZ kernels are specialised for
)
# L p on either side of 2^63 at 61 bits takes four and five of the LARGEST 61-bit primes.  Three and four of the SMALLEST,
# generate_primes([61] * (L + 1), True, 4096), are no parameter sets: the smallest 61-bit NTT primes ARE the Bsk base
# (RnsTool.swift:30-33), so Context.init fails on moduli that are not coprime; and 4 p < 2^63 for every p < 2^61, so four
# moduli never reach the other side.  test_word32_cases.py asserts both statements.
INADMISSIBLE_SETS = (([61] * 4, True), ([61] * 5, True))
FINISH_IN_STORE_ROWS = {32: 2048, 64: 1024}  # polys * 2 * (L + 1) above this: the key switch ends in the transform's store


def many_moduli_set(oracle, name):
    """-> (word bits, t, moduli)."""
    _, word_bits, bits, small = next(s for s in MANY_MODULI_SETS if s[0] == name)
    t = oracle.generate_primes([17], True, MANY_MODULI_DEGREE)[0]
    return word_bits, t, oracle.generate_primes(bits, small, MANY_MODULI_DEGREE, word_bits=word_bits)


def batch_above_finish_threshold(word_bits, L):
    """The smallest polys with polys * 2 * (L + 1) > the threshold."""
    return FINISH_IN_STORE_ROWS[word_bits] // (2 * (L + 1)) + 1


def many_moduli_slab(rng, prefix, moduli, zero_second=True, degree=MANY_MODULI_DEGREE):
    """[*prefix][len(moduli)][N]: block 0 along the first axis holds modulus - 1 in every residue, block 1 zeros (ciphertext
    batches; a key keeps it uniform: zero_second=False), the rest uniform words."""
    rows = [rng.integers(0, q, size=tuple(prefix) + (degree,), dtype=np.uint64) for q in moduli]
    slab = np.ascontiguousarray(np.stack(rows, axis=len(prefix)))
    slab[0] = (np.array(moduli, dtype=np.uint64) - np.uint64(1))[:, None]
    if zero_second and prefix[0] > 1:
        slab[1] = 0
    return slab
