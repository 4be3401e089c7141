"""The device-side arithmetic of csrc/device_math.hpp on its own (tests/device_probe/arith_probe.hip runs each function one lane
per operand tuple): the congruence or exact value and the range that the header's comment states for it, against Python integers,
inside the function's stated preconditions -- every 64-bit pattern where it states none.  Constants (Shoup and Barrett factors)
are computed here from their definitions.  tests/test_device_math_bounds.py holds the same claims on Python integers.

The limb-wise Shoup products and the shift-folded products (probe kinds 0 .. 7) -- for ANY 64-bit operand, which is what the
butterflies rely on (the forward transform never folds its words, the limb-wise inverse multiplies x - y as a signed word without
adding a bound first):
    split_mul_add<false / true, false>        [0, 8p), = y w (mod p)           test_split_products_any_word
    split_mul_signed<false / true>            (0, 6p), = d w (mod p), d signed  test_split_products_any_word
    fold_mul<false / true, false / true>      [0, 6p), = y w (mod p)           test_folded_products_any_word

Every other function (probe kind in brackets) and the contract asserted:
    mulhi32 [10], mullo32 [11]                exact high / low word of a 32 x 32 product           test_word_products
    mulhi64 [12], mul_wide [15]               exact                                                test_word_products
    mulhi64_approx [13]                       in [exact - 2, exact]                                test_word_products
    mullo64_sum2 [14]                         = a b + c d (mod 2^64)                               test_word_products
    csub63<false> [16], csub63<true> [17]     x < 2m, m <= 2^63: x - m if x >= m, else x           test_conditional_subtract
    add_mod [18], sub_mod [19], neg_mod [20]  canonical operands: the canonical sum, difference,
      and _uniform [21, 22, 23]               negation; neg_mod(0) = 0                             test_modular_add_sub_neg
    shoup_quotient<U, false> [26, 27]         x, f < 2^63: in [floor(x f / 2^64) - 1, the same]    test_shoup_quotient
    shoup_quotient<U, true> [28, 29]          any x, f: in [floor(x f / 2^64) - 2, the same]       test_shoup_quotient
    shoup_lazy [24]                           any x: [0, 2p), = x w                                test_shoup_products
    shoup_mul [25]                            any x: x w mod p                                     test_shoup_products
    shoup_lazy4 [30], _uniform [31]           any x, 4p < 2^64: [0, 4p), = x w                     test_shoup_products
    shoup_lazy4_fma<false / true> [32, 33]    = addend + shoup_lazy4 (mod 2^64)                    test_shoup_products
    shoup_headroom [34], _uniform [35]        x < 2^63, 5p < 2^64: [0, 5p), = x w                  test_shoup_products
    shoup_headroom_fma<false / true> [36, 37] = addend + shoup_headroom (mod 2^64)                 test_shoup_products
    shoup_mul_uniform_lazy [38]               x < 2^63, p <= 2^62 - 1: [0, 3p), = x w              test_shoup_products
    shoup_mul_uniform [39]                    x < 2^63, p <= 2^62 - 1: x w mod p                   test_shoup_products
    barrett_reduce64 [40], _uniform [42]      any x: x mod p                                       test_barrett_reduce64
    barrett_reduce64_uniform_lazy [41]        any x: [0, 2p), = x (both sides of p = 2^32)         test_barrett_reduce64
    barrett_mul [43]                          x, y < p: x y mod p                                  test_barrett_mul
    barrett_reduce128 [44]                    any 128-bit x: x mod p                               test_barrett_reduce128
    product_sum_add [60]; _add_one<false / true> [61, 62]; _add_pair [63, 64]; _add_triple [65, 66];
      _add_all<1, 2, 3, 4, 5, 7; false / true> [67 .. 78]; _add_uniform [79]; _add_uniform_short [80];
      _first [81], _first_uniform [82], _first_uniform_short [83] (each followed by its _add):
                                              every sum's value = its own sum of a_k b_k (mod 2^128), and product_sum_value
                                              of the lane's fields = the fields' value; NARROW: operands < 2^56, <= 127 terms,
                                              exact; _short: terms (hi32(a_max) + hi32(b_max) + 2) <= 2^32
                                                                                                   test_product_sum_accumulation,
                                                                                                   test_product_sum_narrow_limits,
                                                                                                   test_product_sum_short_limits
    product_sum_value [45]                    = t + c 2^32 + (h + t_carry + c_carry 2^32) 2^64 (mod 2^128), any fields
                                                                                                   test_product_sum_value_any_fields
    reduce_product_sum [46]                   value < 2^127, p <= 2^62 - 1: value mod p            test_reduce_product_sum
    reduce_product_sum_lazy [47]              value < 2^127, 5p < 2^64: [0, 5p), = value           test_reduce_product_sum
    reduce_product_sum_bounded_lazy [48]      2^33 < p < 2^61, value < 2^(64 + sh): [0, 5p), = value
                                                                                                   test_reduce_product_sum_bounded
    reduce_product_sum_bounded [49]           the same preconditions: value mod p                  test_reduce_product_sum_bounded
    shoup32_lazy [50]                         any 32-bit x, p <= 2^30 - 1: [0, 2p), = x w          test_word32_products
    shoup32_lazy_mad<false / true> [51, 52]   the same word as shoup32_lazy                        test_word32_products
"""
import ctypes
import os
import random

import numpy as np
import pytest

import device_math_cases as cases
from device_math_cases import MASK32, MASK64, MASK128

pytestmark = pytest.mark.gpu

PROBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_probe", "libarith_probe.so")


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tests/device_probe/libarith_probe.so is built by __graft_entry__.build()"
    # PyTorch ships its own HIP runtime: import it first, as heamd.load_library() does, so that the probe binds to that
    # instance -- loaded the other way round, every later torch test of the same session finds no device
    import torch  # noqa: F401

    lib = ctypes.CDLL(PROBE)
    lib.arith_probe_split_product.restype = ctypes.c_int
    lib.arith_probe_split_product.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.c_void_p]
    lib.arith_probe_fold_product.restype = ctypes.c_int
    lib.arith_probe_fold_product.argtypes = lib.arith_probe_split_product.argtypes
    lib.arith_probe_contract.restype = ctypes.c_int
    lib.arith_probe_contract.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    lib.arith_probe_product_sum.restype = ctypes.c_int
    lib.arith_probe_product_sum.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                            ctypes.c_void_p]
    lib.arith_probe_product_sum_sums.restype = ctypes.c_int
    lib.arith_probe_product_sum_sums.argtypes = [ctypes.c_int]
    return lib


def _run(lib, kind, p, operands, constants):
    a = np.array(operands, dtype=np.uint64)
    c = np.array(constants, dtype=np.uint64)
    out = np.zeros(len(operands), dtype=np.uint64)
    entry = lib.arith_probe_split_product if kind < 4 else lib.arith_probe_fold_product
    status = entry(kind, p, a.ctypes.data, c.ctypes.data, len(operands), out.ctypes.data)
    assert status == 0, status
    return [int(v) for v in out]


_operands = cases.operands
_constants = cases.constants


MODULI = [(1 << 40) + 15, 1099511922689, 281474976694273, 18014398509309953, 36028797018652673, 36028797018914815,
          (1 << 55) - 55]


@pytest.mark.parametrize("p", MODULI)
def test_split_products_any_word(probe, p):
    """split_mul_add (unsigned word y): y w - Q 2p in [0, 8p), congruent to y w.  split_mul_signed (signed word d, the
    constant's second word in signed limbs): d w + bias - ... in (0, 6p), congruent to d w -- both for every 64-bit pattern,
    limb edges and sign edges included, constants at the ends of [0, p); moduli across [2^40, 2^55) (the products use nothing
    of a modulus but its size and oddness, so the list is not restricted to primes or NTT moduli)."""
    assert (1 << 40) <= p < (1 << 55) and p % 2 == 1
    rng = random.Random(p)
    count = 1 << 14
    operands = _operands(rng, count)
    rng.shuffle(operands)
    constants = _constants(rng, p, count)
    # every edge word against every edge constant, then the shuffled lists pair by pair
    edge_words, edge_constants = _operands(rng, 20), _constants(rng, p, 10)
    operands = [y for y in edge_words for _ in edge_constants] + operands
    constants = [w for _ in edge_words for w in edge_constants] + constants
    for kind in (0, 1):
        got = _run(probe, kind, p, operands, constants)
        for y, w, r in zip(operands, constants, got):
            value = y if kind == 0 else (y - (1 << 64) if y >> 63 else y)
            assert (r - value * w) % p == 0, (kind, hex(y), w, r)
            assert (0 <= r < 8 * p) if kind == 0 else (0 < r < 6 * p), (kind, hex(y), w, r // p)
    # wave-uniform constants (the constant's words in scalar registers): one constant per launch
    for w in constants[:12] + constants[-4:]:
        for kind in (2, 3):
            got = _run(probe, kind, p, operands[:1024], [w] * 1024)
            for y, r in zip(operands[:1024], got):
                value = y if kind == 2 else (y - (1 << 64) if y >> 63 else y)
                assert (r - value * w) % p == 0, (kind, hex(y), w, r)
                assert (0 <= r < 8 * p) if kind == 2 else (0 < r < 6 * p), (kind, hex(y), w, r // p)


# p = 2^b - d at both ends of d < 2^(b-32) for b = 41, 47, 52, 55 (kModeFoldLazy: the bound since round 6, 2^(b-33) before --
# both kept), 56 and 60 (kModeFoldMinus: d < 2^(b-33))
FOLD_MINUS = [(1 << 41) - 1, (1 << 41) - 255, (1 << 41) - 511, (1 << 47) - 8191, (1 << 47) - 16383, (1 << 47) - 32767,
              (1 << 52) - 245759, (1 << 52) - 524287, (1 << 52) - 1048575, (1 << 55) - 55, (1 << 55) - 4087807,
              (1 << 55) - 4194303, (1 << 55) - 8388607, (1 << 56) - 27, (1 << 56) - 8388607, (1 << 60) - 93,
              (1 << 60) - 134217727]
# p = 2^60 + e, e < 2^24 (the BEHZ auxiliary primes' form)
FOLD_PLUS = [(1 << 60) + 33, (1 << 60) + 1, (1 << 60) + (1 << 24) - 1, (1 << 60) + 8380417]


@pytest.mark.parametrize("p", FOLD_MINUS + FOLD_PLUS)
def test_folded_products_any_word(probe, p):
    """fold_mul (csrc/device_math.hpp): the product by a constant folded by a shift at 2^(b+2) (p = 2^b - d) or 2^62 (p = 2^60 + e):
    congruent to y w and below 6p for EVERY 64-bit y -- what lets kModeFoldLazy's butterflies run without a conditional
    subtract (tests/test_fold_product_bounds.py holds the same claims on Python integers); constants in vector registers and
    wave-uniform."""
    plus = p > (1 << 60)
    rng = random.Random(p)
    count = 1 << 13
    edge_words, edge_constants = _operands(rng, 20), _constants(rng, p, 10)
    operands = [y for y in edge_words for _ in edge_constants] + _operands(rng, count)
    constants = [w for _ in edge_words for w in edge_constants] + _constants(rng, p, count)
    got = _run(probe, 6 if plus else 4, p, operands, constants)
    for y, w, r in zip(operands, constants, got):
        assert (r - y * w) % p == 0, (hex(y), w, r)
        assert 0 <= r < 6 * p, (hex(y), w, r / p)
    for w in constants[:12] + constants[-4:]:
        got = _run(probe, 7 if plus else 5, p, operands[:1024], [w] * 1024)
        for y, r in zip(operands[:1024], got):
            assert (r - y * w) % p == 0, (hex(y), w, r)
            assert 0 <= r < 6 * p, (hex(y), w, r / p)


# ---- every other function of device_math.hpp ---------------------------------------------------------------------------


def _eval(lib, kind, columns, outputs=1):
    """One launch of probe kind `kind`: columns of equal length (a plain integer stands for a column of that constant) -> the
    output column, or the list of output columns."""
    count = max(len(c) for c in columns if not isinstance(c, int))
    data = np.array([[c] * count if isinstance(c, int) else c for c in columns], dtype=np.uint64)
    assert data.shape == (len(columns), count) and count <= 1 << 14
    out = np.zeros((outputs, count), dtype=np.uint64)
    status = lib.arith_probe_contract(kind, data.ctypes.data, len(columns), count, out.ctypes.data, outputs)
    assert status == 0, (kind, status)
    result = [[int(v) for v in row] for row in out]
    return result[0] if outputs == 1 else result


def _accumulate(lib, kind, a, b):
    """a[sums][terms][lanes], b[terms][lanes] -> [sum][lane] = (t, c, h, t_carry, c_carry, value.lo, value.hi)."""
    a, b = np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64)
    sums, terms, lanes = a.shape
    assert b.shape == (terms, lanes) and sums == lib.arith_probe_product_sum_sums(kind)
    out = np.zeros((sums, 7, lanes), dtype=np.uint64)
    status = lib.arith_probe_product_sum(kind, a.ctypes.data, b.ctypes.data, terms, lanes, out.ctypes.data)
    assert status == 0, (kind, status)
    return [[tuple(int(v) for v in out[j, :, i]) for i in range(lanes)] for j in range(sums)]


def test_word_products(probe):
    """mulhi32, mullo32, mulhi64, mul_wide exact; mullo64_sum2 exact mod 2^64; mulhi64_approx in [exact - 2, exact] -- limbs at
    0, 1, 2^31 - 1, 2^31 and all ones in every combination (the dropped low-column carries are largest there), the word edges
    crossed with each other, and random words."""
    rng = random.Random(101)
    words = cases.LIMB_WORDS + cases.WORD_EDGES + cases.CARRY_WORDS
    a, b = cases.crossed(words, words)
    a, b = a + _operands(rng, 4000), b + [rng.getrandbits(64) for _ in range(4000)]
    c, d = [rng.choice(words + [rng.getrandbits(64)]) for _ in a], [rng.choice(words + [rng.getrandbits(64)]) for _ in a]
    high32, low32, high, approx = (_eval(probe, kind, [a, b]) for kind in (10, 11, 12, 13))
    sum2 = _eval(probe, 14, [a, b, c, d])
    wide_lo, wide_hi = _eval(probe, 15, [a, b], outputs=2)
    lowest = 0
    for i, (x, y) in enumerate(zip(a, b)):
        narrow = (x & MASK32) * (y & MASK32)
        assert (high32[i], low32[i]) == (narrow >> 32, narrow & MASK32), (hex(x), hex(y))
        assert high[i] == (x * y) >> 64, (hex(x), hex(y))
        assert (wide_lo[i], wide_hi[i]) == ((x * y) & MASK64, (x * y) >> 64), (hex(x), hex(y))
        assert ((x * y) >> 64) - 2 <= approx[i] <= (x * y) >> 64, (hex(x), hex(y), approx[i] - ((x * y) >> 64))
        lowest = max(lowest, ((x * y) >> 64) - approx[i])
        assert sum2[i] == (x * y + c[i] * d[i]) & MASK64, (hex(x), hex(y), hex(c[i]), hex(d[i]))
    assert lowest == 2  # the operands reach the bound they test


CSUB_MODULI = [3, 1 << 32, (1 << 62) - 57, 1 << 63]


def test_conditional_subtract(probe):
    """csub63<false / true>(x, 2^64 - m) for x < 2m, m <= 2^63: x - m if x >= m, else x -- at both ends of both ranges, m = 2^63
    (where the sign of the wrapped difference alone decides) included."""
    rng = random.Random(102)
    xs, ms = [], []
    for m in CSUB_MODULI:
        for x in [0, m - 1, m, m + 1, 2 * m - 1, m // 2, m + m // 2] + [rng.randrange(2 * m) for _ in range(200)]:
            xs.append(x)
            ms.append(m)
    got = _eval(probe, 16, [xs, [(-m) & MASK64 for m in ms]])
    for x, m, r in zip(xs, ms, got):
        assert r == (x - m if x >= m else x), (hex(x), hex(m), hex(r))
    for m in CSUB_MODULI:
        mine = [x for x, mm in zip(xs, ms) if mm == m]
        for x, r in zip(mine, _eval(probe, 17, [mine, (-m) & MASK64])):
            assert r == (x - m if x >= m else x), (hex(x), hex(m), hex(r))


def test_modular_add_sub_neg(probe):
    """add_mod, sub_mod, neg_mod and their _uniform twins on canonical operands, p <= 2^62 - 1: the canonical result, with the
    operands at the ends of [0, p) in every combination and neg_mod(0) = 0."""
    rng = random.Random(103)
    moduli = [3] + cases.SHOUP_MODULI + [(1 << 62) - 1]
    per_modulus = {}
    for p in moduli:
        ends = [0, 1, p - 1, p - 2, p >> 1, (p >> 1) + 1]
        a, b = cases.crossed(ends, ends)
        per_modulus[p] = (a + [rng.randrange(p) for _ in range(100)], b + [rng.randrange(p) for _ in range(100)])

    def check(p, a, b, added, subtracted, negated):
        for x, y, s, d, n in zip(a, b, added, subtracted, negated):
            assert s == (x + y) % p and d == (x - y) % p and n == (-x) % p, (p, x, y, s, d, n)

    a = [x for p in moduli for x in per_modulus[p][0]]
    b = [y for p in moduli for y in per_modulus[p][1]]
    ps = [p for p in moduli for _ in per_modulus[p][0]]
    got = (_eval(probe, 18, [a, b, ps]), _eval(probe, 19, [a, b, ps]), _eval(probe, 20, [a, ps]))
    for x, y, p, s, d, n in zip(a, b, ps, *got):
        check(p, [x], [y], [s], [d], [n])
    for p in moduli:
        a, b = per_modulus[p]
        check(p, a, b, _eval(probe, 21, [a, b, p]), _eval(probe, 22, [a, b, p]), _eval(probe, 23, [a, p]))
        assert _eval(probe, 20, [[0], [p]]) == [0] and _eval(probe, 23, [[0], p]) == [0]


def test_shoup_quotient(probe):
    """shoup_quotient<UNIFORM, CARRY>(x, f) against floor(x f / 2^64): never above; CARRY = false (x, f < 2^63) at most 1
    below, CARRY = true (any x, f) at most 2 below -- all-ones limbs in every combination, and for the CARRY forms x and f with
    both top bits set over all-ones low limbs, where the cross column's 65th bit fires."""
    rng = random.Random(104)
    for carry, kinds, slack in ((False, (26, 27), 1), (True, (28, 29), 2)):
        limit = 1 << 64 if carry else 1 << 63
        words = [x for x in cases.LIMB_WORDS + cases.WORD_EDGES + (cases.CARRY_WORDS if carry else []) if x < limit]
        xs, fs = cases.crossed(words, words)
        xs, fs = xs + [rng.randrange(limit) for _ in range(4000)], fs + [rng.randrange(limit) for _ in range(4000)]
        lowest, fired = 0, 0
        for x, f, q in zip(xs, fs, _eval(probe, kinds[0], [xs, fs])):
            exact = (x * f) >> 64
            assert exact - slack <= q <= exact, (kinds[0], hex(x), hex(f), q - exact)
            lowest = max(lowest, exact - q)
            fired += ((x & MASK32) * (f >> 32) + (x >> 32) * (f & MASK32)) >> 64
        assert lowest >= 1 and (fired > 50) == carry
        # wave-uniform factor: one per launch, every edge factor and a few random ones
        for f in words + [rng.randrange(limit) for _ in range(4)]:
            mine = words + cases.quotient_steps(f, limit) + [rng.randrange(limit) for _ in range(64)]
            for x, q in zip(mine, _eval(probe, kinds[1], [mine, f])):
                exact = (x * f) >> 64
                assert exact - slack <= q <= exact, (kinds[1], hex(x), hex(f), q - exact)


@pytest.mark.parametrize("p", cases.SHOUP_MODULI)
def test_shoup_products(probe, p):
    """The Shoup family at one modulus, each function inside its own bound on p and on x: constants at the ends of [0, p) and
    at floor(p / 2) +- 1; multiplicands at k p - 1, k p, k p + 1 up to the largest k the precondition admits, next to the
    steps of the exact quotient floor(x wf / 2^64), with all-ones limbs, and random.  Ranges and congruences as the module's
    docstring lists them; the _fma forms equal addend + plain result mod 2^64, with addends that wrap."""
    rng = random.Random(p)
    ws = cases.shoup_constants(p) + [rng.randrange(p) for _ in range(3)]
    any_word, below_2_63 = 1 << 64, 1 << 63

    def gather(limit, halved):
        xs, cs = [], []
        for w in ws:
            wf = cases.shoup_factor(w, p)
            mine = cases.shoup_operands(rng, p, w, wf >> 1 if halved else wf, limit, 60)
            xs.append(mine)
            cs.append((w, wf))
        return xs, cs

    def flat(xs, cs, halved):
        x = [v for mine in xs for v in mine]
        w = [c[0] for mine, c in zip(xs, cs) for _ in mine]
        wf = [(c[1] >> 1 if halved else c[1]) for mine, c in zip(xs, cs) for _ in mine]
        return x, w, wf

    def check(name, x, w, r, bound):
        assert (r - x * w) % p == 0, (name, p, w, hex(x), r)
        assert 0 <= r < bound * p, (name, p, w, hex(x), r // p)

    def addends(plain):
        return [rng.choice([MASK64, (-r) & MASK64, (1 - r) & MASK64, rng.getrandbits(64), 0]) for r in plain]

    # any 64-bit x: shoup_lazy [0, 2p), shoup_mul canonical (2p < 2^64 holds for every modulus of the list)
    xs, cs = gather(any_word, False)
    x, w, wf = flat(xs, cs, False)
    for xi, wi, lazy, canonical in zip(x, w, _eval(probe, 24, [x, w, wf, p]), _eval(probe, 25, [x, w, wf, p])):
        check("shoup_lazy", xi, wi, lazy, 2)
        assert canonical == xi * wi % p, ("shoup_mul", p, wi, hex(xi), canonical)
    # any 64-bit x, 4p < 2^64: lazy4
    if 4 * p < 1 << 64:
        plain = _eval(probe, 30, [x, w, wf, p])
        for xi, wi, r in zip(x, w, plain):
            check("shoup_lazy4", xi, wi, r, 4)
        added = addends(plain)
        assert _eval(probe, 32, [x, w, wf, p, added]) == [(a + r) & MASK64 for a, r in zip(added, plain)]
        for mine, (wi, wfi) in zip(xs, cs):
            plain = _eval(probe, 31, [mine, wi, wfi, p])
            for xi, r in zip(mine, plain):
                check("shoup_lazy4_uniform", xi, wi, r, 4)
            assert plain == _eval(probe, 30, [mine, wi, wfi, p])
            added = addends(plain)
            assert _eval(probe, 33, [mine, wi, wfi, p, added]) == [(a + r) & MASK64 for a, r in zip(added, plain)]
    # x < 2^63 and the halved factor
    xs, cs = gather(below_2_63, True)
    x, w, wf_half = flat(xs, cs, True)
    if 5 * p < 1 << 64:
        plain = _eval(probe, 34, [x, w, wf_half, p])
        for xi, wi, r in zip(x, w, plain):
            check("shoup_headroom", xi, wi, r, 5)
        added = addends(plain)
        assert _eval(probe, 36, [x, w, wf_half, p, added]) == [(a + r) & MASK64 for a, r in zip(added, plain)]
    assert p <= (1 << 62) - 1
    for mine, (wi, wfi) in zip(xs, cs):
        if 5 * p < 1 << 64:
            plain = _eval(probe, 35, [mine, wi, wfi >> 1, p])
            for xi, r in zip(mine, plain):
                check("shoup_headroom_uniform", xi, wi, r, 5)
            assert plain == _eval(probe, 34, [mine, wi, wfi >> 1, p])
            added = addends(plain)
            assert _eval(probe, 37, [mine, wi, wfi >> 1, p, added]) == [(a + r) & MASK64 for a, r in zip(added, plain)]
        for xi, lazy, canonical in zip(mine, _eval(probe, 38, [mine, wi, wfi, p]), _eval(probe, 39, [mine, wi, wfi, p])):
            check("shoup_mul_uniform_lazy", xi, wi, lazy, 3)
            assert canonical == xi * wi % p, ("shoup_mul_uniform", p, wi, hex(xi), canonical)


BARRETT_MODULI = [3, 5, (1 << 16) + 1, (1 << 31) - 1, (1 << 32) - 5, (1 << 32) - 1, (1 << 32) + 1, (1 << 32) + 15, (1 << 40) + 15,
                  (1 << 55) - 55, (1 << 61) - 1, (1 << 62) - 57]


@pytest.mark.parametrize("p", BARRETT_MODULI)
def test_barrett_reduce64(probe, p):
    """barrett_reduce64 and barrett_reduce64_uniform: x mod p for any 64-bit x; _uniform_lazy: [0, 2p) and congruent.  Moduli
    on both sides of 2^32 (2^32 - 5 and 2^32 + 15 among them: the uniform form's branch on hi32(factor)) and down to 3; x at
    the word edges, next to multiples of p and next to the steps of the quotient estimate."""
    rng = random.Random(p)
    factor = (1 << 64) // p
    x = sorted(set(cases.WORD_EDGES + cases.LIMB_WORDS + cases.near_multiples(p, 1 << 64) + cases.quotient_steps(factor, 1 << 64)))
    x += [rng.getrandbits(64) for _ in range(2000)]
    plain, lazy, uniform = _eval(probe, 40, [x, p, factor]), _eval(probe, 41, [x, p, factor]), _eval(probe, 42, [x, p, factor])
    for xi, r, l, u in zip(x, plain, lazy, uniform):
        assert r == xi % p and u == xi % p, (p, hex(xi), r, u)
        assert (l - xi) % p == 0 and 0 <= l < 2 * p, (p, hex(xi), l)


def test_barrett_mul(probe):
    """barrett_mul(x, y) = x y mod p for canonical x, y in {0, 1, p - 1, ...} and random, factor = floor(2^(bits + 62) / p)."""
    rng = random.Random(105)
    x, y, ps, factors, shifts = [], [], [], [], []
    for p in BARRETT_MODULI + [(1 << 62) - 1]:
        ends = [0, 1, 2, p - 1, p - 2, p >> 1, (p >> 1) + 1] + [rng.randrange(p) for _ in range(12)]
        a, b = cases.crossed(ends, ends)
        a, b = a + [rng.randrange(p) for _ in range(300)], b + [rng.randrange(p) for _ in range(300)]
        x, y, ps = x + a, y + b, ps + [p] * len(a)
        factors += [(1 << (p.bit_length() + 62)) // p] * len(a)
        shifts += [p.bit_length() - 2] * len(a)
    assert max(factors) <= MASK64
    for xi, yi, p, r in zip(x, y, ps, _eval(probe, 43, [x, y, ps, factors, shifts])):
        assert r == xi * yi % p, (p, xi, yi, r)


def test_barrett_reduce128(probe):
    """barrett_reduce128(x) = x mod p for any 128-bit x, factor = floor(2^128 / p) in two words: both words of x over the
    edges, and x = k p - 1, k p, k p + 1 next to 2^128."""
    rng = random.Random(106)
    lo, hi, ps = [], [], []
    for p in BARRETT_MODULI + [(1 << 62) - 1]:
        a, b = cases.crossed(cases.WORD_EDGES, cases.WORD_EDGES)
        values = [(h << 64) | l for l, h in zip(a, b)] + cases.near_multiples(p, 1 << 128) + [rng.getrandbits(128) for _ in range(300)]
        lo, hi, ps = lo + [v & MASK64 for v in values], hi + [v >> 64 for v in values], ps + [p] * len(values)
    factors = [(1 << 128) // p for p in ps]
    got = _eval(probe, 44, [lo, hi, ps, [f & MASK64 for f in factors], [f >> 64 for f in factors]])
    for l, h, p, r in zip(lo, hi, ps, got):
        assert r == ((h << 64) | l) % p, (p, hex(h), hex(l), r)


FULL_SUM_KINDS = [60, 61, 63, 65] + [67 + 2 * k for k in range(6)] + [79, 81, 82]
NARROW_SUM_KINDS = [62, 64, 66] + [68 + 2 * k for k in range(6)]
SHORT_SUM_KINDS = [80, 83]
UNIFORM_SUM_KINDS = [79, 80, 82, 83]


def _check_sums(kind, got, a, b, modulus=1 << 128):
    """Every sum of every lane: product_sum_value and the raw fields both give that sum's own reference."""
    for j, lanes in enumerate(got):
        for i, (t, c, h, t_carry, c_carry, lo, hi) in enumerate(lanes):
            expected = sum(int(a[j][k][i]) * int(b[k][i]) for k in range(len(b)))
            assert expected < modulus or modulus == 1 << 128
            assert (hi << 64) | lo == expected % (1 << 128), (kind, j, i, len(b))
            assert cases.field_value(t, c, h, t_carry, c_carry) == expected % (1 << 128), (kind, j, i, len(b))


@pytest.mark.parametrize("kind", FULL_SUM_KINDS)
def test_product_sum_accumulation(probe, kind):
    """The accumulations that count every carry: each sum = its own sum of a_k b_k (mod 2^128) for 1, 2, 3, 63, 64, 65 and 300
    terms of all-ones words, words with all-ones low limbs (every term carries out of t and of c), zeros and random words.
    Every sum of a pair / triple / _add_all gets its own a, so that a swapped operand index shows."""
    rng = random.Random(kind)
    sums = probe.arith_probe_product_sum_sums(kind)
    for terms in cases.SUM_TERMS:
        names = list(cases.sum_operand_classes(rng, terms))
        drawn = [cases.sum_operand_classes(rng, terms) for _ in range(sums)]
        b_lane = drawn[0]
        # one lane per operand class; the wave-uniform kinds read lane 0's b, so they take one class per launch
        groups = [[name] for name in names] if kind in UNIFORM_SUM_KINDS else [names]
        for group in groups:
            a = [[[drawn[j][name][0][k] for name in group] for k in range(terms)] for j in range(sums)]
            b = [[b_lane[name][1][k] for name in group] for k in range(terms)]
            got = _accumulate(probe, kind, a, b)
            _check_sums(kind, got, a, b)
            if "low limbs ones" in group and terms >= 3 and kind not in (81, 82):
                t_carry, c_carry = got[0][group.index("low limbs ones")][3:5]
                assert t_carry > 0 and c_carry > 0  # both counters are driven


@pytest.mark.parametrize("kind", NARROW_SUM_KINDS)
def test_product_sum_narrow_limits(probe, kind):
    """The NARROW accumulations (operands below 2^56, at most 127 terms, no carry count on the middle column): every operand at
    2^56 - 1 at the callers' cadence of 64 terms and at the stated limit of 127 -- the value is exact -- and random operands
    below 2^56 at the smaller term counts, each sum with its own a."""
    rng = random.Random(kind)
    sums = probe.arith_probe_product_sum_sums(kind)
    for terms in (1, 2, 3, 63, 64, 65, 127):
        top = cases.NARROW_WORD
        lanes = [lambda: top, lambda: rng.getrandbits(56), lambda: (rng.getrandbits(24) << 32) | MASK32, lambda: rng.choice([0, top])]
        a = [[[draw() for draw in lanes] for _ in range(terms)] for _ in range(sums)]
        b = [[draw() for draw in lanes] for _ in range(terms)]
        got = _accumulate(probe, kind, a, b)
        _check_sums(kind, got, a, b, modulus=127 << 112)
        if terms in (64, 127):
            assert all(((lanes_[0][6] << 64) | lanes_[0][5]) == terms * top * top for lanes_ in got)


@pytest.mark.parametrize("kind", SHORT_SUM_KINDS)
def test_product_sum_short_limits(probe, kind):
    """The _short accumulations (b wave-uniform, no carry count on the middle column) while
    terms (hi32(a_max) + hi32(b_max) + 2) <= 2^32: at equality and just under it with all-ones low limbs, and the case the header
    names, four 55-bit residues times 61-bit constants."""
    rng = random.Random(kind)
    for a_max, b_max, terms in cases.short_sum_cases():
        assert terms * ((a_max >> 32) + (b_max >> 32) + 2) <= 1 << 32
        below = lambda: (rng.randrange((a_max >> 32) + 1) << 32) | rng.getrandbits(32)
        a = [[[a_max, below(), (rng.randrange((a_max >> 32) + 1) << 32) | MASK32] for _ in range(terms)]]
        b = [[b_max] * 3 for _ in range(terms)]
        _check_sums(kind, _accumulate(probe, kind, a, b), a, b)
        if terms <= 300:  # constants that differ from term to term, still wave-uniform and inside the bound
            b = [[(rng.randrange((b_max >> 32) + 1) << 32) | MASK32] * 3 for _ in range(terms)]
            _check_sums(kind, _accumulate(probe, kind, a, b), a, b)


def test_product_sum_value_any_fields(probe):
    """product_sum_value = t + c 2^32 + (h + t_carry + c_carry 2^32) 2^64 (mod 2^128) for any field values: each at 0, all
    ones and random, in every combination."""
    rng = random.Random(107)
    wide = [0, MASK64, MASK32, MASK32 << 32, rng.getrandbits(64)]
    narrow = [0, MASK32, 1, rng.getrandbits(32)]
    fields = [(t, c, h, tc, cc) for t in wide for c in wide for h in wide for tc in narrow for cc in narrow]
    fields += [(rng.getrandbits(64), rng.getrandbits(64), rng.getrandbits(64), rng.getrandbits(32), rng.getrandbits(32))
               for _ in range(2000)]
    lo, hi = _eval(probe, 45, [list(column) for column in zip(*fields)], outputs=2)
    for f, l, h in zip(fields, lo, hi):
        assert (h << 64) | l == cases.field_value(*f), [hex(v) for v in f]


def _representations(rng, values):
    fields, owners = [], []
    for value in values:
        for f in cases.field_representations(rng, value):
            fields.append(f)
            owners.append(value)
    return [list(column) for column in zip(*fields)], owners


@pytest.mark.parametrize("p", [3, (1 << 31) - 1] + cases.SHOUP_MODULI[2:] + [(1 << 62) - 1])
def test_reduce_product_sum(probe, p):
    """reduce_product_sum: the canonical residue of a value below 2^127 (p <= 2^62 - 1); reduce_product_sum_lazy (5p < 2^64):
    [0, 5p) and congruent.  The same value comes through several representations (c and both carry counts in use)."""
    rng = random.Random(p)
    limit = 1 << 127
    values = sorted({0, 1, p, MASK64, 1 << 64, limit - 1, limit - (1 << 64), (limit - 1) & ~MASK64, ((1 << 63) - 1) << 64})
    values += cases.near_multiples(p, limit) + [(h << 64) | l for l in cases.LIMB_WORDS[::3] for h in cases.LIMB_WORDS[::3] if h < 1 << 63]
    values += [rng.randrange(limit) for _ in range(500)]
    columns, owners = _representations(rng, values)
    m = cases.ReduceModulus(p)
    for value, r in zip(owners, _eval(probe, 46, columns + m.columns())):
        assert r == value % p, (p, hex(value), r)
    if 5 * p < 1 << 64:
        for value, r in zip(owners, _eval(probe, 47, columns + m.columns())):
            assert (r - value) % p == 0 and 0 <= r < 5 * p, (p, hex(value), r // p)


@pytest.mark.parametrize("p", cases.BOUNDED_MODULI)
def test_reduce_product_sum_bounded(probe, p):
    """reduce_product_sum_bounded_lazy for 2^33 < p < 2^61 and a value below 2^(64 + sh), sh = bits(p) - 1: [0, 5p) and congruent;
    reduce_product_sum_bounded: canonical.  Values at 2^(64 + sh) - 1, at k p - 1 and k p for the largest k, with the low word
    all ones, and random; each through several representations."""
    assert 1 << 33 < p < 1 << 61
    rng = random.Random(p)
    m = cases.ReduceModulus(p)
    assert m.wide_factor <= MASK64 and 32 <= m.wide_shift <= 60
    columns, owners = _representations(rng, cases.bounded_values(rng, p, 1500))
    assert max(owners) == (1 << (64 + m.wide_shift)) - 1
    for value, lazy, canonical in zip(owners, _eval(probe, 48, columns + m.columns()), _eval(probe, 49, columns + m.columns())):
        assert (lazy - value) % p == 0 and 0 <= lazy < 5 * p, (p, hex(value), lazy // p)
        assert canonical == value % p, (p, hex(value), canonical)


@pytest.mark.parametrize("p", cases.WORD32_MODULI)
def test_word32_products(probe, p):
    """shoup32_lazy: [0, 2p) and congruent to x w for ANY 32-bit x (p <= 2^30 - 1, wf = floor(w 2^32 / p));
    shoup32_lazy_mad<false / true>: the same word as shoup32_lazy."""
    rng = random.Random(p)
    ws = sorted(set(_constants(rng, p, 14)))
    words = sorted(set(cases.WORD32_EDGES + [v for v in cases.near_multiples(p, 1 << 32)]))
    x, w = cases.crossed(words + [rng.getrandbits(32) for _ in range(300)], ws)
    wf = [(c << 32) // p for c in w]
    plain = _eval(probe, 50, [x, w, wf, p])
    for xi, wi, r in zip(x, w, plain):
        assert (r - xi * wi) % p == 0 and 0 <= r < 2 * p, (p, wi, hex(xi), r)
    assert _eval(probe, 51, [x, w, wf, p]) == plain
    for wi in ws:
        mine = [xi for xi, c in zip(x, w) if c == wi]
        expected = [r for r, c in zip(plain, w) if c == wi]
        assert _eval(probe, 52, [mine, wi, (wi << 32) // p, p]) == expected, (p, wi)
