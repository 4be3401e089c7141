"""The instruction sequences of csrc/device_math.hpp whose output ranges rest on an approximate quotient or on a dropped carry
count, restated limb by limb on Python integers: every "fits its register" claim and every stated range is asserted on the way,
at the operands where it is tightest (tests/device_math_cases.py -- the same classes tests/test_gpu_device_math.py gives the
device).  `mad` is one v_mad_u64_u32: 32 x 32 + 64 -> 64 with a carry-out.

    mulhi64_approx                  floor(a b / 2^64) - 2 <= r <= floor(a b / 2^64)
    shoup_quotient<., false>        x, f < 2^63: the cross column stays inside 64 bits; low by <= 1
    shoup_quotient<., true>         any x, f: the cross column's 65th bit re-enters as bit 32; low by <= 2 (in fact <= 1)
    shoup_lazy4                     any x, 4p < 2^64:  x w - q p in [0, 4p)
    shoup_headroom                  x < 2^63, 5p < 2^64:  x w - q 2p in [0, 5p)
    shoup_mul_uniform_lazy          x < 2^63, p <= 2^62 - 1:  exact quotient by the halved factor, [0, 3p)
    reduce_product_sum_bounded_lazy 2^33 < p < 2^61, value < 2^(64 + sh):  [0, 5p)
    NARROW / _short accumulations   the middle column never wraps inside the stated operand and term bounds
"""
import random

import device_math_cases as cases
from device_math_cases import MASK32, MASK64, MASK128


def mad(a, b, c):
    """v_mad_u64_u32: (low 64 bits, carry-out) of a b + c."""
    assert 0 <= a <= MASK32 and 0 <= b <= MASK32 and 0 <= c <= MASK64
    full = a * b + c
    return full & MASK64, full >> 64


def limbs(v):
    assert 0 <= v <= MASK64
    return v & MASK32, v >> 32


def mulhi64_approx(a, b):
    a0, a1 = limbs(a)
    b0, b1 = limbs(b)
    p01_hi = (a0 * b1) >> 32
    p10_hi = (a1 * b0) >> 32
    r, carry = mad(a1, b1, p01_hi + p10_hi)
    assert carry == 0, "a1 b1 + two high words is below the exact high word, hence inside 64 bits"
    return r


def shoup_quotient(x, f, carry_form):
    a0, a1 = limbs(x)
    b0, b1 = limbs(f)
    cross, carry = mad(a0, b1, 0)
    assert carry == 0
    cross, carry = mad(a1, b0, cross)
    if not carry_form:
        assert carry == 0, "x, f < 2^63: a0 b1 + a1 b0 never leaves 64 bits"
        carried = 0
    else:
        carried = carry
    q, carry = mad(a1, b1, cross >> 32)
    assert carry == 0
    high = (q >> 32) + carried
    assert high <= MASK32, "the estimate is not above the exact quotient, so the re-entering bit cannot overflow"
    return (high << 32) | (q & MASK32)


def shoup_low64(addend, x, w, q, neg):
    """The low 64 bits of addend + x w + q neg from the two column chains (carries out of either chain are dropped: mod 2^64)."""
    a0, a1 = limbs(x)
    q0, q1 = limbs(q)
    w0, w1 = limbs(w)
    n0, n1 = limbs(neg)
    acc, _ = mad(a0, w0, addend)
    acc, _ = mad(q0, n0, acc)
    high, _ = mad(a0, w1, 0)
    high, _ = mad(a1, w0, high)
    high, _ = mad(q0, n1, high)
    high, _ = mad(q1, n0, high)
    return (acc & MASK32) | ((((acc >> 32) + high) & MASK32) << 32)


def shoup_lazy4(x, w, wf, p, addend=0):
    return shoup_low64(addend, x, w, shoup_quotient(x, wf, True), (-p) & MASK64)


def shoup_headroom(x, w, wf_half, p, addend=0):
    return shoup_low64(addend, x, w, shoup_quotient(x, wf_half, False), (-2 * p) & MASK64)


def shoup_mul_uniform_lazy(x, w, wf, p):
    wf_half = wf >> 1
    a0, a1 = limbs(x)
    b0, b1 = limbs(wf_half)
    low, carry = mad(a0, b0, 0)
    cross, carry = mad(a0, b1, low >> 32)
    assert carry == 0
    cross, carry = mad(a1, b0, cross)
    assert carry == 0, "a0 b1 + a1 b0 + hi32(a0 b0) < 2^64 for x, wf_half < 2^63"
    q, carry = mad(a1, b1, cross >> 32)
    assert carry == 0
    assert q == (x * wf_half) >> 64, "the quotient by the halved factor is exact"
    return shoup_low64(0, x, w, q, (-2 * p) & MASK64)


def product_sum_value(t, c, h, t_carry, c_carry):
    lo = (t + (c << 32)) & MASK64
    hi = (h + t_carry + (c >> 32) + (c_carry << 32) + ((t + ((c << 32) & MASK64)) >> 64)) & MASK64
    return lo, hi


def reduce_product_sum_bounded_lazy(fields, m):
    lo, hi = product_sum_value(*fields)
    sh = m.wide_shift
    assert 32 <= sh <= 60 and m.wide_factor <= MASK64
    value = (hi << 64) | lo
    assert value >> (64 + sh) == 0, "precondition: the sum is below 2^(64 + sh)"
    shift = sh - 32
    x0 = (((hi & MASK32) << 32 | (lo >> 32)) >> shift) & MASK32  # v_alignbit_b32(lo32(hi), hi32(lo), shift)
    x1 = (((hi >> 32) << 32 | (hi & MASK32)) >> shift) & MASK32
    x = (x1 << 32) | x0
    assert x == value >> sh, "T >> sh fits a word"
    q = shoup_quotient(x, m.wide_factor, True)
    exact = value // m.p
    assert exact - 4 <= q <= exact, (exact - q)
    q0, q1 = limbs(q)
    n0, n1 = limbs((-m.p) & MASK64)
    c0, _ = mad(q0, n0, lo)
    c1, _ = mad(q0, n1, 0)
    c1, _ = mad(q1, n0, c1)
    return (c0 & MASK32) | ((((c0 >> 32) + c1) & MASK32) << 32)


class Sum:
    """ProductSum: sum = t + c 2^32 + (h + t_carry + c_carry 2^32) 2^64; h may wrap (mod 2^128)."""

    def __init__(self):
        self.t = self.c = self.h = self.t_carry = self.c_carry = 0

    def add(self, a, b, count_cross_carries):
        a0, a1 = limbs(a)
        b0, b1 = limbs(b)
        self.t, carry = mad(a0, b0, self.t)
        self.t_carry += carry
        self.c, carry = mad(a0, b1, self.c)
        if count_cross_carries:
            self.c_carry += carry
        else:
            assert carry == 0, "the middle column wrapped although its carry is not counted"
        self.c, carry = mad(a1, b0, self.c)
        if count_cross_carries:
            self.c_carry += carry
        else:
            assert carry == 0, "the middle column wrapped although its carry is not counted"
        self.h = (self.h + a1 * b1) & MASK64
        assert self.t_carry <= MASK32 and self.c_carry <= MASK32

    def fields(self):
        return self.t, self.c, self.h, self.t_carry, self.c_carry

    def value(self):
        lo, hi = product_sum_value(*self.fields())
        return (hi << 64) | lo


# ---- the tests --------------------------------------------------------------------------------------------------------


def test_mulhi64_approx_is_low_by_at_most_two():
    rng = random.Random(11)
    words = cases.LIMB_WORDS + cases.WORD_EDGES + cases.CARRY_WORDS
    pairs = [(a, b) for a in words for b in words] + [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(4000)]
    worst = 0
    for a, b in pairs:
        exact = (a * b) >> 64
        r = mulhi64_approx(a, b)
        assert exact - 2 <= r <= exact, (hex(a), hex(b))
        worst = max(worst, exact - r)
    assert worst == 2, "the operand classes reach the stated bound"


def test_shoup_quotient_without_carry_is_low_by_at_most_one():
    rng = random.Random(12)
    words = [x for x in cases.LIMB_WORDS + cases.WORD_EDGES if x < 1 << 63]
    pairs = [(x, f) for x in words for f in words] + [(rng.getrandbits(63), rng.getrandbits(63)) for _ in range(4000)]
    worst = 0
    for x, f in pairs:
        exact = (x * f) >> 64
        q = shoup_quotient(x, f, False)
        assert exact - 1 <= q <= exact, (hex(x), hex(f))
        worst = max(worst, exact - q)
    assert worst == 1


def test_shoup_quotient_with_carry_any_words():
    rng = random.Random(13)
    words = cases.LIMB_WORDS + cases.WORD_EDGES + cases.CARRY_WORDS
    pairs = [(x, f) for x in words for f in words] + [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(4000)]
    carried = 0
    for x, f in pairs:
        exact = (x * f) >> 64
        q = shoup_quotient(x, f, True)
        assert exact - 2 <= q <= exact, (hex(x), hex(f))
        a0, a1 = limbs(x)
        b0, b1 = limbs(f)
        carried += (a0 * b1 + a1 * b0) >> 64
    assert carried > 50, "the operand classes drive the 65th bit of the cross column"


def _shoup_cases(rng, limit_of, moduli):
    for p in moduli:
        limit = limit_of(p)
        if limit is None:
            continue
        for w in cases.shoup_constants(p) + [rng.randrange(p) for _ in range(3)]:
            wf = cases.shoup_factor(w, p)
            yield p, w, wf, limit


def test_shoup_lazy4_stays_below_4p():
    rng = random.Random(14)
    for p, w, wf, limit in _shoup_cases(rng, lambda p: 1 << 64 if 4 * p < 1 << 64 else None, cases.SHOUP_MODULI):
        worst = 0
        for x in cases.shoup_operands(rng, p, w, wf, limit, 50):
            r = shoup_lazy4(x, w, wf, p)
            assert r % p == x * w % p and 0 <= r < 4 * p, (p, w, hex(x), r // p)
            worst = max(worst, r // p)
            addend = rng.choice([MASK64, r, rng.getrandbits(64)])
            assert shoup_lazy4(x, w, wf, p, addend) == (addend + r) & MASK64
        assert worst <= 2, "in fact below 3p: Shoup's exact estimate leaves [0, 2p), the dropped column costs one p more"


def test_shoup_headroom_stays_below_5p():
    rng = random.Random(15)
    seen = 0
    for p, w, wf, limit in _shoup_cases(rng, lambda p: 1 << 63 if 5 * p < 1 << 64 else None, cases.SHOUP_MODULI):
        for x in cases.shoup_operands(rng, p, w, wf >> 1, limit, 50):
            r = shoup_headroom(x, w, wf >> 1, p)
            assert r % p == x * w % p and 0 <= r < 5 * p, (p, w, hex(x), r // p)
            seen = max(seen, r // p)
            addend = rng.choice([MASK64, r, rng.getrandbits(64)])
            assert shoup_headroom(x, w, wf >> 1, p, addend) == (addend + r) & MASK64
    assert seen >= 3, "the operand classes leave the canonical and the 2p ranges"


def test_shoup_mul_uniform_lazy_stays_below_3p():
    rng = random.Random(16)
    seen = 0
    for p, w, wf, limit in _shoup_cases(rng, lambda p: 1 << 63, cases.SHOUP_MODULI):
        assert p <= (1 << 62) - 1
        for x in cases.shoup_operands(rng, p, w, wf >> 1, limit, 50):
            r = shoup_mul_uniform_lazy(x, w, wf, p)
            assert r % p == x * w % p and 0 <= r < 3 * p, (p, w, hex(x), r // p)
            seen = max(seen, r // p)
    assert seen == 2


def test_reduce_product_sum_bounded_lazy_stays_below_5p():
    rng = random.Random(17)
    for p in cases.BOUNDED_MODULI:
        assert 1 << 33 < p < 1 << 61
        m = cases.ReduceModulus(p)
        for value in cases.bounded_values(rng, p, 300):
            for fields in cases.field_representations(rng, value):
                assert cases.field_value(*fields) == value
                r = reduce_product_sum_bounded_lazy(fields, m)
                assert r % p == value % p and 0 <= r < 5 * p, (p, hex(value), r // p)


def test_product_sum_value_of_any_fields():
    rng = random.Random(18)
    edges = [0, MASK64, rng.getrandbits(64)]
    edges32 = [0, MASK32, rng.getrandbits(32)]
    for t in edges:
        for c in edges:
            for h in edges:
                for t_carry in edges32:
                    for c_carry in edges32:
                        lo, hi = product_sum_value(t, c, h, t_carry, c_carry)
                        assert (hi << 64) | lo == cases.field_value(t, c, h, t_carry, c_carry)


def test_full_accumulation_counts_every_carry():
    rng = random.Random(19)
    for terms in cases.SUM_TERMS:
        for name, (a, b) in cases.sum_operand_classes(rng, terms).items():
            s = Sum()
            for x, y in zip(a, b):
                s.add(x, y, True)
            assert s.value() == sum(x * y for x, y in zip(a, b)) & MASK128, (terms, name)
            if name == "low limbs ones" and terms >= 3:
                assert s.t_carry > 0 and s.c_carry > 0, "this class drives both carry counts"


def test_narrow_accumulation_fits_its_middle_column():
    """Operands below 2^56, at most 127 terms: the uncounted middle column a0 b1 + a1 b0 never wraps."""
    for terms in (int(cases.SUM_TERMS[4]), 127):  # the callers' cadence (kNarrowProductSumCadence = 64) and the stated limit
        s = Sum()
        for _ in range(terms):
            s.add(cases.NARROW_WORD, cases.NARROW_WORD, False)
        assert s.c <= MASK64 and s.c_carry == 0
        assert s.value() == terms * cases.NARROW_WORD * cases.NARROW_WORD


def test_short_accumulation_fits_its_middle_column():
    """terms (hi32(a_max) + hi32(b_max) + 2) <= 2^32: the uncounted middle column never wraps, up to equality."""
    for a_max, b_max, terms in cases.short_sum_cases():
        s = Sum()
        for _ in range(terms):
            s.add(a_max, b_max, False)
        assert s.value() == (terms * a_max * b_max) & MASK128, (hex(a_max), hex(b_max), terms)
