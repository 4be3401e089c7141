"""Operand generators shared by tests/test_device_math_bounds.py (the instruction sequences of csrc/device_math.hpp restated on
Python integers) and tests/test_gpu_device_math.py (the same functions on the device): the words at which an approximate quotient
or a dropped carry costs most.  Constants are computed here from their definitions, never taken from the library's host code."""

MASK32, MASK64, MASK128 = (1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1

WORD_EDGES = [0, 1, 2, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1,
              (1 << 64) - 1, (1 << 64) - 2, (1 << 64) - (1 << 32), (1 << 64) - (1 << 32) - 1, 0xFFFFFFFF00000000, 0x7FFFFFFFFFFFFFFF,
              0x80000000FFFFFFFF, 0x7FFFFFFF00000000, 0x00000000FFFFFFFF]


def operands(rng, count):
    """The 64-bit edge words, then random words up to `count`."""
    return WORD_EDGES + [rng.getrandbits(64) for _ in range(count - len(WORD_EDGES))]


def constants(rng, p, count):
    """Constants at the ends and the middle of [0, p), then random ones up to `count`."""
    edges = [0, 1, 2, p - 1, p - 2, p >> 1, (p >> 1) + 1, (1 << 31) % p, (1 << 32) % p, ((1 << 32) - 1) % p]
    return edges + [rng.randrange(p) for _ in range(count - len(edges))]


def crossed(first, second):
    """Every element of `first` against every element of `second`, as two parallel lists."""
    return [x for x in first for _ in second], [y for _ in first for y in second]


# limbs that maximise (all ones), straddle (top bit alone, all but the top bit) or remove (0, 1) the carries between columns
LIMB_EDGES = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
LIMB_WORDS = [(high << 32) | low for high in LIMB_EDGES for low in LIMB_EDGES]

# x and f with both top bits set and all-ones low limbs: the 65th bit of shoup_quotient<., true>'s cross column
CARRY_WORDS = [MASK64, 0x80000000FFFFFFFF, 0xC0000000FFFFFFFF, 0xFFFFFFFEFFFFFFFF, 0xFFFFFFFFFFFFFFFE, 0x8000000100000000 | MASK32,
               0xFFFFFFFF80000000, 0xFFFFFFFF00000001]

# odd, not all prime: the products use nothing of a modulus but its size and oddness
SHOUP_MODULI = [(1 << 20) + 7, (1 << 31) - 1, (1 << 32) - 5, (1 << 32) + 15, (1 << 40) + 15, (1 << 55) - 55, (1 << 60) - 93,
                (1 << 61) - 1, (1 << 62) - 57]


def shoup_factor(w, p):
    return (w << 64) // p


def shoup_constants(p):
    """w at the ends of [0, p) and at floor(p / 2) +- 1."""
    return sorted({0, 1, 2, p - 2, p - 1, p // 2 - 1, p // 2, p // 2 + 1})


def near_multiples(p, limit):
    """k p - 1, k p, k p + 1 inside [0, limit) for small k, the largest k that fits and a few on the way."""
    top = (limit - 1) // p
    ks = {0, 1, 2, 3, 4, 5, top // 3, top // 2, top - 2, top - 1, top}
    return sorted({x for k in ks if k >= 0 for x in (k * p - 1, k * p, k * p + 1) if 0 <= x < limit})


def quotient_steps(factor, limit):
    """The words next to floor(j 2^64 / factor) inside [0, limit), small and large j: where floor(x factor / 2^64) steps from
    j - 1 to j, so that an estimate which is low there costs a whole modulus."""
    if factor == 0:
        return []
    top = ((limit - 1) * factor) >> 64
    js = {1, 2, 3, 4, 7, top // 2, top - 2, top - 1, top}
    words = set()
    for j in js:
        if j >= 1:
            step = -((-j << 64) // factor)  # the least x with x factor >= j 2^64
            words.update(x for x in (step - 2, step - 1, step, step + 1) if 0 <= x < limit)
    return sorted(words)


def shoup_operands(rng, p, w, factor, limit, randoms):
    """Adversarial multiplicands below `limit` for the constant w (quotient factor `factor`) and a few random ones."""
    words = set(x for x in WORD_EDGES + LIMB_WORDS + CARRY_WORDS if x < limit)
    words.update(near_multiples(p, limit))
    words.update(quotient_steps(factor, limit))
    if w:
        # x w next to a multiple of p: x = ceil(k p / w) for large k
        for k in (1, 2, (limit - 1) * w // p, (limit - 1) * w // p - 1):
            if k >= 1:
                x = -(-k * p // w)
                words.update(v for v in (x - 1, x, x + 1) if 0 <= v < limit)
    return sorted(words) + [rng.randrange(limit) for _ in range(randoms)]


# ---- sums of products -------------------------------------------------------------------------------------------------

SUM_TERMS = [1, 2, 3, 63, 64, 65, 300]
NARROW_WORD = (1 << 56) - 1


def sum_operand_classes(rng, terms):
    """name -> (a[terms], b[terms]) for one sum: all-ones words (every column at its maximum), words whose LOW limbs are all ones
    (every term carries out of t, every second cross product out of c), zeros and random words."""
    low_ones = lambda: (rng.getrandbits(32) << 32) | MASK32
    return {
        "all ones": ([MASK64] * terms, [MASK64] * terms),
        "low limbs ones": ([low_ones() | (1 << 63) for _ in range(terms)], [low_ones() | (1 << 63) for _ in range(terms)]),
        "all ones times low ones": ([MASK64] * terms, [low_ones() for _ in range(terms)]),
        "zeros": ([0] * terms, [rng.getrandbits(64) for _ in range(terms)]),
        "random": ([rng.getrandbits(64) for _ in range(terms)], [rng.getrandbits(64) for _ in range(terms)]),
    }


def short_sum_cases():
    """(a_max, b_max, terms) with terms (hi32(a_max) + hi32(b_max) + 2) equal to 2^32 or just under it -- the bound of the _short
    accumulations -- with all-ones low limbs; and the case their comment names: four 55-bit residues times 61-bit constants."""
    cases = []
    for terms in (2, 64, 300, 1 << 12):
        budget = (1 << 32) // terms - 2  # hi32(a_max) + hi32(b_max)
        for high_a in (budget // 2, budget, 0, budget - 1):
            high_b = budget - high_a
            assert terms * (high_a + high_b + 2) <= 1 << 32
            cases.append(((high_a << 32) | MASK32, (high_b << 32) | MASK32, terms))
    assert any(terms * ((a >> 32) + (b >> 32) + 2) == 1 << 32 for a, b, terms in cases)
    cases.append(((1 << 55) - 1, (1 << 61) - 1, 4))
    return cases


def field_representations(rng, value):
    """Five-field ProductSum representations (t, c, h, t_carry, c_carry) of one 128-bit value: the plain one and some with the
    middle column and both carry counts in use.  t + c 2^32 + (h + t_carry + c_carry 2^32) 2^64 = value (mod 2^128)."""
    lo, hi = value & MASK64, value >> 64
    reps = [(lo, 0, hi, 0, 0)]
    for c, t_carry, c_carry in ((MASK64, MASK32, MASK32), (rng.getrandbits(64), rng.getrandbits(32), rng.getrandbits(32)),
                                (rng.getrandbits(64), 0, 1), (MASK32 << 32, 1, 0)):
        rest = (value - (c << 32) - ((t_carry + (c_carry << 32)) << 64)) & MASK128
        reps.append((rest & MASK64, c, rest >> 64, t_carry, c_carry))
    for t, c, h, t_carry, c_carry in reps:
        assert (t + (c << 32) + ((h + t_carry + (c_carry << 32)) << 64)) & MASK128 == value
    return reps


def field_value(t, c, h, t_carry, c_carry):
    return (t + (c << 32) + ((h + t_carry + (c_carry << 32)) << 64)) & MASK128


class ReduceModulus:
    """The constants of the `Modulus` parameter of reduce_product_sum*, from their definitions."""

    def __init__(self, p):
        bits = p.bit_length()
        self.p = p
        self.barrett64 = (1 << 64) // p
        self.two64_mod_p = (1 << 64) % p
        self.two64_mod_p_shoup = (self.two64_mod_p << 64) // p
        self.wide_shift = bits - 1
        self.wide_factor = (1 << (64 + bits - 1)) // p

    def columns(self):
        return [self.p, self.barrett64, self.two64_mod_p, self.two64_mod_p_shoup, self.wide_shift, self.wide_factor]


# 2^33 < p < 2^61 (reduce_product_sum_bounded*), next to both ends and next to powers of two on either side
BOUNDED_MODULI = [(1 << 33) + 17, (1 << 34) - 41, (1 << 40) + 15, (1 << 55) - 55, (1 << 60) - 93, (1 << 60) + 33, (1 << 61) - 1]


def bounded_values(rng, p, randoms):
    """128-bit values below 2^(64 + sh), sh = bits(p) - 1: the top of the range, multiples of p and their neighbours, low word all
    ones, and random ones."""
    limit = 1 << (64 + p.bit_length() - 1)
    top = (limit - 1) // p
    values = {0, 1, p - 1, p, limit - 1, limit - 2, limit - (1 << 64), (limit - 1) & ~MASK64, MASK64, (1 << 64), (p << 64) % limit | MASK64}
    for k in (1, 2, top // 2, top - 1, top):
        values.update(v for v in (k * p - 1, k * p, k * p + 1) if 0 <= v < limit)
    for high in (1, (limit >> 64) - 1, (limit >> 65)):
        values.add((high << 64) | MASK64)
    values = sorted(values) + [rng.randrange(limit) for _ in range(randoms)]
    assert all(0 <= v < limit for v in values)
    return values


WORD32_MODULI = [3, (1 << 17) - 1, (1 << 27) - 39, (1 << 30) - 35, (1 << 30) - 1]
WORD32_EDGES = [0, 1, 2, (1 << 15) - 1, 1 << 16, (1 << 30) - 1, 1 << 30, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 2, (1 << 32) - 1]
