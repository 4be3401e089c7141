"""fold_mul_signed (csrc/device_math.hpp) and the signed lazy schedule built on it (ntt_common.hpp kModeFoldSigned), checked in
Python integers: the instruction sequence limb by limb (tests/fold_signed_model.py), never as y * w % p.  No GPU.

Moduli: every eligible modulus generate_primes returns for the parameter sets the repository runs, plus the eligibility edges
b = 41 and b = 55 with d = 1 and with the largest eligible d = 2^(b-32) - 1 (these need not be prime: the identities hold for
every odd 2^b - d).  Multiplicands: the ends of [-2^62, 2^62), the words around zero, low words 0 and 0xFFFFFFFF, random
words.  Constants: 0, 1, p - 1 and constants whose second word w 2^32 mod p has the low limb 0x7FFFFFFF, 0x80000000 or
0xFFFFFFFF (where the signed-limb form borrows or does not)."""
import random

import pytest

import fold_signed_model as M

# (degree, bit sizes) of the contexts the benchmark, smoke() and bench_tools/param_sets_bench.py build
PARAMETER_SETS = [(8192, [55, 55, 55, 55]), (8192, [55] * 5), (8192, [55] * 6), (4096, [55, 55]), (16384, [55] * 7),
                  (32768, [55] * 7), (8192, [29, 60, 60]), (8192, [40, 60, 60]), (4096, [60, 60, 60]), (8192, [40, 40, 40, 41]),
                  # (a prime 1 mod 2N lies at least 2N - 1 below 2^b: at N = 8192 the small sizes yield no eligible modulus)
                  (8192, [41]), (4096, [44, 45, 46]), (8192, [46, 47, 48, 49]), (8192, [50, 51, 52, 53, 54])]


def _edges():
    out = []
    for b in (41, 55):
        out += [(1 << b) - 1, (1 << b) - ((1 << (b - 32)) - 1)]
    return out


@pytest.fixture(scope="module")
def moduli():
    import oracle

    found = set()
    for degree, bits in PARAMETER_SETS:
        found.update(int(p) for p in oracle.generate_primes(bits, False, degree) if M.eligible(int(p)))
    assert sum(p.bit_length() == 55 for p in found) >= 7, sorted(found)  # the benchmark's primes are among them
    return sorted(found) + _edges()


def constants_for(p):
    """(w, signed limbs of w 2^32 mod p)"""
    inverse = pow(1 << 32, -1, p)
    ws = [0, 1, p - 1]
    for low in (0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        highs = {0, (p >> 32) - 1, (p >> 33)}
        for high in highs:
            wt = (high << 32) | low
            assert wt < p
            ws.append(wt * inverse % p)
    rng = random.Random(p)
    ws += [rng.randrange(p) for _ in range(3)]
    return [(w, M.signed_limbs(M.second_word(w, p))) for w in ws]


def multiplicands(rng, count):
    edge = [M.WORD_LO, M.WORD_LO + 1, -1, 0, 1, M.WORD_HI - 1]
    for high in (-(1 << 30), -1, 0, 1, (1 << 30) - 1, -12345, 0x2AAAAAAA):
        edge += [high << 32, (high << 32) | 0xFFFFFFFF]
    assert all(M.WORD_LO <= y < M.WORD_HI for y in edge)
    return edge + [rng.randrange(M.WORD_LO, M.WORD_HI) for _ in range(count)]


def test_bias_is_the_multiple_of_p_just_above_2_61(moduli):
    for p in moduli:
        c = M.Constants(p)
        assert c.signed_bias == p * (((1 << 61) + 1 + p - 1) // p)
        assert c.signed_bias % p == 0 and (1 << 61) <= c.signed_bias < (1 << 61) + p


def test_signed_limbs_are_the_table_convention(moduli):
    for p in moduli:
        for w, limbs in constants_for(p):
            wt = M.second_word(w, p)
            t0s, t1 = M.s32(limbs), limbs >> 32
            assert t0s + (t1 << 32) == wt and limbs & M.M32 == wt & M.M32
            assert 0 <= t1 <= 1 << (p.bit_length() - 32)


def test_product_limb_by_limb(moduli):
    covered = {0x7FFFFFFF: 0, 0x80000000: 0, 0xFFFFFFFF: 0}
    for p in moduli:
        c = M.Constants(p)
        assert -p < c.r_lo and c.r_hi < 6 * p  # the range stated in device_math.hpp, inside the (-p, 6p) the schedule uses
        rng = random.Random(p ^ 0x5EED)
        for w, limbs in constants_for(p):
            if limbs & M.M32 in covered:
                covered[limbs & M.M32] += 1
            for y in multiplicands(rng, 300):
                trace = {}
                r = M.fold_mul_signed(y, w, limbs, c, trace)
                where = (p, w, y)
                assert 0 < trace["a"] < 1 << 63, where
                assert 0 <= trace["column0"] < 1 << 65, where
                assert trace["u_carry"] == 0 and abs(trace["u"]) < 1 << 63, where
                assert abs(trace["u"]) < 1 << 56, where
                assert -(1 << 31) <= trace["high"] < 1 << 31 and trace["high"] == trace["high_word"], where
                assert c.high_lo <= trace["high"] <= c.high_hi, where
                assert r == trace["r"], where  # the last multiply-add does not wrap
                assert (r - y * w) % p == 0, where
                assert c.r_lo <= r <= c.r_hi and -p < r < 6 * p, where
    assert all(covered.values()), covered


@pytest.mark.parametrize("log_n", [12, 13])
def test_forward_words_stay_in_range(moduli, log_n):
    """signed words through every stage: inside [-2^62, 2^62) as multiplicands; the final lift by 2^7 p lands in [0, 2^10 p)"""
    for p in moduli:
        c = M.Constants(p)
        intervals = M.forward_intervals(c, log_n)
        for lo, hi in intervals:
            assert M.WORD_LO <= lo and hi < M.WORD_HI, (p, lo, hi)
            assert -(1 + 6 * log_n) * p < lo and hi < (1 + 6 * log_n) * p
        lo, hi = intervals[-1]
        lift = p << M.LIFT_LOG
        assert 0 <= lo + lift and hi + lift < p << M.REDUCER_LOG and hi + lift < 1 << 64


@pytest.mark.parametrize("log_n", [12, 13])
def test_inverse_words_stay_in_range(moduli, log_n):
    """up to every re-bias point: words below their stage's bound in magnitude, differences inside [-2^62, 2^62), the biased
    sums non-negative and inside what the reducer / the division by N take"""
    for p in moduli:
        c = M.Constants(p)
        stages = M.inverse_stages(c, log_n)
        assert len(stages) == log_n
        for stage in stages[:-1]:
            bound = p << stage["in_shift"]
            lo, hi = stage["words"]
            assert -bound < lo and hi < bound, (p, stage)
            assert M.WORD_LO <= stage["diff"][0] and stage["diff"][1] < M.WORD_HI, (p, stage)
            if stage["fold"]:
                assert 0 <= stage["biased_sum"][0] and stage["biased_sum"][1] < p << M.REDUCER_LOG, (p, stage)
        last = stages[-1]
        bound = p << last["in_shift"]
        assert -bound < last["words"][0] and last["words"][1] < bound
        for lo, hi in (last["sum"], last["diff"]):
            # divide_by_degree takes x < 2^9 p; the last product (split_mul_add) any 64-bit word
            assert 0 <= lo and hi < p << 9 and hi < 1 << 64, (p, last)
