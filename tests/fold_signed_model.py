"""Python-integer model of csrc/device_math.hpp fold_mul_signed, instruction by instruction, and of the signed lazy schedule
(ntt_common.hpp kModeFoldSigned) as worst-case intervals.  Shared by tests/test_fold_signed_bounds.py (no GPU) and
tests/test_gpu_fold_signed_probe.py (the device's results word for word)."""

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
WORD_LO, WORD_HI = -(1 << 62), 1 << 62  # the multiplicand's range [-2^62, 2^62)


def s32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def s64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def eligible(p):
    """p = 2^b - d with 41 <= b <= 55 and d < 2^(b-32): DeviceModulus::split_shift != 0 (poly_context.cpp)"""
    b = p.bit_length()
    return 41 <= b <= 55 and (1 << b) - p < (1 << (b - 32))


class Constants:
    """device_math.hpp fold_constants<false>(p)"""

    def __init__(self, p):
        assert eligible(p), p
        self.p, self.b = p, p.bit_length()
        self.d = (1 << self.b) - p
        self.multiplier = 4 * self.d
        self.shift = self.b - 30
        self.mask = (1 << self.shift) - 1
        self.signed_bias = (p << (61 - self.b)) + p  # K
        # the product's range, derived in device_math.hpp: high = u >> shift lies in [-2^28, 2^30 + 2^28 + 2^(63-b)]
        self.high_lo, self.high_hi = -(1 << 28), (1 << 30) + (1 << 28) + (1 << (63 - self.b))
        self.r_lo = self.high_lo * self.multiplier                                # inclusive
        self.r_hi = (1 << (self.b + 2)) - 1 + self.high_hi * self.multiplier       # inclusive


def signed_limbs(wt):
    """(t0s | t1' << 32) as PolyContext::upload stores it: the same low word, t1' = hi32(wt) + (lo32(wt) >> 31)"""
    return (wt + ((wt & 0x80000000) << 1)) & M64


def second_word(w, p):
    return (w << 32) % p


def mad_u64_u32(a, b, c):
    """-> (64-bit result, carry-out)"""
    assert 0 <= a <= M32 and 0 <= b <= M32 and 0 <= c <= M64
    full = a * b + c
    return full & M64, full >> 64


def mad_i64_i32(a, b, c):
    """signed 32 x 32 + 64 -> the low 64 bits (as an unsigned pattern) and the exact value"""
    exact = s32(a) * s32(b) + s64(c)
    return exact & M64, exact


def fold_mul_signed(y, w, wt_limbs, c, trace=None):
    """y: a Python integer in [-2^62, 2^62); w: the constant; wt_limbs: signed_limbs(w 2^32 mod p).  Returns r as a signed
    integer (the device's 64-bit two's-complement word).  `trace`: a dict that receives the intermediate exact values."""
    word = y & M64
    b0, b1 = word & M32, word >> 32
    w0, w1, t0, t1 = w & M32, w >> 32, wt_limbs & M32, wt_limbs >> 32
    a, a_exact = mad_i64_i32(b1, t0, c.signed_bias)
    t, carry = mad_u64_u32(b0, w0, a)
    u = (t >> 32) | (carry << 32)
    u, u_carry = mad_u64_u32(b0, w1, u)
    u, u_exact = mad_i64_i32(b1, t1, u)
    high = ((u >> c.shift) & M32)  # v_alignbit_b32(hi32(u), lo32(u), shift): bits [shift, shift + 32) of u
    kept = (u & M32) & c.mask
    r, r_exact = mad_i64_i32(high, c.multiplier, (t & M32) | (kept << 32))
    if trace is not None:
        trace.update(a=a_exact, column0=b0 * w0 + a_exact, u=u_exact, u_carry=u_carry, high=s64(u) >> c.shift,
                     high_word=s32(high), r=r_exact)
    return s64(r)


# ---- the schedule, as intervals [lo, hi] (inclusive) of the signed words ---------------------------------------------------
LIFT_LOG = 7            # canonicalize_all: forward words + 2^7 p in front of the reducer
INVERSE_CAP_LOG = 6     # Lazy<kModeFoldSigned>::kInverseCapLog
PRODUCT_LOG = 3         # Lazy<>::kProductLog
REDUCER_LOG = 10        # LazyReducer takes x < 2^10 p


def inverse_in_shift(b):
    """ntt_common.hpp inverse_in_shift for the split modes"""
    shift = 0
    for _ in range(b):
        sums = 1 if shift + 1 > INVERSE_CAP_LOG else shift + 1
        shift = max(sums, PRODUCT_LOG)
    return shift


def forward_intervals(c, log_n):
    """[(lo, hi)] of the words entering each stage and, last, leaving the transform"""
    lo, hi = 0, c.p - 1
    out = [(lo, hi)]
    for _ in range(log_n):
        lo, hi = min(lo + c.r_lo, lo - c.r_hi), max(hi + c.r_hi, hi - c.r_lo)
        out.append((lo, hi))
    return out


def inverse_stages(c, log_n):
    """per stage below the last: dict(b, in_shift, fold, words, diff, biased_sum); then the last stage's dict(b, in_shift, words, sum,
    diff) with the bias 2 bound added -- all as inclusive intervals"""
    p = c.p
    lo, hi = 0, p - 1
    stages = []
    for b in range(log_n):
        in_shift = 0 if b == 0 else inverse_in_shift(b)
        bound = p << in_shift
        diff = (lo - hi, hi - lo)
        total = (2 * lo, 2 * hi)
        if b == log_n - 1:
            stages.append(dict(b=b, in_shift=in_shift, words=(lo, hi), sum=(total[0] + 2 * bound, total[1] + 2 * bound),
                               diff=(diff[0] + 2 * bound, diff[1] + 2 * bound)))
            break
        fold = in_shift + 1 > INVERSE_CAP_LOG
        stage = dict(b=b, in_shift=in_shift, fold=fold, words=(lo, hi), diff=diff, biased_sum=None)
        if fold:
            stage["biased_sum"] = (total[0] + 2 * bound, total[1] + 2 * bound)
            total = (0, 2 * p - 1)
        stages.append(stage)
        lo, hi = min(total[0], c.r_lo), max(total[1], c.r_hi)
    return stages
