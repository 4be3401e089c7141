"""The RNS roundings of the BEHZ toolbox in Python integers, and inputs built to sit on their decision thresholds.

Statement by statement after the reference -- RnsTool.swift (scaleAndRound :272-302, liftQToQBsk :313-368, approximateFloor
and convertApproximateBskToQ :378-450), RnsBaseConverter.swift:97-143 (every sum there is exact, so a conversion is one
`sum(...) % modulus`), Bfv+Encrypt.swift:75-140 (plaintextTranslate), PolyRq.swift:365-393 (divideAndRoundQLast) -- on
Python `int` only.  Imports neither the CPU oracle nor the device package: both are held to what is written here.

Every restatement returns (words, decision) so that a test can assert which side of a comparison a coefficient is on;
every construction returns the residues of ONE coefficient whose decision variable has the asked value.
"""
import random
from fractions import Fraction

import numpy as np

MASK64 = (1 << 64) - 1


def prod(xs):
    out = 1
    for x in xs:
        out *= x
    return out


class Level:
    """One level's _RnsTool constants.  q: this level's ciphertext moduli; bsk_top: the TOP level's Bsk primes (the shared
    RnsToolContext, RnsTool.swift:28-66) -- a level with L moduli sees the first L + 2 of [Bsk..., mTilde] (:185-186)."""

    def __init__(self, q, bsk_top, t, gamma, mtilde):
        self.q, self.t, self.gamma, self.mtilde = list(q), t, gamma, mtilde
        self.L = L = len(self.q)
        self.ext = (list(bsk_top) + [mtilde])[:L + 2]  # at the top level the last one is mTilde, below it a Bsk prime
        self.bsk = self.ext[:L + 1]
        self.b_moduli, self.m_sk = self.bsk[:L], self.bsk[L]
        self.top_m_sk = bsk_top[-1]  # mSkContext: one for every level (:58-62, 241)
        self.Q, self.B = prod(self.q), prod(self.b_moduli)
        self.inv_punctured_q = [pow(self.Q // qi, -1, qi) for qi in self.q]        # CrtComposer.inversePuncturedProducts
        self.inv_punctured_b = [pow(self.B // bi, -1, bi) for bi in self.b_moduli]
        self.neg_inv_q_mod_mtilde = -pow(self.Q, -1, mtilde) % mtilde                 # :159-165
        # :242-246: B mod the shared (top) m_sk, inverted mod THIS level's m_sk
        self.b_mod_msk = self.B % self.top_m_sk
        self.inv_b_mod_msk = pow(self.b_mod_msk, -1, self.m_sk)
        # (Q/q_i) mod an output modulus and (B/Bsk_i) mod one: RnsBaseConverter.puncturedProducts
        self.q_to = {m: [self.Q // qi % m for qi in self.q] for m in self.ext + [t, gamma]}
        self.b_to = {m: [self.B // bi % m for bi in self.b_moduli] for m in self.q + [self.top_m_sk]}
        self.inv_mtilde_mod_bsk = [pow(mtilde, -1, b) for b in self.bsk]              # :221-224
        self.inv_q_mod_bsk = [pow(self.Q, -1, b) for b in self.bsk]                   # :235-239
        self.neg_inv_q_mod_t_gamma = {m: -pow(self.Q, -1, m) % m for m in (t, gamma)}  # :154-157

    # ---- liftQToQBsk ------------------------------------------------------------------------------------------
    def lift_products(self, x):
        """:314 poly * mTildeModQ, then RnsBaseConverter.swift:97-106 convertApproximateProducts."""
        return [xi * (self.mtilde % qi) % qi * inv % qi for xi, qi, inv in zip(x, self.q, self.inv_punctured_q)]

    def lift(self, x):
        """x: L residues -> (2L + 1 words over [q, Bsk], r).  r is the word `r < mTilde/2` is decided on."""
        y = self.lift_products(x)
        conv = [sum(yi * c for yi, c in zip(y, self.q_to[m])) % m for m in self.ext]  # RnsBaseConverter.swift:117-143
        r = conv[self.L + 1] * self.neg_inv_q_mod_mtilde % self.mtilde                  # :343-346
        below = r < self.mtilde >> 1                                                    # :340, 347
        out = list(x)                                                                   # :329
        for j, bsk in enumerate(self.bsk):
            centered = r if below else r + bsk - self.mtilde                            # :357-360
            out.append((conv[j] + self.Q % bsk * centered) * self.inv_mtilde_mod_bsk[j] % bsk)  # :362-363
        return out, r

    def exact_centered_lift(self, x_int):
        """What the lift is FOR at the top level (RnsToolTests.swift:168-208): the centred representative of x over [q, Bsk]."""
        big = self.Q * prod(self.bsk)
        value = big - (self.Q - x_int) if x_int > self.Q // 2 else x_int
        return [value % m for m in self.q + self.bsk]

    def lift_input_with_r(self, rng, target):
        """L residues whose lift has r == target.  r = conv * (-Q^-1) mod mTilde, so conv = target * (-Q^-1)^-1 (mod mTilde),
        and conv = sum_i y_i (Q/q_i) mod `last`.  All y_i but the widest row's are drawn; that one is solved for.
        Top level (last = mTilde): y_w is fixed mod mTilde, plus a random multiple of mTilde below q_w.
        Below it (last = a Bsk prime p): conv = c + mTilde k for some k, so y_w = (c - rest + mTilde k) (Q/q_w)^-1 mod p must
        fall below q_w -- the smallest such k comes from the Euclid-like descent of first_multiple_in_range()."""
        last, M = self.ext[self.L + 1], self.mtilde
        w = max(range(self.L), key=lambda i: self.q[i])
        c = target * pow(self.neg_inv_q_mod_mtilde, -1, M) % M
        for _ in range(64):
            y = [rng.randrange(qi) for qi in self.q]
            rest = sum(y[i] * (self.Q // self.q[i] % last) for i in range(self.L) if i != w)
            inv_w = pow(self.Q // self.q[w], -1, last)
            if last == M:
                y_w = (c - rest) * inv_w % M
                if y_w >= self.q[w]:
                    continue
                y_w += M * rng.randrange((self.q[w] - y_w + M - 1) // M)
            else:
                # y_w(k) = base + k step (mod p), wanted in [0, min(q_w, p)): k step mod p in [-base, -base + width)
                # (with one modulus conv IS y_w: a random start k0 below q_w / mTilde spreads it; with more, `rest` does)
                step, width = M * inv_w % last, min(self.q[w], last)
                k0 = rng.randrange(max(1, (width - c) // M)) if self.L == 1 else 0
                base = ((c - rest) * inv_w + k0 * step) % last
                low = -base % last
                k = 0 if base < width else first_multiple_in_range(step, last, low, low + width - 1)
                if k is None or c + M * (k0 + k) >= last:
                    continue
                y_w = (base + k * step) % last
            y[w] = y_w
            # back from the products to the residues: x_i = y_i (Q/q_i) mTilde^-1 mod q_i
            x = [yi * (self.Q // qi) * pow(M, -1, qi) % qi for yi, qi in zip(y, self.q)]
            if self.lift(x)[1] == target:
                return x
        return None

    # ---- approximateFloor + convertApproximateBskToQ ----------------------------------------------------------
    def floor_parts(self, x):
        """x: 2L + 1 residues over [q, Bsk] -> (f [L + 1] = approximateFloor's words, alpha0, conv_msk)."""
        L = self.L
        y = [xi * inv % qi for xi, qi, inv in zip(x, self.q, self.inv_punctured_q)]
        conv = [sum(yi * c for yi, c in zip(y, self.q_to[b])) % b for b in self.bsk]                   # :385
        f = [(x[L + j] + b - conv[j]) * self.inv_q_mod_bsk[j] % b for j, b in enumerate(self.bsk)]     # :394
        z = [fi * inv % bi for fi, bi, inv in zip(f, self.b_moduli, self.inv_punctured_b)]             # :414
        alpha0 = sum(zi * c for zi, c in zip(z, self.b_to[self.top_m_sk])) % self.top_m_sk            # :415
        return f, z, alpha0, conv[L]

    def floor(self, x):
        """-> (L words over q, alpha).  alpha is the word `alpha > m_sk/2` is decided on."""
        f, z, alpha0, _ = self.floor_parts(x)
        m_sk = self.m_sk
        alpha = (alpha0 + m_sk - f[self.L]) * self.inv_b_mod_msk % m_sk                                 # :427-428
        exceeds = alpha > m_sk >> 1                                                                     # :419, 430
        out = []
        for qi in self.q:
            converted = sum(zi * c for zi, c in zip(z, self.b_to[qi])) % qi                            # :433
            adjust = self.B % qi * (m_sk - alpha) % qi if exceeds else -self.B % qi * alpha % qi        # :441-444
            out.append((converted + adjust) % qi)                                                       # :445
        return out, alpha

    def floor_input_with_alpha(self, rng, target):
        """2L + 1 random residues with the m_sk one set so that alpha == target: alpha = (alpha0 - f_msk) B^-1, hence
        f_msk = alpha0 - target B (mod m_sk) (B as inverseBModMSk sees it), and x_msk = f_msk Q + conv_msk (:394 backwards)."""
        x = [rng.randrange(m) for m in self.q + self.bsk]
        _, _, alpha0, conv_msk = self.floor_parts(x)
        f_msk = (alpha0 - target * self.b_mod_msk) % self.m_sk
        x[2 * self.L] = (f_msk * self.Q + conv_msk) % self.m_sk
        return x if self.floor(x)[1] == target else None

    def floor_alpha_targets(self):
        m, L = self.m_sk, self.L
        return [0, 1, L, m - 1, m - L, m // 2 - 1, m // 2, m // 2 + 1]

    # ---- scaleAndRound ------------------------------------------------------------------------------------------
    def scale_and_round(self, x, scaling_factor=1):
        """x: L residues -> (word mod t, mod_gamma).  mod_gamma is the word `> gamma/2` is decided on."""
        t, gamma = self.t, self.gamma
        y = [xi * (gamma * t % qi) % qi * inv % qi for xi, qi, inv in zip(x, self.q, self.inv_punctured_q)]   # :274, 276
        mod_t, mod_gamma = (sum(yi * c for yi, c in zip(y, self.q_to[m])) % m * self.neg_inv_q_mod_t_gamma[m] % m
                            for m in (t, gamma))                                                              # :276-277
        if mod_gamma > gamma // 2:                                                                            # :280, 290
            s_gamma = -((gamma - mod_gamma) % t) % t                                                          # :288
        else:
            s_gamma = mod_gamma % t                                                                           # :289
        scaled_inverse = pow(gamma, -1, t) * scaling_factor % t                                               # :298
        return (mod_t - s_gamma) % t * scaled_inverse % t, mod_gamma                                          # :295, 299

    def scale_and_round_reaches_targets(self):
        """gamma t x / Q moves by less than one per unit of x only when Q > gamma t; below that the constructed x cannot
        be steered onto a chosen mod_gamma: every level with one modulus, and no other of the sets below."""
        return self.Q > self.gamma * self.t

    def scale_and_round_input_with_mod_gamma(self, rng, target, draws=4000):
        """mod_gamma = floor(gamma t x / Q) - a (mod gamma) for the converter's overshoot a in [0, L): take
        x = ceil(Q (n gamma + target + a) / (gamma t)) + {0, 1, 2} over random n and a and keep the first hit."""
        gt = self.gamma * self.t
        for _ in range(draws):
            n, a = rng.randrange(self.t - 1), rng.randrange(self.L)
            base = -(-self.Q * (n * self.gamma + target + a) // gt)
            for x_int in (base, base + 1, base + 2):
                if x_int < self.Q:
                    x = [x_int % qi for qi in self.q]
                    if self.scale_and_round(x)[1] == target:
                        return x
        return None

    def scale_and_round_targets(self):
        g = self.gamma
        return [0, 1, g // 2 - 1, g // 2, g // 2 + 1, g - 1]

    def noise_bound(self):
        """RnsTool.swift:263: the largest integer |v| with |v| <= Q/t (1/2 - k/gamma) - |Q|_t / 2."""
        bound = Fraction(self.Q, self.t) * (Fraction(1, 2) - Fraction(self.L, self.gamma)) - Fraction(self.Q % self.t, 2)
        return bound.numerator // bound.denominator

    def noise_bound_applies(self):
        """The bound speaks of Delta m + v for EVERY m < t only where Delta's own truncation, (Q mod t) m / Q of a unit, stays
        inside the rounding margin 1/2 - k/gamma: a level whose Q is not far above t^2 (one 30-bit modulus under a 17-bit t)
        is outside it, and there only the words are compared."""
        margin = Fraction(1, 2) - Fraction(self.L, self.gamma)
        return self.noise_bound() > 0 and Fraction(self.Q % self.t * (self.t - 1), self.Q) < margin

    # ---- plaintextTranslate -------------------------------------------------------------------------------------
    def plaintext_translate(self, c0, m, subtract=False):
        """c0: L residues, m < t -> (L words, one_short).  one_short: whether the double-word Barrett estimate of
        floor(((Q mod t) m + (t + 1)/2) / t) from floor(2^128 / t) -- the high 64 bits of the 256-bit product, as the device
        takes them -- is one below the quotient, so that its one-word fix-up adds 1."""
        t = self.t
        dividend = self.Q % t * m + (t + 1) // 2                                    # Bfv+Encrypt.swift:95-96, 102-104
        adjust = dividend // t                                                       # :97, 105
        estimate = (dividend * (((1 << 128) - 1) // t) >> 128) & MASK64
        one_short = ((dividend - estimate * t) & MASK64) >= t
        assert estimate + one_short == adjust, "the estimate is at most one short"
        out = []
        for ci, qi in zip(c0, self.q):
            term = (self.Q // t % qi * m + adjust) % qi                              # :117-120
            out.append((ci - term) % qi if subtract else (ci + term) % qi)           # :121, 132-134
        return out, one_short

    def plaintext_one_short_message(self):
        """The estimate x floor(2^128/t) / 2^128 is below x/t by less than x / 2^128 < t^2 / 2^128 < 1/t (t < 2^62), so it
        falls one short exactly where t divides the dividend: (Q mod t) m + (t + 1)/2 = 0 (mod t), one message per level."""
        return -((self.t + 1) // 2) * pow(self.Q % self.t, -1, self.t) % self.t

    def plaintext_messages(self):
        t = self.t
        return [0, 1, (t + 1) // 2 - 1, (t + 1) // 2, t - 1, self.plaintext_one_short_message()]


def first_multiple_in_range(a, m, low, high):
    """The least k >= 0 with low <= a k mod m <= high (0 <= low <= high < m, 0 <= a < m), or None.  If no multiple of a
    lies in [low, high] before the first wrap, then a k - m y is in the range for the least y with
    m y mod a in [-high mod a, -low mod a] -- the same question on (m mod a, a)."""
    if low == 0:
        return 0
    if a == 0:
        return None
    k = -(-low // a)
    if a * k <= high:
        return k
    y = first_multiple_in_range(m % a, a, -high % a, -low % a)
    if y is None:
        return None
    return -(-(low + m * y) // a)


# ---- divideAndRoundQLast -----------------------------------------------------------------------------------------
def divide_and_round_q_last(x_int, moduli):
    """PolyRq.swift:365-393 on the composed integer: x + h2 - ((x_last + h2) mod q_last) = q_last floor((x + h2) / q_last)
    with h2 = q_last >> 1, so every remaining row holds round-half-up(x / q_last) -> (the integer, x mod q_last)."""
    q_last = moduli[-1]
    return (x_int + (q_last >> 1)) // q_last, x_int % q_last


def mod_switch_chain(x_int, moduli):
    """Ciphertext.modSwitchDownToSingle (Bfv.swift:163-171): the steps down to one modulus -> (integer, [x mod q_last per step])."""
    remainders = []
    for count in range(len(moduli), 1, -1):
        x_int, h = divide_and_round_q_last(x_int, moduli[:count])
        remainders.append(h)
    return x_int, remainders


def q_last_remainders(q_last):
    return [0, 1, q_last // 2 - 1, q_last // 2, q_last // 2 + 1, q_last - 1]


def mod_switch_integer(rng, moduli, h, k_kind):
    """k q_last + h with k in {0, 1, random, floor(Q / q_last) - 1} (k_kind 0..3)."""
    rest = prod(moduli[:-1])
    k = (0, min(1, rest - 1), rng.randrange(rest), rest - 1)[k_kind]
    return k * moduli[-1] + h


def nested_mod_switch_integer(rng, moduli, pick):
    """((k q_1 + h_1) q_2 + h_2) ... with every h_i = q_last_remainders(q_i)[pick(i)], corrected for the rounding of the step
    before: a step with h above q_i / 2 rounds up, so its quotient is taken one lower and the NEXT step still meets the
    remainder it was given."""
    value = rng.randrange(1, moduli[0])
    for i in range(1, len(moduli)):
        h = q_last_remainders(moduli[i])[pick(i)]
        value = (value - (1 if h > moduli[i] >> 1 else 0)) * moduli[i] + h
    return value


# ---- the two host flags that choose the kernel forms (bfv_context.cpp, the block that fills RnsToolDevice) ------------
def _wide_shift(p):
    bits = p.bit_length()
    return bits - 1 if 34 <= bits <= 61 and p & (p - 1) else 0


def floor_merge_ok(level):
    worst = (max(level.bsk) - 1) * (max(level.q) - 1)
    return worst == 0 or (1 << 127) // worst > level.L + 1


def wide_reduce_ok(level):
    def fits(worst, p):
        return _wide_shift(p) != 0 and worst >> (64 + _wide_shift(p)) == 0

    L, q, bsk, m_sk, top = level.L, level.q, level.bsk, level.m_sk, level.top_m_sk
    q_sum, bsk_sum = sum(qi - 1 for qi in q), sum(b - 1 for b in bsk[:L])
    ok = all(fits((q_sum + b - 1) * (b - 1), b) for b in bsk)
    ok = ok and fits(bsk_sum * (top - 1), top) and fits(bsk_sum * (m_sk - 1), m_sk)
    ok = ok and all(fits((bsk_sum + m_sk - 1) * (qi - 1), qi) for qi in q)
    high = lambda v: (v >> 32) + 1
    return ok and (L + 1) * (high(max(q)) + high(max(bsk + [top]))) <= 1 << 32


# ---- whole polynomials: the targets cycled over the coefficient index ----------------------------------------------
def cycled(count, degree):
    """Target index per coefficient: k + k // count steps the cycle by one extra per pass, so every lane of a pair or a
    quad (k mod 2, k mod 4) meets every target once degree >= 4 count even where count is even."""
    return [(k + k // count) % count for k in range(degree)]


def columns_to_rows(columns):
    """[degree][rows] python ints -> [rows][degree]."""
    return [list(row) for row in zip(*columns)]


# ---- parameter sets and whole test polynomials -------------------------------------------------------------------------
# (name, word bits, degree, ciphertext moduli bits, key-switching modulus bits, t as bits or [value]).  The smallest shapes at
# which every kernel form runs: lift two coefficients per lane (8-byte, wide_reduce_ok, L <= 6) and one (L > 6 or not
# wide_reduce_ok), the merged and the separate floor correction, the rolled / unrolled / to-single mod switch, the four
# words per lane of 4-byte slabs (degree >= 4).
PARAMETER_SETS = [
    ("q40x3", 64, 64, [40, 40, 40], 41, 17),
    ("q55x4", 64, 256, [55, 55, 55, 55], 55, [557057]),
    ("q62_62_61", 64, 64, [62, 62, 61], 62, 17),
    ("q61_33_62_45", 64, 64, [61, 33, 62, 45], 62, 32),
    ("q60x8", 64, 64, [60] * 8, 60, 41),
    ("q45x9", 64, 64, [45] * 9, 45, 17),
    ("w32_27_28_28_n64", 32, 64, [27, 28, 28], 28, 10),
    ("w32_27_28_28_n1024", 32, 1024, [27, 28, 28], 28, 17),
    ("w32_30_20_30_n1024", 32, 1024, [30, 20, 30], 29, 17),
]
GAMMA = {64: (1 << 62) - 40797, 32: (1 << 30) - 20405}  # T.rnsCorrectionFactor (ModularArithmetic/Scalar.swift:498-525)
MTILDE = {64: 1 << 32, 32: 1 << 16}                     # T.mTilde
DISTINCT = 64  # constructed coefficients per polynomial; a longer polynomial repeats them
SETS = {s[0]: s for s in PARAMETER_SETS}


def tile(columns, degree):
    """[DISTINCT][rows] -> [rows][degree], the columns repeated along the polynomial."""
    return [[columns[k % len(columns)][row] for k in range(degree)] for row in range(len(columns[0]))]


def lift_r_targets(level):
    M = level.mtilde
    return [0, 1, M // 2 - 1, M // 2, M // 2 + 1, M - 1]


def lift_integers(level):
    Q = level.Q
    return [0, 1, Q - 1, Q // 2 - 1, Q // 2, Q // 2 + 1]


def lift_threshold_columns(level, seed):
    rng, targets = random.Random(seed), lift_r_targets(level)
    return [level.lift_input_with_r(rng, targets[i]) for i in cycled(len(targets), DISTINCT)]


def lift_integer_columns(level):
    values = lift_integers(level)
    picks = cycled(len(values), DISTINCT)
    return [[values[i] % qi for qi in level.q] for i in picks], [values[i] for i in picks]


def floor_threshold_columns(level, seed):
    rng, targets = random.Random(seed), level.floor_alpha_targets()
    return [level.floor_input_with_alpha(rng, targets[i]) for i in cycled(len(targets), DISTINCT)]


def floor_integers(level, rng):
    Q, big = level.Q, level.Q * prod(level.bsk)
    k = rng.randrange(2, prod(level.bsk) - 1)
    return [0, 1, Q - 1, Q, big - 1, k * Q - 1, k * Q + 1]


def floor_integer_columns(level, seed):
    rng = random.Random(seed)
    moduli = level.q + level.bsk
    columns = []
    for i in cycled(7, DISTINCT):
        columns.append([floor_integers(level, rng)[i] % m for m in moduli])
    return columns


def scale_threshold_columns(level, seed):
    """Every target where the level can reach them; otherwise random coefficients (the test then asks for both sides only)."""
    rng, targets = random.Random(seed), level.scale_and_round_targets()
    if not level.scale_and_round_reaches_targets():
        return [[rng.randrange(qi) for qi in level.q] for _ in range(DISTINCT)]
    return [level.scale_and_round_input_with_mod_gamma(rng, targets[i]) for i in cycled(len(targets), DISTINCT)]


def scale_genuine_columns(level, seed):
    """Delta m + v with |v| at the bound of RnsTool.swift:263 and one below it -> (columns, messages).
    t (Delta m + v) / Q = m - (Q mod t) m / Q + t v / Q: the truncation of Delta pulls DOWN by up to (Q mod t) m / Q, which the
    bound's |Q|_t / 2 covers for a negative v only while m <= t/2 -- so a negative v comes with such an m, a positive v with any."""
    rng, bound, delta, t = random.Random(seed), level.noise_bound(), level.Q // level.t, level.t
    columns, messages = [], []
    for k in range(DISTINCT):
        v = (bound, -bound, bound - 1, 1 - bound)[k % 4] if bound > 0 else 0
        m = ((0, 1, t - 1, rng.randrange(t)) if v >= 0 else (0, 1, t // 2, rng.randrange(t // 2)))[(k // 4) % 4]
        columns.append([(delta * m + v) % level.Q % qi for qi in level.q])
        messages.append(m)
    return columns, messages


def translate_messages(level, degree):
    values = level.plaintext_messages()
    return [values[i] for i in cycled(len(values), degree)]


def mod_switch_columns(moduli, seed):
    """One step: k q_last + h, h cycled over the six remainders, k over its four kinds -> (residue columns, integers)."""
    rng, remainders = random.Random(seed), q_last_remainders(moduli[-1])
    picks = cycled(len(remainders), DISTINCT)
    integers = [mod_switch_integer(rng, moduli, remainders[i], (k // len(remainders)) % 4) for k, i in enumerate(picks)]
    return [[x % m for m in moduli] for x in integers], integers


def mod_switch_chain_columns(moduli, seed):
    """The chain to one modulus: nested integers, the steps' remainders walking the six values out of phase."""
    rng = random.Random(seed)
    picks = cycled(6, DISTINCT)
    integers = [nested_mod_switch_integer(rng, moduli, lambda i, c=c: (c + i) % 6) for c in picks]
    return [[x % m for m in moduli] for x in integers], integers


def top_level_lift_is_centered(level, integers, lifted):
    """The top level's lift is the centred lift (RnsToolTests.swift:168-208) -- up to the converter's overshoot.  The small
    Montgomery reduction hands back (c + Q r) / mTilde for c = [x mTilde]_Q + a Q, 0 <= a < L, and r centred in
    [-mTilde/2, mTilde/2): the representative of x in [-Q/2, Q/2 + L Q / mTilde).  So every x outside (Q/2, Q/2 + L Q / mTilde)
    gets exactly its centred representative, and an x inside that sliver (floor(Q/2) + 1 is one) either of the two."""
    moduli = level.q + level.bsk
    for x, words in zip(integers, lifted):
        exact = level.exact_centered_lift(x)
        in_sliver = level.Q // 2 < x < level.Q // 2 + level.L * level.Q // level.mtilde
        if words != exact and not (in_sliver and words == [x % m for m in moduli]):
            return False
    return True


# ---- for the tests: a parameter set's contexts, and polynomials as arrays ---------------------------------------------------
def levels_of(ctx, word_bits):
    """{level: Level} of an oracle BfvContext, whatever its moduli come from."""
    q, bsk_top = [int(m) for m in ctx.coefficient_moduli], ctx.rns_tool(ctx.L).bsk
    return {L: Level(q[:L], bsk_top, ctx.t, GAMMA[word_bits], MTILDE[word_bits]) for L in range(1, ctx.L + 1)}


def build_set(oracle, name, t_bits=None, t_value=None):
    """-> (oracle BfvContext, {level: Level}) of a parameter set.  t_bits overrides the bit count of the set's plaintext
    modulus (an NTT-friendly prime of that size is generated), t_value gives the modulus itself, NTT-friendly or not."""
    _, word_bits, degree, bits, ks_bits, t = SETS[name]
    t = t_bits if t_bits is not None else t
    t = [t_value] if t_value is not None else t
    t = t[0] if isinstance(t, list) else oracle.generate_primes([t], True, degree, word_bits=word_bits)[0]
    q = oracle.generate_primes(bits + [ks_bits], False, degree, word_bits=word_bits)
    assert len(set(q)) == len(q)
    ctx = oracle.BfvContext(degree, t, q, word_bits=word_bits)
    return ctx, levels_of(ctx, word_bits)


def rows(columns, degree):
    return np.array(tile(columns, degree), dtype=np.uint64)


def expected_rows(columns, degree, restate):
    words = [restate(x)[0] for x in columns]
    return rows([w if isinstance(w, list) else [w] for w in words], degree)
