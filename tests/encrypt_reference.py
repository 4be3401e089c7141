"""Secret keys, encryption and key-switch keys restated in Python integers over a byte stream given as an argument
(reference Sources/HomomorphicEncryption/: PolyRq/PolyRq+Randomize.swift:87-167, Bfv/Bfv+Encrypt.swift:66-181,
Bfv/Bfv+Keys.swift:20-103).  `stream(seed, count)` returns the first `count` bytes of the generator seeded with `seed`;
oracle_stream is NistAes128Ctr(seed:) -- BufferedRng over 4096-byte generate() calls of the oracle's CtrDrbg, which other tests
hold to the NIST vectors and to wire_format_reference.CtrDrbg.  The oracle serves for the transforms, the products and the
uniform polynomial `a`; the samplers and the joins are spelled out here.  Polynomials are numpy uint64 arrays [rows][N]."""
import math

import numpy as np

SEED_BYTES = 32
CHUNK = 4096  # BufferedRng's refill (Random/NistAes128Ctr.swift)
TRIAL_BITS = math.ceil(2 * 3.2 * 3.2)  # k of ErrorStdDev.stdDev32, PolyRq+Randomize.swift:131-132


def oracle_stream(oracle):
    def stream(seed, count):
        drbg = oracle.CtrDrbg(bytes(seed))
        return b"".join(bytes(drbg.generate(CHUNK)) for _ in range(-(-count // CHUNK)))[:count]
    return stream


def ternary_values(stream_bytes, n, first=0):
    """randomizeTernary's draws for coefficients first .. first + n - 1: 0, 1, 2 (PolyRq+Randomize.swift:95-99)"""
    out = []
    for k in range(first, first + n):
        record = stream_bytes[12 * k:12 * k + 12]
        u64, u32 = int.from_bytes(record[:8], "little"), int.from_bytes(record[8:], "little")
        out.append(((u64 << 32) | u32) % 3)
    return out


def ternary(stream_bytes, n, moduli, first=0):
    return np.array([[(v - 1) % q for v in ternary_values(stream_bytes, n, first)] for q in moduli], dtype=np.uint64)


def binomial_values(stream_bytes, n, first=0):
    """randomizeCenteredBinomialDistribution's signed draws (PolyRq+Randomize.swift:134-160): two UInt64 per coefficient"""
    assert TRIAL_BITS == 21
    mask = (1 << TRIAL_BITS) - 1
    out = []
    for j in range(first, first + n):
        record = stream_bytes[16 * j:16 * j + 16]
        pos = bin(int.from_bytes(record[:8], "little") & mask).count("1")
        neg = bin(int.from_bytes(record[8:], "little") & mask).count("1")
        out.append(pos - neg)
    return out


def centered_binomial(stream_bytes, n, moduli, first=0):
    return np.array([[v % q for v in binomial_values(stream_bytes, n, first)] for q in moduli], dtype=np.uint64)


def generate_secret_key(secret_ctx, seed, stream):
    """Bfv.generateSecretKey (Bfv+Keys.swift:20-26) -> [L_all][N] Eval"""
    n = secret_ctx.degree
    return secret_ctx.forward_ntt(ternary(stream(seed, 12 * n), n, secret_ctx.moduli))


class HostSide:
    """The CPU side of one parameter set on one word size with the secret key of key_seeds[0]: the oracle's contexts, the byte
    stream, the key in Eval form and a BfvClient that holds it.  tests/test_gpu_encrypt.py puts a device context beside it,
    tests/predefined_sets.py the oracle's chain of operations."""

    def __init__(self, oracle, degree, t, moduli, word, key_seeds):
        from bfv_helpers import BfvClient

        self.oracle = oracle
        self.degree, self.t, self.moduli, self.word = degree, t, [int(q) for q in moduli], word
        self.ref_ctx = oracle.BfvContext(degree, t, self.moduli, word_bits=word)
        self.stream = oracle_stream(oracle)
        self.secret_ctx = oracle.PolyContext(degree, self.moduli)
        self.key_seeds = key_seeds
        self.s_eval = generate_secret_key(self.secret_ctx, bytes(key_seeds[0]), self.stream)
        self.client = BfvClient(oracle, self.ref_ctx)
        self.client.s_eval_all = self.s_eval
        self.L_all = len(self.moduli)


def encrypt_zero(poly_ctx, s_eval, a_seed, error_seed, stream, eval_out=False):
    """Bfv.encryptZero(for:using:with:) (Bfv+Encrypt.swift:150-181) over poly_ctx; s_eval [>= L'][N], its first rows are used.
    -> [2][L'][N], Coeff, or forward-transformed (what _generateKeySwitchKey does next) with eval_out."""
    n, rows = poly_ctx.degree, len(poly_ctx.moduli)
    a = poly_ctx.random_from_seeds(np.frombuffer(bytes(a_seed), dtype=np.uint8)[None])[0]
    error = centered_binomial(stream(error_seed, 16 * n), n, poly_ctx.moduli)
    c0 = poly_ctx.inverse_ntt(poly_ctx.mul(a, np.asarray(s_eval[:rows], dtype=np.uint64)))
    c0 = poly_ctx.add(c0, error)
    ct = np.stack([poly_ctx.neg(c0), poly_ctx.inverse_ntt(a)])
    return poly_ctx.forward_ntt(ct) if eval_out else ct


def plaintext_translate_add(ct, message, moduli, t):
    """plaintextTranslate(.Add) (Bfv+Encrypt.swift:75-139) on c0 of a Coeff ciphertext [2][L][N]"""
    q = 1
    for m in moduli:
        q *= int(m)
    q_mod_t, q_div_t, t_threshold = q % t, q // t, (t + 1) // 2
    out = ct.copy()
    for i, qi in enumerate(moduli):
        for k, m in enumerate(message):
            adjust = (q_mod_t * int(m) + t_threshold) // t
            out[0, i, k] = (int(ct[0, i, k]) + (q_div_t % qi) * int(m) % qi + adjust) % qi
    return out


def encrypt(poly_ctx, t, message, s_eval, a_seed, error_seed, stream):
    """Bfv.encrypt (Bfv+Encrypt.swift:66-73)"""
    return plaintext_translate_add(encrypt_zero(poly_ctx, s_eval, a_seed, error_seed, stream), message, poly_ctx.moduli, t)


def key_switch_key(ks_ctx, s_eval, current_eval, a_seeds, error_seeds, stream):
    """Bfv._generateKeySwitchKey (Bfv+Keys.swift:69-103): ks_ctx over all L + 1 moduli -> [L][2][L+1][N] Eval"""
    moduli = [int(q) for q in ks_ctx.moduli]
    q_ks = moduli[-1]
    ciphers = []
    for row, qi in enumerate(moduli[:-1]):
        key = encrypt_zero(ks_ctx, s_eval, a_seeds[row], error_seeds[row], stream, eval_out=True)
        factor = q_ks % qi
        key[0, row] = ((key[0, row].astype(object) + factor * np.asarray(current_eval[row]).astype(object)) % qi).astype(np.uint64)
        ciphers.append(key)
    return np.stack(ciphers)


def relinearization_current_key(secret_ctx, s_eval):
    """s s (Bfv+Keys.swift:62)"""
    return secret_ctx.mul(np.asarray(s_eval, dtype=np.uint64), np.asarray(s_eval, dtype=np.uint64))


def galois_current_key(secret_ctx, s_eval, element):
    """secretKey.poly.applyGalois(element:) in Eval form (Bfv+Keys.swift:39)"""
    return secret_ctx.apply_galois(np.asarray(s_eval, dtype=np.uint64)[None], element, eval_format=True)[0]
