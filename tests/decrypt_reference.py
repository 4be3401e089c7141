"""Decryption, noise budget and transparency restated in Python integers (reference Sources/HomomorphicEncryption/:
Bfv/Bfv+Decrypt.swift:21-39,116-204, Bfv/Bfv+Encrypt.swift:48-62, CrtComposer.swift:54-97).  The oracle is used for the
transforms only; everything else is spelled out here, so that tests/test_gpu_decrypt.py has something to compare the device
with that shares no code with it.  Polynomials are numpy uint64 arrays [rows][N]; composed values are Python integers."""
import functools
import math

import numpy as np


def product(moduli):
    q = 1
    for m in moduli:
        q *= int(m)
    return q


def dot_product(poly_ctx, ct, s_eval, eval_format=False):
    """Bfv.dotProduct (Bfv+Decrypt.swift:188-204): ct [polys][L][N], s_eval [>= L][N] Eval (the first L rows are used,
    PolyRq.swift:184-194) -> c0 + c1 s + c2 s^2 ... as [L][N] Coeff."""
    moduli = [int(q) for q in poly_ctx.moduli]
    ct_eval = np.asarray(ct, dtype=np.uint64) if eval_format else poly_ctx.forward_ntt(np.asarray(ct, dtype=np.uint64))
    polys, rows, n = ct_eval.shape
    assert rows == len(moduli) <= len(s_eval)
    dot = np.zeros((rows, n), dtype=np.uint64)
    for i, q in enumerate(moduli):  # rows of Python integers (object arrays): exact, whatever the modulus
        s = np.asarray(s_eval[i]).astype(object)
        total, power = ct_eval[0][i].astype(object), s
        for c in range(1, polys):
            total = total + ct_eval[c][i].astype(object) * power
            power = power * s % q
        dot[i] = (total % q).astype(np.uint64)
    return poly_ctx.inverse_ntt(dot)


@functools.lru_cache(maxsize=None)
def _composer(moduli):
    """(Q, [(q_i, Q / q_i, (Q / q_i)^-1 mod q_i)]) of CrtComposer.init (CrtComposer.swift:32-50)"""
    q = product(moduli)
    return q, [(qi, q // qi, pow(q // qi % qi, -1, qi)) for qi in moduli]


def crt_compose(residues, moduli):
    """CrtComposer.compose (CrtComposer.swift:76-97) for one coefficient, accumulated as the reference does."""
    q, rows = _composer(tuple(int(m) for m in moduli))
    composed = 0
    for r, (qi, punctured, inverse_punctured) in zip(residues, rows):
        tmp = inverse_punctured * int(r) % qi  # inversePuncturedProduct.multiplyMod
        composed += tmp * punctured  # below q: tmp < qi
        if composed >= q:  # addMod
            composed -= q
    return composed


def centred_magnitude(x, q):
    """Bfv+Decrypt.swift:136-143"""
    q_div_2 = (q + 1) >> 1
    return q - x if x > q_div_2 else x


def composed_t_dot(dot, moduli, t):
    """[t dot_k]_Q for every coefficient: CrtComposer.compose row by row, as the reference walks its Array2d (rows of Python
    integers)"""
    q, rows = _composer(tuple(int(m) for m in moduli))
    composed = np.zeros(dot.shape[1], dtype=object)
    for values, (qi, punctured, inverse_punctured) in zip(dot, rows):
        tmp = int(t) * values.astype(object) % qi * inverse_punctured % qi
        composed = composed + tmp * punctured
        composed = np.where(composed >= q, composed - q, composed)  # addMod
    return [int(x) for x in composed]


def noise_norm(dot, moduli, t):
    q = product(moduli)
    return max(centred_magnitude(x, q) for x in composed_t_dot(dot, moduli, t))


def noise_budget(norm, moduli):
    """Bfv+Decrypt.swift:144-148; float(int) rounds to nearest, ties to even, as Swift's Double(_:) does"""
    if norm == 0:
        return math.inf
    q_double = 1.0
    for m in moduli:
        q_double *= float(int(m))
    return math.log2(q_double / (2 * float(norm)))


def _power(x, exponent):
    try:
        return x**exponent
    except OverflowError:
        return math.inf


def needs_variable_time(moduli, word_bits):
    """Bfv+Decrypt.swift:151-173: None when the composed width fits T (no precondition), True when a wider integer is used
    (precondition(variableTime)); raises where the reference's preconditionFailure would."""
    doubles = [float(int(m)) for m in moduli]
    q_double = 1.0
    for d in doubles:
        q_double *= d
    crt_max = doubles[0] if len(doubles) == 1 else 2.0 * q_double  # CrtComposer.swift:54-61
    t_max = float(2**word_bits - 1)
    if crt_max < t_max:
        return None
    if crt_max < _power(t_max, 32):
        return True
    raise ValueError("crtMaxIntermediateValue too large")


def decrypt(dot, moduli, t, correction_factor=1):
    """round(t [dot]_Q / Q) mod t on exact integers (what scaleAndRound computes, RnsTool.swift:272-302), times the inverse of the
    correction factor (Bfv+Decrypt.swift:34-36)"""
    q = product(moduli)
    scaling = pow(int(correction_factor), -1, int(t))
    out = []
    for k in range(dot.shape[1]):
        x = crt_compose([int(dot[i][k]) for i in range(len(moduli))], moduli)
        if x > q // 2:
            x -= q
        out.append((2 * int(t) * x + q) // (2 * q) % int(t) * scaling % int(t))
    return out


def is_transparent(ct):
    """Bfv+Encrypt.swift:48-62"""
    return not np.asarray(ct)[1:].any()


def transparent_ciphertext(values, n, moduli, t, polys=2):
    """A Coeff ciphertext [polys][L][N] whose composed value [t dot_k]_Q is exactly values[k] (0 where k is not a key):
    c1.. = 0, so the dot product is c0 whatever the key, and c0 = w t^-1 mod Q in RNS."""
    q = product(moduli)
    inverse_t = pow(int(t), -1, q)
    ct = np.zeros((polys, len(moduli), n), dtype=np.uint64)
    for k, w in values.items():
        c0 = int(w) % q * inverse_t % q
        for i, qi in enumerate(moduli):
            ct[0][i][k] = c0 % int(qi)
    return ct
