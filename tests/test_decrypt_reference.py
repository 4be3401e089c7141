"""tests/decrypt_reference.py held to the tests' other statements of decryption (bfv_helpers.BfvClient.decrypt_exact and
bfv_helpers.crt_compose, a different composition formula), and the library's host entries for the noise budget
(he_bfv_noise_norm_limbs, he_bfv_noise_budget_from_norm) held to the restatement.  No device is needed: the contexts are
host-only."""
import ctypes
import math
import random

import numpy as np
import pytest

import bfv_helpers
import decrypt_reference as ref
import heamd


def _client(oracle, degree, bits, t_bits=17, seed=3):
    t = oracle.generate_primes([t_bits], True, degree)[0]
    q = oracle.generate_primes(bits, False, degree)
    ctx = oracle.BfvContext(degree, t, q)
    return ctx, bfv_helpers.BfvClient(oracle, ctx, seed=seed)


@pytest.mark.parametrize("degree,bits", [(8, [30, 30]), (16, [40, 41, 42]), (8, [27, 28, 28, 29])])
def test_restatement_decrypts_as_the_exact_client_does(oracle, degree, bits):
    ctx, client = _client(oracle, degree, bits)
    rng = random.Random(degree)
    for moduli_count in range(ctx.L, 0, -1):
        poly_ctx = ctx.ciphertext_context(moduli_count)
        moduli = [int(q) for q in poly_ctx.moduli]
        message = [rng.randrange(ctx.t) for _ in range(degree)]
        ct = client.encrypt(message, moduli_count)
        dot = ref.dot_product(poly_ctx, ct, client.s_eval_all)  # more key rows than the level uses
        assert ref.decrypt(dot, moduli, ctx.t) == client.decrypt_exact(ct, moduli_count) == message
        assert ref.decrypt(dot, moduli, ctx.t) == client.decrypt(ct, moduli_count)
        eval_ct = poly_ctx.forward_ntt(ct)
        assert np.array_equal(ref.dot_product(poly_ctx, eval_ct, client.s_eval_all, eval_format=True), dot)
        five = ref.decrypt(dot, moduli, ctx.t, correction_factor=5)
        assert [v * 5 % ctx.t for v in five] == message
        # the composition, against a different formula
        for k in range(degree):
            residues = [int(dot[i][k]) for i in range(moduli_count)]
            assert ref.crt_compose(residues, moduli) == bfv_helpers.crt_compose(residues, moduli)
        # a fresh ciphertext has noise budget to spare, and the budget is the reference's formula on the exact norm
        norm = ref.noise_norm(dot, moduli, ctx.t)
        q = ref.product(moduli)
        assert 0 < norm <= (q + 1) >> 1
        assert ref.noise_budget(norm, moduli) > 0
        assert not ref.is_transparent(ct)


def test_constructed_ciphertexts_compose_to_the_chosen_value(oracle):
    degree = 8
    ctx, client = _client(oracle, degree, [30, 31, 32])
    poly_ctx = ctx.ciphertext_context(2)
    moduli = [int(q) for q in poly_ctx.moduli]
    q = ref.product(moduli)
    half = (q + 1) >> 1
    values = {0: 0, 1: 1, 2: half - 1, 3: half, 4: half + 1, 5: q - 1}
    ct = ref.transparent_ciphertext(values, degree, moduli, ctx.t)
    assert ref.is_transparent(ct)
    dot = ref.dot_product(poly_ctx, ct, client.s_eval_all)
    assert ref.composed_t_dot(dot, moduli, ctx.t) == [0, 1, half - 1, half, half + 1, q - 1, 0, 0]
    assert [ref.centred_magnitude(x, q) for x in (0, 1, half - 1, half, half + 1, q - 1)] == [0, 1, half - 1, half, half - 2, 1]
    assert ref.noise_norm(dot, moduli, ctx.t) == half
    assert ref.noise_budget(0, moduli) == math.inf
    one_poly = ct[:1]
    assert ref.is_transparent(one_poly)
    ct[1][1][degree - 1] = 1
    assert not ref.is_transparent(ct)


# (bit counts, preferring_small): Q just below and just above a limb boundary, one modulus, and many
LIMB_SETS = [([32, 32], False), ([33, 33], True), ([43, 43, 42], False), ([44, 44, 43], True), ([55], False),
             ([55, 55, 55, 55], False), ([50] * 16, False)]


def _host_context(bits, preferring_small, degree=8, t_bits=17):
    moduli = heamd.generate_primes(bits + [bits[-1]], preferring_small, degree)  # (the last one is the key-switching modulus)
    t = heamd.generate_primes([t_bits], True, degree)[0]
    return heamd.BfvContext(degree, t, moduli, host_only=True), moduli[:-1]


@pytest.mark.parametrize("bits,preferring_small", LIMB_SETS)
def test_noise_norm_limbs(bits, preferring_small):
    ctx, moduli = _host_context(bits, preferring_small)
    assert ctx.L == len(moduli)
    for count in range(1, ctx.L + 1):
        assert ctx.noise_norm_limbs(count) == (ref.product(moduli[:count]).bit_length() + 63) // 64
    lib = heamd.load_library()
    assert lib.he_bfv_noise_norm_limbs(ctx.h, 0) == 0 and lib.he_bfv_noise_norm_limbs(ctx.h, ctx.L + 1) == 0
    assert lib.he_bfv_noise_norm_limbs(None, 1) == 0


def test_limb_boundaries_are_what_the_sets_were_chosen_for():
    q = {tuple(bits): ref.product(_host_context(bits, small)[1]) for bits, small in LIMB_SETS[:4]}
    assert 2**63 < q[(32, 32)] < 2**64 < q[(33, 33)] < 2**64 + 2**48
    assert 2**127 < q[(43, 43, 42)] < 2**128 < q[(44, 44, 43)] < 2**128 + 2**112


@pytest.mark.parametrize("bits,preferring_small", LIMB_SETS)
def test_noise_budget_from_norm_is_the_restatements_double(bits, preferring_small):
    """Both end in the platform's log2 of the same double quotient, so the library's value is within one ulp of Python's;
    on this platform every value below came out equal."""
    ctx, moduli = _host_context(bits, preferring_small)
    rng = random.Random(len(bits))
    for count in {1, ctx.L}:
        q = ref.product(moduli[:count])
        half = (q + 1) >> 1
        norms = [1, 2, 3, half - 1, half, q - 1, rng.randrange(1, half), rng.randrange(1, half)]
        # ties and near-ties of the conversion to double: 53 bits kept, at every position the integer allows
        for top in range(54, q.bit_length()):
            low = top - 54  # the bit below the last one kept
            base = (1 << top) | (1 << (low + 1))
            norms += [(1 << top) + (1 << low), base + (1 << low), (1 << top) + (1 << low) + 1, base + (1 << low) - 1]
        equal = 0
        for norm in norms:
            if norm >= q:
                continue
            ours = ctx.noise_budget_from_norm(norm, count, variable_time=True)
            expected = ref.noise_budget(norm, moduli[:count])
            assert abs(ours - expected) <= math.ulp(expected), (norm, ours, expected)
            equal += ours == expected
        print(f"{bits} x{count}: {equal} of {len(norms)} budgets equal Python's, the rest within one ulp")
        assert ctx.noise_budget_from_norm(0, count) == math.inf


def _budget_status(ctx, word_bits, count, variable_time):
    limbs = (ctypes.c_uint64 * 16)(1)
    out = ctypes.c_double(-1.0)
    status = heamd.load_library().he_bfv_noise_budget_from_norm(ctx.h, word_bits, count, limbs, variable_time, ctypes.byref(out))
    return heamd.binding.STATUS_NAMES[status]


# the composed width against one word of T (Bfv+Decrypt.swift:151-173), for both words: sets on either side of the switch
@pytest.mark.parametrize("word_bits,bits,small", [
    (64, [62], False), (64, [31, 31], False), (64, [32, 32], False), (64, [55, 55, 55, 55], False), (64, [50] * 16, False),
    (32, [30], False), (32, [15, 15], False), (32, [16, 16], False), (32, [27, 28, 28], False), (32, [26] * 16, False),
])
def test_width_rule(word_bits, bits, small):
    degree = 8
    ctx, moduli = _host_context(bits, small, degree, t_bits=5 if min(bits) < 20 else 17)
    assert ctx.t < min(moduli)
    for count in range(1, ctx.L + 1):
        needs = ref.needs_variable_time(moduli[:count], word_bits)
        assert _budget_status(ctx, word_bits, count, 1) == "ok"
        assert _budget_status(ctx, word_bits, count, 0) == ("invalidArgument" if needs else "ok"), (count, needs)
    # what the cases were chosen for
    top = ref.needs_variable_time(moduli, word_bits)
    assert top is (None if bits in ([62], [31, 31], [30], [15, 15]) else True)


def test_budget_argument_errors():
    ctx, _ = _host_context([30, 30], False)
    assert _budget_status(ctx, 16, 1, 1) == "invalidArgument"
    assert _budget_status(ctx, 64, 0, 1) == "invalidArgument"
    assert _budget_status(ctx, 64, ctx.L + 1, 1) == "invalidArgument"
    lib = heamd.load_library()
    assert heamd.binding.STATUS_NAMES[lib.he_bfv_noise_budget_from_norm(ctx.h, 64, 1, None, 1, None)] == "invalidArgument"
    # the device entries refuse a host-only context before anything else about the slabs
    assert heamd.binding.STATUS_NAMES[lib.he_bfv_decrypt_device(ctx.h, 64, 1, 2, 0, None, None, 1, None, 1, None, 0, None)] == \
        "deviceError"
    assert lib.he_bfv_decrypt_workspace_bytes(ctx.h, 64, 2, 2, 0, 3) == (3 * 2 * 8 + 3 * 1 * 2 * 8) * 8  # the dot product, c1's copy
    assert lib.he_bfv_decrypt_workspace_bytes(ctx.h, 32, 2, 3, 1, 3) == 3 * 2 * 8 * 4
    assert lib.he_bfv_decrypt_workspace_bytes(ctx.h, 64, 2, 1, 0, 3) == 3 * 2 * 8 * 8
    assert lib.he_bfv_decrypt_workspace_bytes(ctx.h, 64, 2, 3, 0, 3) == (3 * 2 * 8 + 3 * 2 * 2 * 8) * 8  # c1 and c2
    assert lib.he_bfv_decrypt_workspace_bytes(ctx.h, 64, 3, 2, 0, 3) == 0 == lib.he_bfv_decrypt_workspace_bytes(ctx.h, 64, 2, 4, 0, 3)
