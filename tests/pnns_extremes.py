"""Worst-case inputs for the PNNS response (he_pnns_mul_transpose_device and its twins), and the launcher's choice of kernel
form and fold cadence restated in Python, so that a test can say which path of pnns_bsgs_inner_product_kernel its shape takes
and prove that a fold is crossed.  Held to the oracle by tests/test_pnns_extremes.py; used by tests/test_gpu_pnns_moduli.py.

The matrix of mulTranspose is Eval words and any canonical words are valid, so it is set directly.  The rotated query rows go
through rotations and an NTT, so they are steered:
  * polynomial 0 of the query is the constant polynomial q_i - 1 (coefficient 0 is q_i - 1, the rest 0) in every residue row,
    polynomial 1 is uniform random;
  * the Galois key of the rotation by -1 is all zero words; the key of -babyStep stays uniform random.
A Galois automorphism fixes a constant polynomial; the key switch of polynomial 1 under a zero key is the inner product 0, and
0 divided and rounded by the special modulus is 0.  Every rotated state therefore has polynomial 0 equal to the constant
q_i - 1, whose Eval row is q_i - 1 in every slot (and, past the first state, polynomial 1 equal to 0).  Against a plaintext of
words q_i - 1 every term of polynomial 0's sum is (q_i - 1)^2, the largest a canonical operand pair can make."""
import numpy as np

TILE_LIMIT = 128 << 10   # LDS bytes of a workgroup's rotated rows: baby_step x queries x 2 KiB (kPnnsBsgsTileLimit)
NARROW_CADENCE = 64      # kNarrowProductSumCadence
WORD32_CADENCE = 15      # 15 x 2^60 + a folded residue stays below 2^64


def uniform_words(rng, moduli, shape_before, degree):
    """[*shape_before][len(moduli)][N] canonical words."""
    rows = [rng.integers(0, q, size=tuple(shape_before) + (degree,), dtype=np.uint64) for q in moduli]
    return np.stack(rows, axis=len(shape_before))


def top_words(moduli, degree):
    """[len(moduli)][N]: q_i - 1 everywhere."""
    return np.repeat((np.array(moduli, dtype=np.uint64) - np.uint64(1))[:, None], degree, axis=1)


def worst_case_query(rng, ciphertext_moduli, special_modulus, degree, queries):
    """-> (query [Q][2][L][N] Coeff, keys: per query [key of -1 (zero words), key of -babyStep (uniform)], each
    [L][2][L + 1][N]).  Polynomial 1 and the -babyStep key differ per query."""
    L = len(ciphertext_moduli)
    ks_moduli = list(ciphertext_moduli) + [special_modulus]
    query = uniform_words(rng, ciphertext_moduli, (queries, 2), degree)
    query[:, 0] = 0
    query[:, 0, :, 0] = np.array(ciphertext_moduli, dtype=np.uint64) - np.uint64(1)
    keys = [[np.zeros((L, 2, L + 1, degree), dtype=np.uint64), uniform_words(rng, ks_moduli, (L, 2), degree)]
            for _ in range(queries)]
    return query, keys


def worst_case_matrix(rng, moduli, degree, padded_cols, result_count, baby_step):
    """[padded_cols x result_count][L][N] Eval words, plaintext (diagonal d, result c) at d x result_count + c: all q_i - 1 for
    result 0 (every result where there is one only) and for every result of a ragged last giant step; q_i - 1 on the even
    words and uniform words elsewhere for the others."""
    top = top_words(moduli, degree)
    matrix = uniform_words(rng, moduli, (padded_cols, result_count), degree)
    matrix[:, :, :, ::2] = top[None, None, :, ::2]
    matrix[:, 0] = top
    giant_step = -(-padded_cols // baby_step)
    if padded_cols % baby_step != 0:
        matrix[baby_step * (giant_step - 1):] = top
    return matrix.reshape(padded_cols * result_count, len(moduli), degree)


def rotated_rows(oracle_bfv, query, key_one, element_one, baby_step):
    """The states mulTranspose(vector:) rotates to (tests/pnns_reference.py mul_transpose_vector, its first loop), in Eval:
    [baby_step][2][L][N]."""
    ring = oracle_bfv.ciphertext_context()
    states, state = [], query
    for step in range(baby_step):
        states.append(ring.forward_ntt(state))
        if step != baby_step - 1:
            state = oracle_bfv.apply_galois(state, element_one, key_one)[0]
    return np.stack(states)


def is_worst_case(rotated, moduli):
    """Polynomial 0 of every rotated state is q_i - 1 in every slot."""
    top = top_words(moduli, rotated.shape[-1])
    return bool(np.all(rotated[:, 0] == top[None]))


# ---- the launcher's dispatch (pnns_api.cpp mul_transpose, pnns_kernels.hip launch_pnns_bsgs_inner_product) --------------------
def max_lazy(moduli):
    """PolyContext.maxLazyProductAccumulationCount (PolyContext.swift:246-253): products of the largest modulus a 128-bit
    accumulator takes."""
    q_max = max(moduli)
    return min(((1 << 128) - 1 - q_max) // ((q_max - 1) ** 2), (1 << 63) - 1)


def carry_counting_cadence(moduli):
    """min_i floor((2^127 - q_i) / (q_i - 1)^2): a sum that restarts from a folded residue below q_i stays below 2^127."""
    return min(((1 << 127) - q) // ((q - 1) ** 2) for q in moduli)


def queries_per_pass(degree, moduli_count, baby_step, queries, word_bytes=8):
    vector = 16 // word_bytes
    if (moduli_count * degree) % (64 * vector) != 0 or degree < 64 * vector:
        return 1
    per_pass = min(queries, 4)
    while per_pass > 0 and baby_step * 2 * per_pass * 1024 > TILE_LIMIT:
        per_pass -= 1
    return max(per_pass, 1)


def kernel_form(degree, moduli, baby_step, queries_in_pass, word_bytes=8):
    """-> (form, cadence).  form: "narrow" / "wide" (8-byte words, the LDS tile, carry-counting sums without / with the middle
    column's carry counts), "fast" (4-byte words, the tile, 64-bit sums) or "general" (no tile, one query, per-lane modulus:
    128-bit sums on 8-byte words, 64-bit sums on 4-byte words).  cadence: terms between folds of a lazy sum."""
    vector = 16 // word_bytes
    tiled = ((len(moduli) * degree) % (64 * vector) == 0 and degree >= 64 * vector and
             baby_step * 2 * queries_in_pass * 1024 <= TILE_LIMIT)
    if word_bytes == 4:
        return ("fast" if tiled else "general"), min(WORD32_CADENCE, max_lazy(moduli))
    if not tiled:
        return "general", max_lazy(moduli)
    cadence = min(carry_counting_cadence(moduli), max_lazy(moduli))
    if all(q < (1 << 56) for q in moduli):
        return "narrow", min(cadence, NARROW_CADENCE)
    return "wide", cadence


def in_loop_folds(length, cadence):
    """Folds taken inside an item of `length` terms: every `cadence` terms, the one that coincides with the item's end being
    the item's own reduction."""
    return (length - 1) // cadence
