"""tests/pnns_matrix_reference.py checked on the CPU: with real encryption and real Galois keys the decrypted, SIMD-decoded,
dense-column-unpacked result of mulTranspose(matrix:) is matrix x query^T mod t, for every shape tests/test_gpu_pnns_matrix.py
runs at N = 64 and one at N = 256; and the (lower, period, copies) mask rule equals the reference's list construction.

Parameters: t a 17-bit NTT prime, q three (N = 64) or two (N = 256) 40-bit moduli.  Values are bounded so |row . query| <
t / 2.  Noise: two plaintext multiplications (mask, matrix) grow a fresh error of ~2^5 by at most N t / 2 each, < 2^51 at N =
64 against q / 2t > 2^102, and < 2^57 at N = 256 (L = 2) against q / 2t > 2^62; the key switches add far less."""
import numpy as np
import pytest

import heamd
import pnns_matrix_reference as pm
import pnns_reference as pnns
from bfv_helpers import BfvClient

# (N, rows, cols, R, pack plans)
SHAPES = [
    (64, 10, 4, 3, [[(10, 1)], [(8, 1), (2, 1)]]),
    (64, 10, 4, 5, [[(10, 1)]]),
    (64, 10, 4, 7, [[(2, 1), (8, 1)]]),
    (64, 10, 4, 20, [[(10, 1)]]),
    (64, 10, 32, 3, [[(10, 1)]]),
    (64, 32, 4, 3, [[]]),
    (64, 70, 4, 3, [[]]),
    (64, 10, 4, 1, [[]]),
    (64, 3, 4, 5, [[(1, 3)]]),
    (256, 20, 100, 2, [[(20, 1)]]),
]


def element_of_for(degree):
    def element_of(step):
        if step == "swap":
            return heamd.galois_element_swapping_rows(degree)
        return heamd.galois_element_rotating_columns(step, degree)

    return element_of


_contexts = {}


def context(oracle, degree):
    if degree not in _contexts:
        t = oracle.generate_primes([17], True, degree)[0]
        q = oracle.generate_primes([40, 40, 40, 41] if degree == 64 else [40, 40, 41], False, degree)
        _contexts[degree] = (t, oracle.BfvContext(degree, t, q), pnns.SimdEncoder(oracle, degree, t))
    return _contexts[degree]


@pytest.mark.parametrize("degree,rows,cols,row_count,plans", SHAPES)
def test_decrypted_result_is_the_matrix_product(oracle, degree, rows, cols, row_count, plans):
    t, ref, encoder = context(oracle, degree)
    rng = np.random.default_rng(rows * 1000 + cols * 10 + row_count)
    bound = int(np.sqrt((t // 2 - 1) // cols))
    data = rng.integers(-bound, bound + 1, size=(rows, cols))
    queries = rng.integers(-bound, bound + 1, size=(row_count, cols))
    baby_step, _ = pnns.baby_step_giant_step(cols)
    matrix_eval, outside = pnns.diagonal_matrix(ref, encoder, data.reshape(-1), rows, cols, baby_step, False)
    assert not outside
    element_of = element_of_for(degree)
    client = BfvClient(oracle, ref, seed=rows + row_count)
    slots = pm.dense_row_slots(np.mod(queries, t), row_count, cols, degree)
    query = np.stack([client.encrypt([int(v) for v in coefficients]) for coefficients in encoder.encode(slots)])
    steps = {-1, -baby_step, "swap", pnns.next_power_of_two(cols)} | {step for plan in plans for step, _ in plan}
    keys = pm.Keys(ref, {element_of(step): client.galois_key(element_of(step)) for step in steps
                         if step == "swap" or 0 < abs(step) < degree // 2})
    expected = np.mod(data @ queries.T, t).astype(np.uint64)
    for plan in plans:
        result = pm.mul_transpose_matrix(ref, encoder, element_of, matrix_eval, rows, cols, baby_step, query, row_count,
                                         plan, keys)
        assert result.shape[0] == pm.result_ciphertext_count(degree, rows, row_count)
        for moduli_count in (None, 1):
            down = result
            if moduli_count == 1:
                for level in range(ref.L, 1, -1):
                    down = ref.mod_switch_down(down, 2, level)
            decoded = encoder.decode(np.array([client.decrypt(ct, moduli_count) for ct in down], dtype=np.uint64))
            assert np.array_equal(pm.unpack_dense_column(decoded, rows, row_count, degree), expected), (plan, moduli_count)


def test_dense_row_slots_of_one_row_is_the_repeated_vector():
    vector = [3, 1, 4, 1, 5]
    assert np.array_equal(pm.dense_row_slots(vector, 1, 5, 64)[0], pnns.dense_row_vector_slots(vector, 64))


@pytest.mark.parametrize("degree", [16, 64])
def test_mask_rule_equals_the_list_construction(degree):
    for cols in range(1, degree // 2 + 1):
        for row_count in range(2, 41):
            for row_index in range(row_count):
                mask, copies = pm.mask_list(row_index, row_count, cols, degree)
                lower, period, rule_copies = pm.mask_rule(row_index, row_count, cols, degree)
                assert copies == rule_copies and pm.rotate_count(copies, cols, degree) >= 0
                assert np.array_equal(pm.mask_from_rule(lower, period, copies, cols, degree), np.array(mask, dtype=np.uint64)), \
                    (degree, cols, row_count, row_index)
