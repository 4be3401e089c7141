"""Holds tests/pnns_extremes.py to the oracle: the query and keys it builds do rotate to states whose polynomial 0 is q_i - 1
in every Eval slot, and the fold cadence it restates is the one the 62-bit cases of tests/test_gpu_pnns_moduli.py count on.
CPU only."""
import numpy as np
import pytest

import pnns_extremes as extremes


@pytest.mark.parametrize("degree", [64, 1024])
def test_rotated_states_are_the_worst_case(oracle, degree):
    import heamd  # the Galois element helper is host-side arithmetic

    baby_step, queries = 16, 2
    t = oracle.generate_primes([17], True, degree)[0]
    q = oracle.generate_primes([62, 62, 62, 62], False, degree)
    assert len(set(q)) == 4 and all(m >> 61 == 1 for m in q)
    ref = oracle.BfvContext(degree, t, q)
    moduli = q[:ref.L]
    query, keys = extremes.worst_case_query(np.random.default_rng(degree), moduli, q[-1], degree, queries)
    assert query.shape == (queries, 2, ref.L, degree) and keys[0][0].shape == keys[0][1].shape == (ref.L, 2, ref.L + 1, degree)
    assert not np.array_equal(query[0, 1], query[1, 1]) and not np.array_equal(keys[0][1], keys[1][1])
    for row, modulus in enumerate(list(moduli) + [q[-1]]):
        assert int(keys[0][1][:, :, row].max()) < modulus
    element = heamd.galois_element_rotating_columns(-1, degree)
    top = extremes.top_words(moduli, degree)
    for k in range(queries):
        rotated = extremes.rotated_rows(ref, query[k], keys[k][0], element, baby_step)
        assert rotated.shape == (baby_step, 2, ref.L, degree)
        for j in range(baby_step):
            assert np.array_equal(rotated[j, 0], top), (k, j)
        assert extremes.is_worst_case(rotated, moduli)
        assert rotated[0, 1].any() and not rotated[1:, 1].any()  # polynomial 1: the query's own, then the zero key's 0
    # the check itself can fail: one word off in one state
    spoiled = rotated.copy()
    spoiled[baby_step - 1, 0, ref.L - 1, degree - 1] -= np.uint64(1)
    assert not extremes.is_worst_case(spoiled, moduli)


def test_worst_case_matrix_layout():
    rng = np.random.default_rng(1)
    moduli, degree = [(1 << 61) + 1, (1 << 44) + 7], 8
    top = extremes.top_words(moduli, degree)
    matrix = extremes.worst_case_matrix(rng, moduli, degree, 16, 3, 6)  # G = 3, the last giant step sums 4
    assert matrix.shape == (48, 2, 8)
    grid = matrix.reshape(16, 3, 2, 8)
    assert np.all(grid[:, 0] == top) and np.all(grid[12:] == top) and np.all(grid[:, :, :, ::2] == top[:, ::2])
    assert not np.all(grid[:12, 1:] == top)
    for row, modulus in enumerate(moduli):
        assert int(grid[:, :, row].max()) < modulus
    single = extremes.worst_case_matrix(rng, moduli, degree, 4, 1, 4)
    assert np.all(single == top)


def test_cadence_and_form_of_the_launcher(oracle):
    degree = 1024
    q62 = oracle.generate_primes([62, 62, 62, 62], False, degree)[:3]
    # 62-bit moduli: 8 products below 2^127, 16 below the reference's 2^128: baby steps 12 and 16 cross the first
    assert extremes.carry_counting_cadence(q62) == min(((1 << 127) - m) // (m - 1) ** 2 for m in q62) == 8
    assert extremes.max_lazy(q62) == 16 == oracle.PolyContext(degree, q62).max_lazy_product_accumulation_count()
    assert extremes.kernel_form(degree, q62, 16, 4) == ("wide", 8)
    assert extremes.kernel_form(degree, q62, 12, 1) == ("wide", 8)
    assert extremes.kernel_form(degree, q62, 128, 1) == ("general", 16)  # a tile beyond LDS
    assert extremes.kernel_form(64, q62, 32, 1) == ("general", 16)       # below one wavefront of 16-byte lanes
    assert extremes.in_loop_folds(16, 8) == 1 and extremes.in_loop_folds(12, 8) == 1 and extremes.in_loop_folds(8, 8) == 0
    assert extremes.in_loop_folds(128, 16) == 7
    mixed = oracle.generate_primes([62, 45, 61, 62], False, degree)[:3]
    assert extremes.kernel_form(degree, mixed, 16, 3) == ("wide", 8)     # the minimum over the rows
    q56 = oracle.generate_primes([56, 55, 56, 57], False, degree)[:3]
    assert all(m < 1 << 56 for m in q56)
    assert extremes.kernel_form(degree, q56, 64, 1) == ("narrow", 64)
    q57 = oracle.generate_primes([57, 56, 57, 58], False, degree)[:3]
    form, cadence = extremes.kernel_form(degree, q57, 16, 2)
    assert form == "wide" and cadence > 64
    q30 = oracle.generate_primes([30, 30, 30, 30], False, degree, word_bits=32)[:3]
    assert all(15 * (m - 1) ** 2 + m < 1 << 64 for m in q30)
    assert extremes.kernel_form(degree, q30, 16, 4, word_bytes=4) == ("fast", 15)
    assert extremes.kernel_form(64, q30, 32, 1, word_bytes=4) == ("general", 15)
    assert extremes.in_loop_folds(16, 15) == 1 and extremes.in_loop_folds(32, 15) == 2
    # queries per pass: baby_step x queries x 2 KiB within 128 KiB, four at most, one without the tile
    assert [extremes.queries_per_pass(degree, 3, b, n) for b, n in ((16, 4), (12, 5), (64, 2), (128, 2))] == [4, 4, 1, 1]
    assert extremes.queries_per_pass(degree, 3, 32, 3, word_bytes=4) == 2
    assert extremes.queries_per_pass(64, 3, 32, 2) == 1 and extremes.queries_per_pass(64, 3, 32, 2, word_bytes=4) == 1
