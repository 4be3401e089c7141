"""Holds tests/pnns_reference.py to the reference: the 4 x 4 diagonal example of MatrixMultiplication.swift:157-166, the
shapes, plaintext counts and decoded plaintexts of _TestUtilities/PnnsUtilities/PlaintextMatrixTests.swift (restated as data in
tests/golden/pnns_plaintext_matrix_kats.json), the unpack and SIMD round trips, the BSGS defaults, and mulTranspose(vector:)
decrypted against the integer product.  CPU only."""
import json
import math
import os
import random

import numpy as np
import pytest

import pnns_reference as pnns
from bfv_helpers import BfvClient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def matrix_kats():
    with open(os.path.join(ROOT, "tests", "golden", "pnns_plaintext_matrix_kats.json")) as f:
        return json.load(f)


def increasing(rows, cols, t):
    return [(1 + i) % t for i in range(rows * cols)]


# rows x cols for degree N: below, at and above one plaintext per diagonal; one column to the SIMD column count
def shape_list(degree):
    rows = sorted({1, degree - 1, degree, degree + 1, 3 * degree + 5})
    cols = sorted({c for c in (1, 2, 5, 16, 100, degree // 2) if c <= degree // 2})
    return [(r, c) for r in rows for c in cols]


def test_diagonal_example_of_the_reference_comment():
    """MatrixMultiplication.swift:157-166: [[1..4], [5..8], [9..12], [13..16]] packs as its four wrapped diagonals; with one
    giant step (babyStep 4) nothing is rotated."""
    slots = pnns.diagonal_slots_loop(list(range(1, 17)), 4, 4, 8, 4)
    assert [list(map(int, row[:4])) for row in slots] == [[1, 6, 11, 16], [2, 7, 12, 13], [3, 8, 9, 14], [4, 5, 10, 15]]
    assert not slots[:, 4:].any()
    # and the product it describes: sum over diagonals of diagonal * (the vector rotated left by the diagonal's index)
    vector = [1, 2, 3, 4]
    total = [sum(int(slots[d][k]) * vector[(k + d) % 4] for d in range(4)) for k in range(4)]
    assert total == [30, 70, 110, 150]


def test_plaintext_counts_of_the_reference_shapes(matrix_kats):
    degree = matrix_kats["degree"]
    for packing in pnns.PACKINGS:
        assert len(matrix_kats[packing]) >= 13
        for case in matrix_kats[packing]:
            got = pnns.plaintext_count(degree, case["rows"], case["cols"], packing)
            assert got == case["plaintext_count"], (packing, case["rows"], case["cols"])


def test_diagonal_plaintexts_of_the_reference_shapes(matrix_kats):
    degree, t = matrix_kats["degree"], matrix_kats["plaintext_modulus"]
    for case in matrix_kats["diagonal"]:
        rows, cols = case["rows"], case["cols"]
        baby_step, _ = pnns.baby_step_giant_step(pnns.next_power_of_two(cols))
        values = increasing(rows, cols, t)
        slots = pnns.diagonal_slots_loop(values, rows, cols, degree, baby_step)
        assert slots.tolist() == case["decoded"], (rows, cols)
        assert np.array_equal(pnns.diagonal_slots(values, rows, cols, degree, baby_step), slots)
        assert pnns.unpack_diagonal(slots, rows, cols, degree, baby_step) == values
    rotation = matrix_kats["diagonal_rotation"]
    degree, rows, cols = rotation["degree"], rotation["rows"], rotation["cols"]
    baby_step, giant_step = pnns.baby_step_giant_step(cols)
    assert (baby_step, giant_step) == (3, 3)
    slots = pnns.diagonal_slots_loop(increasing(rows, cols, t), rows, cols, degree, baby_step)
    expected = [prefix + [0] * (degree - len(prefix)) for prefix in rotation["decoded_prefixes"]]
    assert slots.tolist() == expected


@pytest.mark.parametrize("degree", [8, 64])
def test_unpack_inverts_diagonal_over_the_shape_list(degree):
    rng = random.Random(degree)
    t = 1153
    for rows, cols in shape_list(degree):
        padded = pnns.next_power_of_two(cols)
        steps = {pnns.baby_step_giant_step(cols)[0], padded}
        steps |= {d for d in range(1, padded + 1) if padded % d == 0 and d * d >= padded and d not in steps}
        for baby_step in sorted(steps)[:3]:
            values = [rng.randrange(t) for _ in range(rows * cols)]
            slots = pnns.diagonal_slots_loop(values, rows, cols, degree, baby_step)
            assert len(slots) == pnns.plaintext_count(degree, rows, cols, "diagonal")
            assert np.array_equal(pnns.diagonal_slots(values, rows, cols, degree, baby_step), slots), (rows, cols, baby_step)
            assert pnns.unpack_diagonal(slots, rows, cols, degree, baby_step) == values, (rows, cols, baby_step)


def test_array_form_matches_the_loop_at_a_larger_degree():
    rng = np.random.default_rng(3)
    degree, t = 256, 65537
    for rows, cols, baby_step in ((255, 100, 12), (257, 128, 16), (773, 5, 8), (256, 16, 4)):
        values = rng.integers(0, t, size=rows * cols).tolist()
        assert np.array_equal(pnns.diagonal_slots(values, rows, cols, degree, baby_step),
                              pnns.diagonal_slots_loop(values, rows, cols, degree, baby_step))


@pytest.mark.parametrize("degree,t_bits", [(8, 11), (64, 17), (1024, 20), (8192, 20)])
def test_simd_round_trip(oracle, degree, t_bits):
    t = oracle.generate_primes([t_bits], True, degree)[0]
    encoder = pnns.SimdEncoder(oracle, degree, t)
    assert sorted(encoder.matrix.tolist()) == list(range(degree))
    rng = np.random.default_rng(degree)
    slots = rng.integers(0, t, size=(3, degree), dtype=np.uint64)
    coefficients = encoder.encode(slots)
    assert np.array_equal(encoder.decode(coefficients), slots)
    # slot-wise: the product of two encodings in the ring is the encoding of the slot products
    ring = encoder.ring
    product = ring.inverse_ntt(ring.mul(ring.forward_ntt(coefficients[0][None]), ring.forward_ntt(coefficients[1][None])))
    assert np.array_equal(encoder.decode(product)[0], slots[0] * slots[1] % np.uint64(t))


def test_encoding_matrix_known_answer():
    # degree 8: 3^i mod 16 = 1, 3, 9, 11 -> (g - 1) / 2 = 0, 1, 4, 5 -> bit-reversed over 3 bits; second row: 7 - that
    assert pnns.encoding_matrix(8).tolist() == [0, 4, 1, 5, 7, 3, 6, 2]


def test_baby_step_giant_step_defaults():
    for cols in range(1, 1025):
        baby_step, giant_step = pnns.baby_step_giant_step(cols)
        dimension = pnns.next_power_of_two(cols)
        assert baby_step == math.ceil(math.sqrt(dimension))
        assert giant_step == -(-dimension // baby_step) and baby_step >= giant_step
        assert (baby_step - 1) * (baby_step - 1) < dimension <= baby_step * baby_step
    assert pnns.baby_step_giant_step(128) == (12, 11) and pnns.baby_step_giant_step(5) == (3, 3)
    assert pnns.baby_step_giant_step(100, 16) == (16, 8)
    with pytest.raises(ValueError):
        pnns.baby_step_giant_step(128, 8)  # giantStep 16 > babyStep


def test_quantize_forms_agree_and_round_half_away():
    assert pnns.round_half_away(np.array([0.5, -0.5, 1.5, 2.5, -2.5, 0.49999997, -0.49999997, 8388609.0],
                                         dtype=np.float32)).tolist() == [1, -1, 2, 3, -3, 0, 0, 8388609]
    rng = np.random.default_rng(5)
    vectors = rng.standard_normal((50, 37)).astype(np.float32)
    vectors[7] = 0
    vectors[9, 1:] = 1e-20
    vectors[9, 0] = 3e18
    assert np.array_equal(pnns.normalized_scaled_and_rounded(vectors, 123.0),
                          pnns.normalized_scaled_and_rounded_loop(vectors, 123.0))
    assert not pnns.normalized_scaled_and_rounded(vectors, 123.0)[7].any()
    # exact ties: a row (3, 4) has norm 5; scaling 2.5 gives 1.5 and 2 -> 2 and 2; scaling -2.5 the mirror image
    assert pnns.normalized_scaled_and_rounded(np.array([[3, 4]], dtype=np.float32), 2.5).tolist() == [[2, 2]]
    assert pnns.normalized_scaled_and_rounded(np.array([[3, 4]], dtype=np.float32), -2.5).tolist() == [[-2, -2]]


@pytest.mark.parametrize("rows,cols,baby_step", [(37, 5, None), (64, 16, 8), (150, 7, None)])
def test_mul_transpose_decrypts_to_the_product(oracle, rows, cols, baby_step):
    degree = 64
    t = oracle.generate_primes([17], True, degree)[0]
    q = oracle.generate_primes([40, 40, 40, 41], False, degree)
    ref = oracle.BfvContext(degree, t, q)
    client = BfvClient(oracle, ref, seed=rows)
    encoder = pnns.SimdEncoder(oracle, degree, t)
    import heamd  # the Galois element helpers are host-side arithmetic

    rng = np.random.default_rng(rows * cols)
    bound = 30
    data = rng.integers(-bound, bound + 1, size=(rows, cols))
    vector = rng.integers(-bound, bound + 1, size=cols)
    if baby_step is None:
        baby_step, _ = pnns.baby_step_giant_step(cols)
    matrix, outside = pnns.diagonal_matrix(ref, encoder, data.reshape(-1), rows, cols, baby_step, reduce=False)
    assert not outside and matrix.shape == (pnns.plaintext_count(degree, rows, cols, "diagonal"), ref.L, degree)
    query_slots = pnns.dense_row_vector_slots(np.mod(vector, t), degree)
    query = client.encrypt([int(v) for v in encoder.encode(query_slots)[0]])

    def rotation(step):
        element = heamd.galois_element_rotating_columns(step, degree)
        key = client.galois_key(element)
        return lambda ct: ref.apply_galois(ct, element, key)[0]

    results = pnns.mul_transpose_vector(ref, matrix, rows, cols, baby_step, query, rotation(-1),
                                        rotation(-baby_step) if baby_step < pnns.next_power_of_two(cols) else None)
    decoded = np.concatenate([encoder.decode(np.array(client.decrypt(ct), dtype=np.uint64))[0] for ct in results])
    assert np.array_equal(decoded[:rows], np.mod(data @ vector, t).astype(np.uint64))
