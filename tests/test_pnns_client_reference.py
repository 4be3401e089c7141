"""tests/pnns_client_reference.py held to itself and to Python's own arithmetic, without a device: compose against the textbook
CRT, the closed form of the dense-row packing against the line-by-line restatement and against unpackDenseRow, the line-by-line
unpackDenseColumn against the inverse of the packing loop, the float scaling where Float(Int64) rounds, and -- for the shapes and
scaling factors tests/test_gpu_pnns_client.py runs end to end -- that the integer products stay inside the centred range, so
that the restated fixedPointCosineSimilarity is exact there."""
import fractions

import numpy as np
import pytest

import pnns_client_reference as client
import pnns_matrix_reference as pm
import pnns_reference as pnns

# (N, rows, cols): the shapes of the GPU file, see there for the branch each reaches
DENSE_ROW_SHAPES = [(64, 1, 4), (64, 3, 4), (64, 5, 3), (64, 20, 4), (64, 27, 4), (64, 3, 32), (64, 16, 4), (64, 8, 4), (64, 40, 2),
                    (1024, 5, 16), (4096, 3, 16)]
DENSE_COLUMN_SHAPES = [(64, 10, 3), (64, 10, 5), (64, 10, 7), (64, 32, 3), (64, 70, 3), (64, 33, 2), (64, 64, 2), (1024, 100, 5)]
# (N, plaintext moduli, database rows, cols, query rows): the end-to-end cases; moduli as the GPU file draws them
T17, T17B = 65537, 114689  # NTT-friendly for N = 64 and N = 1024: 1 mod 2048
END_TO_END = [(64, [T17], 10, 4, 5), (64, [T17, T17B], 10, 4, 5), (1024, [T17], 100, 16, 5)]


def test_the_moduli_are_what_the_gpu_file_assumes():
    for t in (T17, T17B):
        assert t % 2048 == 1 and all(t % p for p in range(2, int(t ** 0.5) + 1))
    assert T17 * T17B > 1 << 26  # Float(signed) rounds


@pytest.mark.parametrize("moduli", [[T17], [T17, T17B], [T17, T17B, 12289], [(1 << 31) - 1, (1 << 31) - 19]])
def test_compose_is_the_chinese_remainder(moduli):
    composer = client.CrtComposer(moduli)
    q = composer.q
    rng = np.random.default_rng(len(moduli))
    values = [0, 1, q - 1, (q - 1) >> 1, ((q - 1) >> 1) + 1] + [int(v) for v in rng.integers(0, q, size=200, dtype=np.uint64)]
    values += [q - t for t in moduli] + [t - 1 for t in moduli]
    for x in values:
        residues = [x % t for t in moduli]
        textbook = sum(r * (q // t) * pow(q // t, -1, t) for r, t in zip(residues, moduli)) % q
        assert composer.compose(residues) == textbook == x
    # extreme residues, every combination of 0 and t - 1
    for mask in range(1 << len(moduli)):
        residues = [(t - 1) if mask >> i & 1 else 0 for i, t in enumerate(moduli)]
        x = composer.compose(residues)
        assert 0 <= x < q and [x % t for t in moduli] == residues


def test_compose_refuses_a_product_that_does_not_fit():
    with pytest.raises(ValueError):
        client.CrtComposer([(1 << 32) - 5, (1 << 32) - 17])  # 2 q > UInt64.max
    client.CrtComposer([(1 << 62) - 57])  # one modulus: no bound


def test_remainder_to_centered():
    for q in (T17, T17 * T17B, 8):
        assert client.remainder_to_centered((q - 1) >> 1, q) == (q - 1) >> 1
        assert client.remainder_to_centered(((q - 1) >> 1) + 1, q) == ((q - 1) >> 1) + 1 - q
        assert client.remainder_to_centered(q - 1, q) == -1 and client.remainder_to_centered(0, q) == 0


@pytest.mark.parametrize("degree,rows,cols", DENSE_ROW_SHAPES)
def test_dense_row_closed_form_and_unpack(degree, rows, cols):
    rng = np.random.default_rng(degree + 31 * rows + cols)
    residues = rng.integers(1, T17, size=(rows, cols), dtype=np.uint64)  # no zero: padding is told from data
    slots = pm.dense_row_slots(residues, rows, cols, degree)
    assert np.array_equal(client.dense_row_closed_form(residues, rows, cols, degree), slots)
    assert np.array_equal(client.unpack_dense_row(slots, rows, cols, degree), residues)


def test_dense_row_shapes_reach_the_branches_they_are_listed_for():
    def tail(rows, cols, degree=64):
        padded = pnns.next_power_of_two(cols)
        held = rows % (degree // padded)
        return held * padded

    assert tail(3, 4) == 12 and tail(20, 4) == 16          # one SIMD row, padded to 16 and repeated four times / twice
    assert tail(5, 3) == 20                                  # column padding, 20 -> 32: the second SIMD row repeats the first
    assert tail(27, 4) == 44                                 # more than one SIMD row: 12 values of the second padded to 16
    assert tail(8, 4) == 32                                  # exactly one SIMD row
    assert tail(16, 4) == 0 and tail(3, 32) == 32           # full last plaintext / P = N / 2: two rows, then one
    assert tail(40, 2) == 16


@pytest.mark.parametrize("degree,rows,cols", DENSE_COLUMN_SHAPES)
def test_dense_column_unpack_is_the_inverse_of_the_packing(degree, rows, cols):
    """slots are numbered, so the line-by-line unpackDenseColumn and the inverse of the packing loop must pick the same ones"""
    count = pnns.plaintext_count(degree, rows, cols, "denseColumn")
    slots = np.arange(1, count * degree + 1, dtype=np.uint64).reshape(count, degree)
    assert np.array_equal(client.unpack_dense_column(slots, rows, cols, degree), pm.unpack_dense_column(slots, rows, cols, degree))
    with pytest.raises(ValueError):
        client.unpack_dense_column(slots[:-1], rows, cols, degree)


def test_float_scaling_above_2_to_the_24():
    """Float(Int64) rounds to nearest even in one step, then one correctly rounded division: against exact rationals"""
    def nearest_float32(value):
        candidate = np.float32(float(value))  # double is exact for these magnitudes (< 2^53)
        around = [np.nextafter(candidate, np.float32(-np.inf), dtype=np.float32), candidate,
                  np.nextafter(candidate, np.float32(np.inf), dtype=np.float32)]
        best = min(around, key=lambda f: (abs(fractions.Fraction(float(f)) - value), int(f.view(np.uint32)) & 1))
        return best

    q = T17 * T17B
    for scaling_factor in (1, 3, 180, 255, 5000):
        scale = np.float32(scaling_factor)
        divisor = fractions.Fraction(float(np.float32(scale * scale)))
        for signed in (0, 1, -1, (1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 25) + 2, (1 << 25) + 6, (q - 1) >> 1,
                       -((q - 1) >> 1) - 1, (1 << 33) + (1 << 9), (1 << 33) + (1 << 9) + 1, (1 << 33) + 3 * (1 << 9)):
            converted = nearest_float32(fractions.Fraction(signed))
            expected = nearest_float32(fractions.Fraction(float(converted)) / divisor)
            got = client.scale_distance(signed, scaling_factor)
            assert got.dtype == np.float32 and got == expected, (signed, scaling_factor)
    assert client.scale_distance((1 << 24) + 1, 1) == np.float32(1 << 24)      # tie to even: down
    assert client.scale_distance((1 << 24) + 3, 1) == np.float32((1 << 24) + 4)  # tie to even: up


def test_max_scaling_factor():
    # floor(sqrt((t - 1) / 2) - sqrt(d) / 2) in float32
    assert client.max_scaling_factor(4, [T17]) == 180
    assert client.max_scaling_factor(16, [T17]) == 179
    assert client.max_scaling_factor(4, [T17, T17B]) == int(np.floor(np.float32(np.sqrt(np.float32((np.float32(T17) * np.float32(T17B)
                                                                                                    - np.float32(1)) / np.float32(2))))
                                                                     - np.float32(1)))


@pytest.mark.parametrize("degree,moduli,rows,cols,query_rows", END_TO_END)
def test_end_to_end_shapes_stay_inside_the_centred_range(degree, moduli, rows, cols, query_rows):
    """With maxScalingFactor every inner product of two quantised unit vectors is below q / 2 in magnitude, so the centred
    product mod q is the integer product and the restated fixedPointCosineSimilarity is exact on these shapes."""
    scaling_factor = client.max_scaling_factor(cols, moduli)
    q = 1
    for t in moduli:
        q *= t
    rng = np.random.default_rng(degree + rows)
    database = rng.standard_normal((rows, cols)).astype(np.float32)
    queries = rng.standard_normal((query_rows, cols)).astype(np.float32)
    queries[0] = database[3]    # a cosine of one: the largest product there is
    queries[1] = -database[4]
    lhs = pnns.normalized_scaled_and_rounded(database, scaling_factor).astype(object)
    rhs = pnns.normalized_scaled_and_rounded(queries, scaling_factor).astype(object)
    exact = lhs.dot(rhs.T)
    assert max(abs(int(v)) for v in exact.reshape(-1)) <= (q - 1) >> 1
    assert np.array_equal(client.matrix_mul_mod(lhs, rhs.T, q), exact)
    if len(moduli) == 1:  # one modulus: the quantised values themselves must be in the centred range (reduce is off)
        assert max(abs(int(v)) for v in np.concatenate([lhs.reshape(-1), rhs.reshape(-1)])) <= (moduli[0] - 1) >> 1
    distances = client.fixed_point_cosine_similarity(database, queries, q, scaling_factor)
    assert distances.dtype == np.float32 and distances.shape == (rows, query_rows)
    assert abs(float(distances[3, 0]) - 1.0) < 0.05 and abs(float(distances[4, 1]) + 1.0) < 0.05
    # the tail of decrypt(response:) on the residues of the exact products gives the same floats
    residues = [np.vectorize(lambda v, t=t: int(v) % t, otypes=[np.uint64])(exact) for t in moduli]
    assert np.array_equal(client.distances_from_residues(residues, moduli, scaling_factor).view(np.uint32),
                          distances.view(np.uint32))
