"""The PNNS server database restated from the reference's algorithm in numpy over the CPU oracle: what
tests/test_gpu_pnns.py and tests/test_pnns_shape.py hold the library to, itself held to the reference's own vectors by
tests/test_pnns_reference.py.

  normalizedScaledAndRounded      PrivateNearestNeighborSearch/Util.swift:74-89
  generateEncodingMatrix,
  encodeSimd / decodeSimd         HomomorphicEncryption/Encoding.swift:197-246
  plaintextCount                  PrivateNearestNeighborSearch/PlaintextMatrix.swift:246-275
  BabyStepGiantStep               PrivateNearestNeighborSearch/MatrixMultiplication.swift:25-61
  diagonalPlaintexts              PlaintextMatrix.swift:417-483
  unpackDiagonal                  PlaintextMatrix.swift:588-643
  mulTranspose(vector:)           MatrixMultiplication.swift:131-226
"""
import math

import numpy as np

PACKINGS = ("denseColumn", "denseRow", "diagonal")  # MatrixPacking's case order


def next_power_of_two(x):
    return 1 if x <= 1 else 1 << (int(x) - 1).bit_length()


def dividing_ceil(a, b):
    return -(-a // b)


# ---- Array2d<Float>.normalizedScaledAndRounded ---------------------------------------------------------------------------
def round_half_away(x):
    """Float.rounded() (toNearestOrAwayFromZero) on float32 values, exactly: x - trunc(x) is exact in float32."""
    x = np.asarray(x, dtype=np.float32)
    whole = np.trunc(x)
    return whole + np.where(np.abs(x - whole) >= np.float32(0.5), np.sign(x), np.float32(0)).astype(np.float32)


def normalized_scaled_and_rounded(vectors, scaling_factor):
    """row.map { $0 * $0 }.reduce(0, +).squareRoot(), then (value * scalingFactor / norm).rounded(): every step in float32,
    the sum left to right (np.cumsum is sequential; np.sum is pairwise)."""
    vectors = np.ascontiguousarray(vectors, dtype=np.float32)
    scale = np.float32(scaling_factor)
    squares = vectors * vectors
    sums = np.cumsum(squares, axis=1, dtype=np.float32)[:, -1]
    norms = np.sqrt(sums, dtype=np.float32)
    out = np.zeros(vectors.shape, dtype=np.int64)
    live = norms != 0
    with np.errstate(all="ignore"):
        quotient = (vectors[live] * scale) / norms[live][:, None]
    out[live] = round_half_away(quotient).astype(np.int64)
    return out


def normalized_scaled_and_rounded_loop(vectors, scaling_factor):
    """The same with the explicit sequential loop (small inputs: it pins the cumsum form)."""
    vectors = np.asarray(vectors, dtype=np.float32)
    out = np.zeros(vectors.shape, dtype=np.int64)
    for r, row in enumerate(vectors):
        total = np.float32(0)
        for v in row:
            total = np.float32(total + np.float32(v * v))
        norm = np.float32(np.sqrt(total))
        if norm == 0:
            continue
        for c, v in enumerate(row):
            out[r, c] = int(round_half_away(np.float32(np.float32(v * np.float32(scaling_factor)) / norm)))
    return out


# ---- signed values -> residues -----------------------------------------------------------------------------------------------
def centered_to_remainder(values, t):
    """SignedScalar.centeredToRemainder (ModularArithmetic/Scalar.swift:85-94) -> (residues, any value out of range)."""
    values = np.asarray(values, dtype=np.int64)
    outside = bool(np.any((values > (t - 1) >> 1) | (values < -(t >> 1))))
    return np.where(values < 0, values + t, values).astype(np.uint64), outside


def reduce_signed(values, t):
    """Modulus.reduce(SignedScalar) (ModularArithmetic/Modulus.swift:292-297): the remainder in [0, t)."""
    return np.mod(np.asarray(values, dtype=np.int64), np.int64(t)).astype(np.uint64)


# ---- SIMD encoding ---------------------------------------------------------------------------------------------------------
def reverse_bits(x, bit_count):
    out = 0
    for _ in range(bit_count):
        out = (out << 1) | (x & 1)
        x >>= 1
    return out


def encoding_matrix(degree):
    """generateEncodingMatrix: slot -> index of the Eval-form slab (GaloisElementGenerator.value = 3)."""
    log_degree = degree.bit_length() - 1
    row_size, mask = degree >> 1, (degree << 1) - 1
    matrix = [0] * degree
    power = 1
    for i in range(row_size):
        matrix[i] = reverse_bits((power - 1) >> 1, log_degree)
        matrix[row_size | i] = reverse_bits((mask - power) >> 1, log_degree)
        power = (power * 3) & mask
    return np.array(matrix, dtype=np.int64)


class SimdEncoder:
    """encodeSimd / decodeSimd through the oracle's NTT on the [t] poly context (plaintextContext)."""

    def __init__(self, oracle, degree, t, threads=1):
        self.degree, self.t, self.threads = degree, t, threads
        self.ring = oracle.PolyContext(degree, [t])
        self.matrix = encoding_matrix(degree)

    def encode(self, slots):
        """[batch][N] slot values mod t -> [batch][N] coefficients (Plaintext<Coeff>)."""
        slots = np.asarray(slots, dtype=np.uint64).reshape(-1, self.degree)
        slab = np.zeros_like(slots)
        slab[:, self.matrix] = slots
        return self.ring.inverse_ntt(slab[:, None, :], threads=self.threads)[:, 0, :]

    def decode(self, coefficients):
        coefficients = np.asarray(coefficients, dtype=np.uint64).reshape(-1, self.degree)
        slab = self.ring.forward_ntt(coefficients[:, None, :], threads=self.threads)[:, 0, :]
        return slab[:, self.matrix]


# ---- shapes -----------------------------------------------------------------------------------------------------------------
def plaintext_count(degree, rows, cols, packing):
    """PlaintextMatrix.plaintextCount; ValueError where the reference throws invalidMatrixDimensions."""
    if rows <= 0 or cols <= 0:
        raise ValueError("invalidMatrixDimensions")
    simd_columns = degree // 2
    if packing == "denseColumn":
        columns_per_plaintext = 2 * (simd_columns // rows)
        if columns_per_plaintext > 1:
            return dividing_ceil(cols, columns_per_plaintext)
        return cols * dividing_ceil(rows, degree)
    if packing == "denseRow":
        if cols > simd_columns:
            raise ValueError("invalidMatrixDimensions")
        return dividing_ceil(rows, 2 * (simd_columns // next_power_of_two(cols)))
    if packing == "diagonal":
        if cols > simd_columns:  # diagonalPlaintexts' guard
            raise ValueError("invalidMatrixDimensions")
        return next_power_of_two(cols) * dividing_ceil(rows, degree)
    raise ValueError("unknown packing")


def baby_step_giant_step(vector_dimension, baby_step=None):
    """BabyStepGiantStep(vectorDimension:) / (vectorDimension:babyStep:) -> (babyStep, giantStep); ValueError on the
    reference's precondition babyStep >= giantStep."""
    dimension = next_power_of_two(vector_dimension)
    if baby_step is None:
        baby_step = math.isqrt(dimension)
        if baby_step * baby_step < dimension:  # Double(dimension).squareRoot().rounded(.up)
            baby_step += 1
    giant_step = dividing_ceil(dimension, baby_step)
    if baby_step < giant_step:
        raise ValueError("babyStep cannot be smaller than giantStep")
    return baby_step, giant_step


# ---- diagonal packing ------------------------------------------------------------------------------------------------------
def rotate_to_start_at(values, index):
    """MutableCollection.rotate(toStartAt:): the element at `index` becomes the first."""
    return values[index:] + values[:index]


def diagonal_slots_loop(values, rows, cols, degree, baby_step):
    """diagonalPlaintexts up to context.encode(values: chunk, format: .simd), line by line: the SIMD slot values of every
    plaintext, [plaintext_count][N].  values: residues mod t, row-major."""
    data = [list(values[r * cols:(r + 1) * cols]) for r in range(rows)]
    padded = next_power_of_two(cols)
    packed = [[0] * rows for _ in range(padded)]
    for row_index in range(padded):
        for column_index in range(rows):
            padded_column = (column_index + row_index) % padded
            if padded_column < cols:
                packed[row_index][column_index] = data[column_index][padded_column]
    expected = plaintext_count(degree, rows, cols, "diagonal")
    per_column = expected // padded
    plaintexts = []
    for row_index in range(padded):
        row = packed[row_index]
        for chunk_index in range(dividing_ceil(len(row), degree)):
            chunk = row[chunk_index * degree:(chunk_index + 1) * degree]
            chunk = chunk + [0] * (degree - len(chunk))
            i = (len(plaintexts) - chunk_index) // per_column
            rotation_step = i - i % baby_step  # previousMultiple(of: babyStep)
            if rotation_step != 0:
                middle = degree // 2
                chunk = rotate_to_start_at(chunk[:middle], middle - rotation_step) + \
                    rotate_to_start_at(chunk[middle:], middle - rotation_step)
            plaintexts.append(chunk)
    assert len(plaintexts) == expected
    return np.array(plaintexts, dtype=np.uint64)


def diagonal_slots(values, rows, cols, degree, baby_step, block=64, first_diagonal=0, diagonal_count=None):
    """diagonal_slots_loop in array form (pinned to it by tests/test_pnns_reference.py): slot k of plaintext (r, c) is
    data[R][(R + r) mod P] with R = c N + ((k & h) | ((k - s) & (h - 1))), s = r - r mod babyStep, h = N / 2.
    first_diagonal / diagonal_count: only the plaintexts of those diagonals."""
    data = np.asarray(values, dtype=np.uint64).reshape(rows, cols)
    padded = next_power_of_two(cols)
    per_column = dividing_ceil(rows, degree)
    half = degree // 2
    k = np.arange(degree, dtype=np.int64)
    last_diagonal = padded if diagonal_count is None else first_diagonal + diagonal_count
    out = np.zeros((last_diagonal - first_diagonal, per_column, degree), dtype=np.uint64)
    for first in range(first_diagonal, last_diagonal, block):
        r = np.arange(first, min(first + block, last_diagonal), dtype=np.int64)[:, None, None]
        step = r - r % baby_step
        source = (k & half) | ((k - step) & (half - 1))                       # [r][1][N]
        row = np.arange(per_column, dtype=np.int64)[None, :, None] * degree + source  # [r][c][N]
        column = (row + r) & (padded - 1)
        live = (row < rows) & (column < cols)
        picked = data[np.where(live, row, 0), np.where(live, column, 0)]
        out[first - first_diagonal:first - first_diagonal + r.shape[0]] = np.where(live, picked, np.uint64(0))
    return out.reshape(-1, degree)


def unpack_diagonal(slots, rows, cols, degree, baby_step):
    """unpackDiagonal on decoded plaintexts [plaintext_count][N] -> the row-major values."""
    padded = next_power_of_two(cols)
    per_column = len(slots) // padded
    middle = degree // 2
    packed = []
    group = baby_step * per_column
    for chunk_index in range(dividing_ceil(len(slots), group)):
        rotation_step = chunk_index * baby_step
        rotated = []
        for decoded in slots[chunk_index * group:(chunk_index + 1) * group]:
            decoded = [int(v) for v in decoded]
            rotated.append(rotate_to_start_at(decoded[:middle], rotation_step) +
                           rotate_to_start_at(decoded[middle:], rotation_step))
        for d in range(0, len(rotated), per_column):
            packed.append([v for part in rotated[d:d + per_column] for v in part][:rows])
    values = [[0] * cols for _ in range(rows)]
    count = 0
    for row_index in range(len(packed)):
        for column_index in range(rows):
            value_column = (row_index + column_index) % padded
            if value_column < cols:
                values[column_index][value_column] = packed[row_index][column_index]
                count += 1
    assert count == rows * cols
    return [v for row in values for v in row]


def diagonal_matrix(oracle_bfv, encoder, signed_values, rows, cols, baby_step, reduce, moduli_count=None, first_diagonal=0,
                    diagonal_count=None):
    """PlaintextMatrix(.diagonal(bsgs), signedValues:reduce:).convertToEvalFormat(moduliCount:) ->
    ([plaintext_count][L][N] Eval words, out of range); first_diagonal / diagonal_count: only those diagonals' plaintexts."""
    t = encoder.t
    if reduce:
        residues, outside = reduce_signed(signed_values, t), False
    else:
        residues, outside = centered_to_remainder(signed_values, t)
    slots = diagonal_slots(residues, rows, cols, encoder.degree, baby_step, first_diagonal=first_diagonal,
                           diagonal_count=diagonal_count)
    return oracle_bfv.plaintext_to_eval(encoder.encode(slots), moduli_count), outside


def dense_row_vector_slots(vector, degree):
    """denseRowPlaintexts (PlaintextMatrix.swift:341-406) of a 1 x cols matrix: the padded row repeated over every slot."""
    padded = next_power_of_two(len(vector))
    row = list(vector) + [0] * (padded - len(vector))
    return np.array(row * (degree // padded), dtype=np.uint64)


# ---- mulTranspose(vector:) over the oracle ------------------------------------------------------------------------------------
def mul_transpose_vector(oracle_bfv, matrix_eval, rows, cols, baby_step, query, rotate_one, rotate_baby):
    """matrix_eval [plaintext_count][L][N] Eval, query [2][L][N] Coeff (dense-row packed); rotate_one / rotate_baby:
    ciphertext -> ciphertext rotated by -1 / -babyStep columns (applyGalois with the element's key).  Returns the
    ceil(rows / N) result ciphertexts [2][L][N] Coeff."""
    ring = oracle_bfv.ciphertext_context()
    degree = oracle_bfv.degree
    dimension = next_power_of_two(cols)
    giant_step = dividing_ceil(dimension, baby_step)
    states, state = [], query
    for step in range(baby_step):
        states.append(state)
        if step != baby_step - 1:
            state = rotate_one(state)
    rotated = np.stack([ring.forward_ntt(s) for s in states])
    result_count = dividing_ceil(rows, degree)
    results = []
    for result_index in range(result_count):
        products = []
        for giant in range(giant_step):
            count = min(len(rotated), dimension - baby_step * giant)
            indices = [result_count * (j + baby_step * giant) + result_index for j in range(count)]
            product = oracle_bfv.inner_product_plain(rotated[:count], matrix_eval[indices])
            products.append(ring.inverse_ntt(product))
        accumulator = products.pop()  # rotateColumnsAndSum
        for product in reversed(products):
            accumulator = ring.add(rotate_baby(accumulator), product)
        results.append(accumulator)
    return results
