"""The PNNS client restated in Python integers and numpy float32 over the restatements already here: what
tests/test_gpu_pnns_client.py holds the device to, itself held to Python's own arithmetic by
tests/test_pnns_client_reference.py.

  Client.generateQuery(for:using:)     PrivateNearestNeighborSearch/Client.swift:74-91
  Client.decrypt(response:using:)      Client.swift:100-127
  unpackDenseRow                       PlaintextMatrix.swift:561-590
  unpackDenseColumn                    PlaintextMatrix.swift:515-555 (line by line; pnns_matrix_reference has the inverse of the
                                       packing loop)
  CrtComposer.init / compose           HomomorphicEncryption/CrtComposer.swift:32-50, 76-97
  remainderToCentered                  ModularArithmetic/Scalar.swift:439-444
  Array2d.mul(_:modulus:),
  fixedPointCosineSimilarity           PrivateNearestNeighborSearch/Util.swift:99-123, 142-151
  ClientConfig.maxScalingFactor        Config.swift:113-120
"""
import numpy as np

import decrypt_reference
import encrypt_reference
import pnns_matrix_reference as pm
import pnns_reference as pnns

UINT64_MAX = (1 << 64) - 1


# ---- the packings ----------------------------------------------------------------------------------------------------------------
def signed_to_residues(values, t, reduce):
    """PlaintextMatrix.init(signedValues:reduce:) (:172-181) -> (residues, a value was out of the centred range)"""
    if reduce:
        return pnns.reduce_signed(values, t), False
    return pnns.centered_to_remainder(values, t)


def dense_row_closed_form(residues, rows, cols, degree):
    """What the packing kernel computes, slot by slot, in closed form: [K][N] slot values.  Held to
    pm.dense_row_slots, the line-by-line restatement, by tests/test_pnns_client_reference.py."""
    data = np.asarray(residues, dtype=np.uint64).reshape(rows, cols)
    padded, half = pnns.next_power_of_two(cols), degree // 2
    per_plaintext = degree // padded
    count = pnns.dividing_ceil(rows, per_plaintext)
    out = np.zeros((count, degree), dtype=np.uint64)
    for p in range(count):
        held = min(rows - p * per_plaintext, per_plaintext)
        length = held * padded
        if held == per_plaintext:
            base, period = 0, degree
        elif length <= half:
            base, period = 0, pnns.next_power_of_two(length)
        else:
            base, period = half, pnns.next_power_of_two(length - half)
        for k in range(degree):
            e = k if k < base else base + (k - base) % period
            row, column = p * per_plaintext + e // padded, e % padded
            if row < rows and column < cols:
                out[p, k] = data[row, column]
    return out


def unpack_dense_row(slots, rows, cols, degree):
    """unpackDenseRow line by line: decoded plaintexts [K][N] -> values [rows][cols]"""
    simd_columns = degree // 2
    padded = pnns.next_power_of_two(cols)
    per_simd_row, pad = simd_columns // padded, padded - cols
    count, values = rows * cols, []
    for decoded in slots:
        for simd_row in range(2):
            for index in range(per_simd_row):
                start = simd_row * simd_columns + index * cols + index * pad
                end = start + min(cols, count - len(values))
                values += [int(v) for v in decoded[start:end]]
                if len(values) == count:
                    return np.array(values, dtype=np.uint64).reshape(rows, cols)
    raise ValueError("wrongEncodingValuesCount")


def unpack_dense_column(slots, rows, cols, degree):
    """unpackDenseColumn line by line: decoded plaintexts [M][N] -> values [rows][cols] (row-major after the transposition)"""
    simd_columns = degree // 2
    columns_per_plaintext = 2 * (simd_columns // rows)
    count, column_major = rows * cols, []
    for decoded in slots:
        decoded = [int(v) for v in decoded]
        if columns_per_plaintext > 1:
            per_simd_row = rows * (simd_columns // rows)
            first = min(per_simd_row, count - len(column_major))
            column_major += decoded[0:first]
            second = min(per_simd_row, count - len(column_major))
            column_major += decoded[simd_columns:simd_columns + second]
        else:
            in_row = len(column_major) % rows
            column_major += decoded[0:min(len(decoded), rows - in_row)]
    if len(column_major) != count:
        raise ValueError("wrongEncodingValuesCount")
    return np.array(column_major, dtype=np.uint64).reshape(cols, rows).T.copy()


# ---- CrtComposer -----------------------------------------------------------------------------------------------------------------
class CrtComposer:
    """init (:32-50) and compose (:76-97) over plaintext moduli, in UInt64 as Client.decrypt instantiates it"""

    def __init__(self, moduli):
        self.moduli = [int(t) for t in moduli]
        self.inverse_punctured = []
        for ti in self.moduli:
            punctured = 1
            for tj in self.moduli:
                if tj != ti:
                    punctured = punctured * tj % ti  # multipliedFullWidth, then reduce
            self.inverse_punctured.append(pow(punctured, -1, ti))
        self.q = 1
        for t in self.moduli:
            self.q *= t
        if len(self.moduli) > 1 and 2 * self.q > UINT64_MAX:  # precondition(Double(V.max) >= composeMaxIntermediateValue)
            raise ValueError("2 q exceeds UInt64.max")

    def compose(self, residues):
        """one column: residues[i] mod moduli[i] -> the value in [0, q)"""
        acc = 0
        for ti, inverse, x in zip(self.moduli, self.inverse_punctured, residues):
            tmp = inverse * int(x) % ti
            addend = (tmp * (self.q // ti)) & UINT64_MAX  # &*
            acc += addend
            assert acc <= UINT64_MAX
            if acc >= self.q:  # addMod
                acc -= self.q
        return acc


def remainder_to_centered(value, modulus):
    return value - modulus if value > (modulus - 1) >> 1 else value


def scale_distance(signed, scaling_factor):
    """Float(signed) / (Float(scalingFactor) * Float(scalingFactor)) in float32: the product first, one division"""
    scale = np.float32(scaling_factor)
    converted = np.array(int(signed), dtype=np.int64).astype(np.float32)  # Float(Int64): one rounding, to nearest even
    return np.float32(converted / np.float32(scale * scale))


def distances_from_residues(values_per_modulus, moduli, scaling_factor):
    """The tail of decrypt(response:): values_per_modulus [contexts][rows][cols] unpacked residues -> float32 [rows][cols]"""
    composer = CrtComposer(moduli)
    values = np.asarray(values_per_modulus, dtype=np.uint64)
    out = np.zeros(values.shape[1:], dtype=np.float32)
    for index in np.ndindex(*out.shape):
        composed = composer.compose([int(values[(i,) + index]) for i in range(len(moduli))])
        out[index] = scale_distance(remainder_to_centered(composed, composer.q), scaling_factor)
    return out


# ---- the client ------------------------------------------------------------------------------------------------------------------
def query_plaintexts(encoder, vectors, scaling_factor, reduce):
    """generateQuery up to encrypt for one context -> (plaintexts [K][N] Coeff, out of range)"""
    vectors = np.asarray(vectors, dtype=np.float32)
    rounded = pnns.normalized_scaled_and_rounded(vectors, scaling_factor)
    residues, outside = signed_to_residues(rounded, encoder.t, reduce)
    slots = pm.dense_row_slots(residues, vectors.shape[0], vectors.shape[1], encoder.degree)
    return encoder.encode(slots), outside


def generate_query(oracle_bfvs, encoders, vectors, scaling_factor, s_eval, a_seeds, error_seeds, stream):
    """Client.generateQuery in Python integers: seeds [contexts][K] of 32 bytes -> [contexts][K][2][L][N] Coeff"""
    out = []
    for c, (bfv, encoder) in enumerate(zip(oracle_bfvs, encoders)):
        plaintexts, _ = query_plaintexts(encoder, vectors, scaling_factor, reduce=len(encoders) > 1)
        ring = bfv.ciphertext_context()
        out.append(np.stack([encrypt_reference.encrypt(ring, encoder.t, [int(v) for v in plaintext], s_eval, a_seeds[c][k],
                                                       error_seeds[c][k], stream)
                             for k, plaintext in enumerate(plaintexts)]))
    return np.stack(out)


def decrypt_response(oracle_bfvs, encoders, response, s_eval, rows, query_rows, scaling_factor, moduli_count=1):
    """Client.decrypt(response:) in Python integers: response [contexts][M][2][moduli_count][N] Coeff -> float32 [rows][query_rows]"""
    unpacked = []
    for bfv, encoder, matrix in zip(oracle_bfvs, encoders, response):
        ring = bfv.ciphertext_context(moduli_count)
        plaintexts = [decrypt_reference.decrypt(decrypt_reference.dot_product(ring, ct, s_eval), ring.moduli, encoder.t)
                      for ct in matrix]
        unpacked.append(unpack_dense_column(encoder.decode(np.array(plaintexts, dtype=np.uint64)), rows, query_rows,
                                            encoder.degree))
    return distances_from_residues(unpacked, [encoder.t for encoder in encoders], scaling_factor)


# ---- what the end-to-end result must be ------------------------------------------------------------------------------------------------
def matrix_mul_mod(lhs, rhs, modulus):
    """Array2d<SignedScalar>.mul(_:modulus:): the centred product mod `modulus`, on Python integers"""
    lhs, rhs = np.asarray(lhs).astype(object), np.asarray(rhs).astype(object)
    product = lhs.dot(rhs) % modulus
    return np.vectorize(lambda v: remainder_to_centered(int(v), modulus), otypes=[object])(product)


def fixed_point_cosine_similarity(database, queries, modulus, scaling_factor):
    """database.fixedPointCosineSimilarity(queries.transposed(), modulus:, scalingFactor:) -> float32 [rows][query_rows].
    (rhs.transposed().normalizedScaledAndRounded().transposed() normalises the query vectors by row, as generateQuery does.)"""
    lhs = pnns.normalized_scaled_and_rounded(database, scaling_factor)
    rhs = pnns.normalized_scaled_and_rounded(queries, scaling_factor).T
    product = matrix_mul_mod(lhs, rhs, modulus)
    out = np.zeros(product.shape, dtype=np.float32)
    for index in np.ndindex(*product.shape):
        out[index] = scale_distance(product[index], scaling_factor)
    return out


def max_scaling_factor(vector_dimension, plaintext_moduli):
    """ClientConfig.maxScalingFactor for cosine similarity, in float32"""
    t = np.float32(1)
    for modulus in plaintext_moduli:
        t = np.float32(t * np.float32(modulus))
    root = np.sqrt(np.float32((t - np.float32(1)) / np.float32(2)), dtype=np.float32)
    return int(np.floor(np.float32(root - np.float32(np.sqrt(np.float32(vector_dimension), dtype=np.float32) / np.float32(2)))))
