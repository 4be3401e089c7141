"""PlaintextMatrix.mulTranspose(matrix:using:) for query matrices of several rows, restated from the reference's algorithm in
numpy over the CPU oracle: what tests/test_gpu_pnns_matrix.py and tests/test_pnns_matrix_abi.py hold the library to, itself
checked by tests/test_pnns_matrix_reference.py (real encryption: the decrypted, unpacked result is matrix x query^T).

  denseRowPlaintexts              PrivateNearestNeighborSearch/PlaintextMatrix.swift:341-406
  denseColumnPlaintexts (inverse) PlaintextMatrix.swift:285-331
  extractDenseRow                 CiphertextMatrix.swift:252-370
  mulTranspose(matrix:)           MatrixMultiplication.swift:236-298
  rotateColumnsMultiStep,
  rotateColumnsAndSum,
  swapRowsAndAdd                  _HomomorphicEncryptionExtras/HeScheme.swift:21-60, 113-151
"""
import numpy as np

import pnns_reference as pnns
from pnns_reference import dividing_ceil, next_power_of_two


# ---- denseRow packing --------------------------------------------------------------------------------------------------------
def dense_row_slots(values, row_count, cols, degree):
    """denseRowPlaintexts up to context.encode(values:format: .simd), line by line: the SIMD slot values of every plaintext,
    [plaintext_count][N].  values: residues mod t, row-major [row_count][cols]."""
    values = [int(v) for v in np.asarray(values).reshape(-1)]
    simd_columns = degree // 2
    if cols > simd_columns:
        raise ValueError("invalidMatrixDimensions")
    pad_values = [0] * (next_power_of_two(cols) - cols)
    plaintexts, packed, index = [], [], 0
    for _ in range(row_count):
        packed += values[index:index + cols]
        index += cols
        packed += pad_values
        if len(packed) < simd_columns and len(packed) + cols > simd_columns:
            packed += [0] * (simd_columns - len(packed))
        if len(packed) + cols > degree:
            plaintexts.append(packed + [0] * (degree - len(packed)))  # encodeSimd pads with zeros
            packed = []
    if packed:
        col_offset = len(packed) % simd_columns
        packed += [0] * (0 if col_offset == 0 else next_power_of_two(col_offset) - col_offset)
        repeat = packed[:] if len(packed) <= simd_columns else packed[simd_columns:]
        while len(packed) < degree:
            packed += repeat
        assert len(packed) == degree
        plaintexts.append(packed)
    assert len(plaintexts) == pnns.plaintext_count(degree, row_count, cols, "denseRow")
    return np.array(plaintexts, dtype=np.uint64)


# ---- extractDenseRow ---------------------------------------------------------------------------------------------------------
def _slot_indices(row_index, ciphertext_index, ciphertext_count, cols, degree):
    """simdSlotIndices (:281-300); ciphertext_index is the extracted row's, also when asked about another row: the closure
    captures it."""
    padded = next_power_of_two(cols)
    simd_columns = degree // 2
    rows_per_ciphertext = (simd_columns // padded) * 2
    batch_start = (row_index % rows_per_ciphertext) * padded
    lower, upper = batch_start, batch_start + padded
    if lower <= simd_columns < upper:
        lower, upper = simd_columns, simd_columns + padded
    elif upper > simd_columns:
        padding = simd_columns % padded
        lower, upper = lower + padding, upper + padding
    if ciphertext_index == ciphertext_count - 1:
        upper = dividing_ceil(upper, simd_columns) * simd_columns
    return lower, upper


def mask_list(row_index, row_count, cols, degree):
    """(:301-338) line by line -> (mask as a list of N values, copiesInMask)."""
    padded = next_power_of_two(cols)
    rows_per_ciphertext = (degree // 2 // padded) * 2
    ciphertext_count = dividing_ceil(row_count, rows_per_ciphertext)
    ciphertext_index = row_index // rows_per_ciphertext

    def indices(index):
        return _slot_indices(index, ciphertext_index, ciphertext_count, cols, degree)

    lower, upper = indices(row_index)
    last = row_index + 1
    while last < row_count and indices(last)[1] == upper:
        last += 1
    first = row_index - 1 if row_index > 0 else 0
    while first > 0 and indices(first)[1] == upper:
        first -= 1
    rows_in_batch = last - first
    repeat_mask = [1] * padded + [0] * (padded * (rows_in_batch - 1))
    repeat_mask += [0] * (next_power_of_two(len(repeat_mask)) - len(repeat_mask))
    mask, copies = [0] * lower, 0
    while len(mask) < upper:
        mask += repeat_mask
        copies += 1
    mask = mask[:degree]
    return mask + [0] * (degree - len(mask)), copies


def mask_rule(row_index, row_count, cols, degree):
    """The same reduced to (lower, period, copies): slot i is 1 iff lower <= i < min(N, lower + copies period) and
    (i - lower) mod period < P."""
    padded = next_power_of_two(cols)
    rows_per_ciphertext = (degree // 2 // padded) * 2
    ciphertext_count = dividing_ceil(row_count, rows_per_ciphertext)
    ciphertext_index = row_index // rows_per_ciphertext

    def upper_of(index):
        return _slot_indices(index, ciphertext_index, ciphertext_count, cols, degree)[1]

    lower, upper = _slot_indices(row_index, ciphertext_index, ciphertext_count, cols, degree)
    last = row_index + 1
    while last < row_count and upper_of(last) == upper:
        last += 1
    first = row_index - 1 if row_index > 0 else 0
    while first > 0 and upper_of(first) == upper:
        first -= 1
    period = next_power_of_two(padded * (last - first))
    return lower, period, dividing_ceil(upper - lower, period)


def mask_from_rule(lower, period, copies, cols, degree):
    padded = next_power_of_two(cols)
    i = np.arange(degree)
    return ((i >= lower) & (i < min(degree, lower + copies * period)) & ((i - lower) % period < padded)).astype(np.uint64)


def rotate_count(copies, cols, degree):
    return degree // 2 // (copies * next_power_of_two(cols)) - 1


class Keys:
    """One client's evaluation key as the restatement uses it: galois(ct [2][L][N], element) -> ciphertext, from a dict
    element -> key words."""

    def __init__(self, oracle_bfv, keys_by_element):
        self.bfv, self.keys = oracle_bfv, keys_by_element

    def galois(self, ct, element):
        return self.bfv.apply_galois(ct, element, self.keys[element])[0]


def extract_dense_row(oracle_bfv, encoder, element_of, query, row_index, row_count, cols, keys):
    """query [K][2][L][N] Coeff -> the one-row ciphertext [2][L][N] Coeff.  element_of(step or "swap") -> Galois element."""
    degree = oracle_bfv.degree
    ring = oracle_bfv.ciphertext_context()
    padded = next_power_of_two(cols)
    rows_per_ciphertext = (degree // 2 // padded) * 2
    if row_count == 1:
        return query[0]
    mask, copies = mask_list(row_index, row_count, cols, degree)
    plaintext = oracle_bfv.plaintext_to_eval(encoder.encode(np.array(mask, dtype=np.uint64)))[0]
    ciphertext_eval = ring.forward_ntt(query[row_index // rows_per_ciphertext])
    ciphertext = ring.inverse_ntt(oracle_bfv.mul_plain(ciphertext_eval[None], plaintext[None], 2)[0])
    copy_right = ciphertext
    for _ in range(rotate_count(copies, cols, degree)):
        copy_right = keys.galois(copy_right, element_of(padded))
        ciphertext = ring.add(ciphertext, copy_right)
    return ring.add(ciphertext, keys.galois(ciphertext, element_of("swap")))


# ---- mulTranspose(matrix:) ---------------------------------------------------------------------------------------------------
def mul_transpose_matrix(oracle_bfv, encoder, element_of, matrix_eval, rows, cols, baby_step, query, row_count, pack_steps,
                         keys):
    """matrix_eval [P C][L][N] Eval, query [K][2][L][N] Coeff, pack_steps the ordered (step, count) plan of
    rotateColumnsMultiStep(by: rows) -> the result ciphertexts [M][2][L][N] Coeff."""
    degree = oracle_bfv.degree
    ring = oracle_bfv.ciphertext_context()
    inner_products = []
    for row_index in range(row_count):
        row = extract_dense_row(oracle_bfv, encoder, element_of, query, row_index, row_count, cols, keys)
        inner_products += pnns.mul_transpose_vector(oracle_bfv, matrix_eval, rows, cols, baby_step, row,
                                                    lambda ct: keys.galois(ct, element_of(-1)),
                                                    lambda ct: keys.galois(ct, element_of(-baby_step)))
    columns_per_simd_row = (degree // 2) // rows
    if columns_per_simd_row == 0:
        return np.stack(inner_products)

    def rotate_multi_step(ct):
        for step, count in pack_steps:
            for _ in range(count):
                ct = keys.galois(ct, element_of(step))
        return ct

    def rotate_and_sum(cts):
        cts = list(cts)
        accumulator = cts.pop()
        for ct in reversed(cts):
            accumulator = ring.add(rotate_multi_step(accumulator), ct)
        return accumulator

    per_ciphertext = 2 * columns_per_simd_row
    packed = []
    for start in range(0, len(inner_products), per_ciphertext):
        chunk = inner_products[start:start + per_ciphertext]
        packed_rows = [rotate_and_sum(chunk[i:i + columns_per_simd_row]) for i in range(0, len(chunk), columns_per_simd_row)]
        if len(chunk) > columns_per_simd_row:
            packed.append(ring.add(keys.galois(packed_rows[1], element_of("swap")), packed_rows[0]))
        else:
            packed.append(packed_rows[0])
    return np.stack(packed)


def result_ciphertext_count(degree, rows, row_count):
    columns_per_simd_row = (degree // 2) // rows
    if columns_per_simd_row > 0:
        return dividing_ceil(row_count, 2 * columns_per_simd_row)
    return row_count * dividing_ceil(rows, degree)


def needs(degree, rows, cols, row_count, baby_step=None):
    """Which key slots (0..3) and whether the pack plan ("pack") a shape reads."""
    baby, giant = pnns.baby_step_giant_step(cols, baby_step)
    columns_per_simd_row = (degree // 2) // rows
    out = set()
    if baby > 1:
        out.add(0)
    if giant > 1:
        out.add(1)
    if row_count > 1 or (columns_per_simd_row > 0 and row_count > columns_per_simd_row):
        out.add(2)
    if row_count > 1 and any(rotate_count(mask_rule(r, row_count, cols, degree)[2], cols, degree) > 0 for r in range(row_count)):
        out.add(3)
    if columns_per_simd_row >= 2 and row_count >= 2:
        out.add("pack")
    return out


# ---- denseColumn unpacking ---------------------------------------------------------------------------------------------------
def unpack_dense_column(slots, rows, cols, degree):
    """The inverse of denseColumnPlaintexts: decoded plaintexts [plaintext_count][N] -> values [rows][cols] (column `c` of the
    result matrix is the product with query row c)."""
    simd_columns = degree // 2
    values = np.zeros((rows, cols), dtype=np.uint64)
    plaintext, offset = 0, 0  # offset: len(packedValues)
    for col in range(cols):
        for row in range(rows):
            values[row, col] = slots[plaintext][offset]
            offset += 1
            if offset == degree:
                plaintext, offset = plaintext + 1, 0
        next_count = offset + rows
        if offset < simd_columns and simd_columns + 1 <= next_count <= degree:
            offset += (degree - offset) % simd_columns
        elif next_count > degree:
            plaintext, offset = plaintext + 1, 0
    return values
