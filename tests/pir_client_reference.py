"""The MulPIR client restated in Python integers (reference Sources/PrivateInformationRetrieval/IndexPir/MulPir.swift:86-109,
150-155, 179-289, PirUtil.swift:361-404, IndexPirProtocol.swift:61-73, 109-119).  The reply's byte string comes from
oracle.coefficients_to_bytes (CoefficientPacking.swift:155-216 as written, unmasked coefficients included); the ciphertext words
from encrypt_reference.py and decrypt_reference.py.  The closed form of the byte string that the device kernel computes is
restated here in numpy (reply_bytes_closed_form) and held to the oracle by tests/test_pir_client_reference.py."""
import numpy as np

import decrypt_reference
import encrypt_reference
from pir_database_reference import encoding_width


def ceil_log2(value):
    return 0 if value <= 1 else (value - 1).bit_length()


def plan(degree, t, dimensions, entry_count, entry_size, encoding, indices_count=1):
    """The keys of heamd's pir_client_plan, and the names of the issue: bits, enc, per, R, S, P, C."""
    bits = t.bit_length() - 1
    bpp = degree * bits // 8
    width = encoding_width(entry_size) if encoding else 0
    enc = width + entry_size
    total = sum(dimensions) * indices_count
    return {"bits": bits, "bytes_per_plaintext": bpp, "entry_size_encoding_width": width, "encoded": enc,
            "entries_per_plaintext": bpp // enc if bpp >= enc else 1, "reply_ciphertext_count": -(-enc // bpp),
            "expanded_query_count": total, "query_ciphertext_count": -(-total // degree), "dimension_sum": sum(dimensions),
            "dimension_product": int(np.prod([int(d) for d in dimensions], dtype=object)), "entry_count": entry_count,
            "entry_size": entry_size, "degree": degree, "dimensions": list(dimensions), "indices_count": indices_count}


def coordinates(p, index):
    """MulPirClient.computeCoordinates(at:) (MulPir.swift:181-193)"""
    assert 0 <= index < p["entry_count"]
    plaintext = index // p["entries_per_plaintext"]
    product = p["dimension_product"]
    out = []
    for size in p["dimensions"]:
        product //= size
        coordinate = plaintext // product
        plaintext -= coordinate * product
        out.append(coordinate)
    return out


def nonzero_positions(p, indices):
    """generateQuery's nonZeroPositions (MulPir.swift:204-212); an index not below entry_count selects nothing (the device's
    rule: the reference throws PirError.invalidIndex)"""
    out, accumulated = [], 0
    for index in indices:
        valid = 0 <= index < p["entry_count"]
        here = coordinates(p, index) if valid else [None] * len(p["dimensions"])
        for size, coordinate in zip(p["dimensions"], here):
            if valid:
                out.append(accumulated + coordinate)
            accumulated += size
    return out


def selection_value(count, t):
    """compressInputsForOneCiphertext's value (PirUtil.swift:367-371)"""
    return pow(pow(2, ceil_log2(count), t), -1, t)


def query_plaintexts(p, t, indices):
    """PirUtil.compressBinaryInputs up to encryption (PirUtil.swift:381-402): [C][N] uint64"""
    degree, total = p["degree"], p["expanded_query_count"]
    ones = nonzero_positions(p, indices)
    out = np.zeros((p["query_ciphertext_count"], degree), dtype=np.uint64)
    processed, c = 0, 0
    while processed < total:
        count = min(total - processed, degree)
        for x in ones:
            if processed <= x < processed + count:
                out[c, x - processed] = selection_value(count, t)
        processed += count
        c += 1
    return out


def generate_query(poly_ctx, t, p, indices, s_eval, a_seeds, error_seeds, stream):
    """MulPirClient.generateQuery(at:using:) on the caller's seeds -> [C][2][L][N] Coeff"""
    plaintexts = query_plaintexts(p, t, indices)
    return np.stack([encrypt_reference.encrypt(poly_ctx, t, plaintexts[c], s_eval, a_seeds[c], error_seeds[c], stream)
                     for c in range(len(plaintexts))])


def evaluation_key_elements(expanded_query_count, degree, key_compression):
    """MulPir.evaluationKeyConfig (MulPir.swift:86-109); key_compression "none", "hybrid" or "max".  An empty range (one input,
    no compression) is a trap in the reference and an empty list here."""
    log_degree = degree.bit_length() - 1
    smallest = log_degree - ceil_log2(min(expanded_query_count, degree)) + 1
    largest = log_degree if key_compression == "none" else max(smallest, -(-(log_degree + 1) // 2))
    elements = [(1 << level) + 1 for level in range(smallest, largest + 1)]
    if key_compression == "hybrid":
        extra = (1 << max(largest, (log_degree + largest + 1) // 2)) + 1
        if extra not in elements:
            elements.append(extra)
    return elements


def reply_bytes(oracle, plaintexts, bits):
    """The byte string of one reply: coefficientsToBytes of each of its plaintexts, back to back (MulPir.swift:256-262)"""
    return b"".join(bytes(oracle.coefficients_to_bytes(np.ascontiguousarray(row, dtype=np.uint64), bits)) for row in plaintexts)


def reply_bytes_closed_form(coefficients, bits):
    """What the device kernel computes for one plaintext, in numpy: stream bit s is bit bits - 1 - (s mod bits) of coefficient
    s / bits; bit `bits` of coefficient k >= 1 is OR-ed into stream bit k bits - 1 unless k bits is a multiple of 8."""
    coefficients = np.asarray(coefficients, dtype=np.uint64)
    count = len(coefficients) * bits // 8 * 8
    s = np.arange(count, dtype=np.int64)
    k, within = s // bits, s % bits
    stream = (coefficients[k] >> (bits - 1 - within).astype(np.uint64)) & np.uint64(1)
    fields = np.arange(1, len(coefficients), dtype=np.int64)
    fields = fields[(fields * bits % 8 != 0) & (fields * bits - 1 < count)]
    stream[fields * bits - 1] |= (coefficients[fields] >> np.uint64(bits)) & np.uint64(1)
    return np.packbits(stream.astype(np.uint8)).tobytes()


def entry_of_reply(p, data, index):
    """MulPirClient.decrypt(response:at:using:)'s last step (MulPir.swift:264-273) -> (entry bytes padded with zeros to E, size):
    a size above E counts as E"""
    width, enc, size = p["entry_size_encoding_width"], p["encoded"], p["entry_size"]
    position = index % p["entries_per_plaintext"]
    record = data[position * enc:(position + 1) * enc]
    if width:
        size = min(int.from_bytes(record[:width], "little"), p["entry_size"])
    body = record[width:width + size]
    return body + bytes(p["entry_size"] - len(body)), size


def decrypt_response(oracle, poly_ctx, t, p, response, indices, s_eval):
    """response [I][R][2][L'][N] Coeff -> [(entry, size)] per index; indices None: decryptFull's byte strings"""
    out = []
    for i, reply in enumerate(response):
        plaintexts = [decrypt_reference.decrypt(decrypt_reference.dot_product(poly_ctx, ct, s_eval), poly_ctx.moduli, t)
                      for ct in reply]
        data = reply_bytes(oracle, plaintexts, p["bits"])
        out.append(data if indices is None else entry_of_reply(p, data, indices[i]))
    return out
