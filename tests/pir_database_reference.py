"""MulPirServer.process(database:with:using:) (reference Sources/PrivateInformationRetrieval/IndexPir/MulPir.swift:431-556)
restated for the tests from two pinned oracle primitives only: oracle.bytes_to_coefficients (CoefficientPacking.swift:59-136)
and oracle.BfvContext.plaintext_to_eval (Plaintext.swift:149-170).  Entries are lists of bytes-like objects of their own
sizes; the parameter is (dimensions, entry_size_in_bytes, encoding_entry_size)."""
import numpy as np


class ProcessError(ValueError):
    pass


def encoding_width(entry_size):
    """IndexPirConfig.entrySizeEncodingWidth (IndexPirProtocol.swift:106-120)."""
    for width, top in ((1, 0xFF), (2, 0xFFFF), (4, 0xFFFFFFFF)):
        if entry_size <= top:
            return width
    return 8


def prefix(size, width):
    """IndexPirConfig.encodeEntrySize: the entry's byte count, `width` little-endian bytes (IndexPirProtocol.swift:123-150)."""
    return int(size).to_bytes(width, "little") if width else b""


def varying_entries(rng, count, entry_size, full=False):
    """Entries of varying sizes (the first full, every fifth all zero) and the padded device image with garbage past each
    entry's size -> (entries, padded uint8 [count][entry_size], sizes uint64 [count])."""
    sizes = np.full(count, entry_size) if full else rng.integers(0, entry_size + 1, size=count)
    if count:
        sizes[0] = entry_size
    entries = [rng.integers(0, 256, size=int(s), dtype=np.uint8).tobytes() for s in sizes]
    for k in range(3, count, 5):
        entries[k] = bytes(int(sizes[k]))
    padded = rng.integers(0, 256, size=(count, entry_size), dtype=np.uint8)
    for row, entry in enumerate(entries):
        padded[row, :len(entry)] = np.frombuffer(entry, dtype=np.uint8)
    return entries, padded, sizes.astype(np.uint64)


def shape(degree, t, dimensions, entry_count, entry_size, encoding):
    """The plan: the keys of heamd's pir_database_shape.  ProcessError where the reorder would give the wrong size."""
    if not dimensions or 0 in dimensions:
        raise ProcessError("empty or zero dimensions")
    bits = t.bit_length() - 1
    bpp = degree * bits // 8
    width = encoding_width(entry_size) if encoding else 0
    encoded = width + entry_size
    if encoded == 0:
        raise ProcessError("zero-byte entries without a prefix")
    per_chunk = int(np.prod(dimensions))
    chunks = -(-encoded // bpp)
    per_plaintext = bpp // encoded if chunks == 1 else 0
    if chunks > 1 and entry_count > per_chunk:
        raise ProcessError("split mode: more entries than plaintexts per chunk")
    if chunks == 1 and -(-entry_count // per_plaintext) > per_chunk:
        raise ProcessError("pack mode: more plaintexts than plaintexts per chunk")
    return {"chunk_count": chunks, "plaintexts_per_chunk": per_chunk, "bytes_per_plaintext": bpp,
            "entries_per_plaintext": per_plaintext, "entry_size_encoding_width": width}


def slot_of(j, dimensions):
    """Where plaintext j lands inside its chunk (MulPir.swift:486-495, 545-553)."""
    d0 = dimensions[0]
    rest = int(np.prod(dimensions)) // d0
    return (j % rest) * d0 + j // rest


def plaintext_bytes(entries, dimensions, degree, t, entry_size, encoding):
    """[chunk][slot] -> the plaintext's byte slice (b"" where there is none)."""
    if any(len(e) > entry_size for e in entries):
        raise ProcessError("entry longer than entry_size_in_bytes")
    plan = shape(degree, t, dimensions, len(entries), entry_size, encoding)
    chunks, per_chunk, bpp = plan["chunk_count"], plan["plaintexts_per_chunk"], plan["bytes_per_plaintext"]
    width = plan["entry_size_encoding_width"]
    out = [[b""] * per_chunk for _ in range(chunks)]
    if chunks > 1:  # processSplitLargeEntries (MulPir.swift:453-500)
        for r, entry in enumerate(entries):
            record = prefix(len(entry), width) + bytes(entry)
            for k in range(chunks):
                out[k][slot_of(r, dimensions)] = record[k * bpp:(k + 1) * bpp]
    else:  # processPackEntries (MulPir.swift:502-556)
        encoded = width + entry_size
        flat = b"".join(prefix(len(e), width) + bytes(e) + bytes(entry_size - len(e)) for e in entries)
        block = plan["entries_per_plaintext"] * encoded
        for j in range(-(-len(entries) // plan["entries_per_plaintext"])):
            out[0][slot_of(j, dimensions)] = flat[j * block:(j + 1) * block]
    return out


def unpack(oracle, data, bits, degree):
    """bytesToCoefficients(bytes:, bitsPerCoeff:, decode: false), zero padded to N coefficients."""
    coefficients = np.zeros(degree, dtype=np.uint64)
    if len(data):
        values = oracle.bytes_to_coefficients(np.frombuffer(bytes(data), dtype=np.uint8), bits, False)
        coefficients[:len(values)] = values
    return coefficients


def process(oracle, ref, entries, dimensions, entry_size, encoding):
    """-> (database [chunks][prod(dimensions)][L][N] Eval, present [chunks][prod(dimensions)] uint8)."""
    slices = plaintext_bytes(entries, dimensions, ref.degree, ref.t, entry_size, encoding)
    bits = ref.t.bit_length() - 1
    chunks, per_chunk = len(slices), len(slices[0])
    coefficients = np.zeros((chunks, per_chunk, ref.degree), dtype=np.uint64)
    for k in range(chunks):
        for s in range(per_chunk):
            coefficients[k, s] = unpack(oracle, slices[k][s], bits, ref.degree)
    present = coefficients.any(axis=2).astype(np.uint8)  # nil: no nonzero coefficient
    database = np.zeros((chunks, per_chunk, ref.L, ref.degree), dtype=np.uint64)
    live = present.astype(bool)
    if live.any():
        database[live] = ref.plaintext_to_eval(np.ascontiguousarray(coefficients[live]))
    return database, present
