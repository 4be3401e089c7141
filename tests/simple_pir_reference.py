"""SimplePIR (reference Sources/PrivateInformationRetrieval/SimplePir/) restated for the tests in numpy from reading it:
computingParams and process (SimplePir+Database.swift:209-290) with the matrix A MATERIALISED (:186-206) from the
NistAes128Ctr stream (oracle.CtrDrbg, 4096-byte refills) and hint = database x A mod p in exact integers; computeResponse
(SimplePir+Server.swift:31-38) as a wrapping matmul and a mask; and the minimum of the client (SimplePir+Client.swift,
SimplePir+Precompute.swift:191-300).  It takes the slow, obvious route on purpose -- no NTT, no Galois map -- so that it
shares no shortcut with the code under test."""
import math

import numpy as np


class ShapeError(ValueError):
    pass


def swift_rounded(x):
    """Double.rounded(): to nearest, halves away from zero (x >= 0 here)."""
    return math.floor(x + 0.5)


def element_bytes(plaintext_bits):
    return 1 if plaintext_bits <= 8 else 2 if plaintext_bits <= 16 else 4 if plaintext_bits <= 32 else 8


def shape(oracle, plaintext_bits, ciphertext_bits, lattice_dimension, entry_count, entry_size_in_bytes, word_bits=64):
    """computingParams (SimplePir+Database.swift:209-243), process's padded column size (:262-268), aPolyCount (:171-175),
    SimplePirContext.init's modulus (SimplePirContext.swift:76-87).  Keys as heamd.simple_pir_shape."""
    if word_bits not in (32, 64) or plaintext_bits < 1 or ciphertext_bits <= plaintext_bits:
        raise ShapeError("bits")
    if ciphertext_bits > (29 if word_bits == 32 else 60):
        raise ShapeError("ciphertext_bits does not fit the word")
    if lattice_dimension < 2 or lattice_dimension & (lattice_dimension - 1):
        raise ShapeError("lattice_dimension")
    if entry_count < 1 or entry_size_in_bytes < 1:
        raise ShapeError("empty database")
    scalars = -(-8 * entry_size_in_bytes // plaintext_bits)  # bytesToCoefficientsCoeffCount(decode: false)
    database_size = entry_count * scalars
    ideal_column_size = int(swift_rounded(math.sqrt(float(database_size))))
    if ideal_column_size > scalars:
        ideal_column_size = scalars
    entries_per_column = max(int(swift_rounded(float(ideal_column_size) / float(scalars))), 1)
    # Int(Double(entrySizeInScalar) / Double(idealColumnSize).rounded()): the divisor is rounded, the quotient truncated
    chunks_per_entry = max(int(float(scalars) / float(swift_rounded(float(ideal_column_size)))), 1)
    if entries_per_column != 1 and chunks_per_entry != 1:
        raise ShapeError("precondition(entriesPerColumn == 1 || chunksPerEntry == 1)")
    if entries_per_column == 1:
        columns = entry_count * chunks_per_entry
    else:
        columns = max(-(-entry_count // entries_per_column), 1)
    padded = scalars if chunks_per_entry == 1 else -(-scalars // chunks_per_entry) * chunks_per_entry
    return {
        "entry_size_in_scalar": scalars, "entries_per_column": entries_per_column, "chunks_per_entry": chunks_per_entry,
        "database_columns": columns, "column_size": padded * entries_per_column // chunks_per_entry,
        "a_poly_count": -(-columns // lattice_dimension),
        "modulus": oracle.generate_primes([ciphertext_bits + 1], True, lattice_dimension)[0],
        "element_bytes": element_bytes(plaintext_bits), "plaintext_bits": plaintext_bits, "ciphertext_bits": ciphertext_bits,
        "lattice_dimension": lattice_dimension, "entry_size_in_bytes": entry_size_in_bytes, "entry_count": entry_count,
    }


def padded_entry_size(params):
    c = params["chunks_per_entry"]
    return params["entry_size_in_scalar"] if c == 1 else -(-params["entry_size_in_scalar"] // c) * c


def chunk_size(params):
    return -(-params["entry_size_in_scalar"] // params["chunks_per_entry"])


def make_database(entry_count, entry_size):
    """DatabaseShape.makeDatabase (_TestUtilities/PirUtilities/SimplePirTests.swift:40-48): bytes 0, 1, 2, ... wrapping."""
    return (np.arange(entry_count * entry_size, dtype=np.uint64) & 0xFF).astype(np.uint8).reshape(entry_count, entry_size)


def process_database(oracle, entries, params):
    """The transposed processedDatabase [column_size][database_columns] (SimplePir+Database.swift:262-275), one uint64 each."""
    padded = padded_entry_size(params)
    flat = np.zeros(params["database_columns"] * params["column_size"], dtype=np.uint64)
    for e, entry in enumerate(entries):
        coefficients = oracle.bytes_to_coefficients(np.ascontiguousarray(entry, dtype=np.uint8), params["plaintext_bits"], False)
        assert len(coefficients) == params["entry_size_in_scalar"]
        flat[e * padded:e * padded + len(coefficients)] = coefficients
    return np.ascontiguousarray(flat.reshape(params["database_columns"], params["column_size"]).T)


def a_polynomials(oracle, params, seed):
    """generateAPolynomials (:178-181): PolyRq.random from ONE NistAes128Ctr(seed), 16 little-endian stream bytes per
    coefficient (PolyRq+Randomize.swift:58-72), the stream drawn in 4096-byte refills."""
    n, p = params["lattice_dimension"], params["modulus"]
    count = params["a_poly_count"] * n
    drbg = oracle.CtrDrbg(bytes(seed))
    stream = b"".join(drbg.generate(4096) for _ in range(-(-count * 16 // 4096)))
    values = [int.from_bytes(stream[16 * i:16 * i + 16], "little") % p for i in range(count)]
    return np.array(values, dtype=np.uint64).reshape(params["a_poly_count"], n)


def negacyclic_matrix(a, p):
    """PolyRq.negacyclicMatrix() (PolyRq.swift:425-431): row i is a * x^i in Z_p[x] / (x^N + 1)."""
    n = len(a)
    a = np.asarray(a, dtype=np.uint64)
    negated = (np.uint64(p) - a) % np.uint64(p)
    rows = np.zeros((n, n), dtype=np.uint64)
    for i in range(n):
        rows[i, i:] = a[:n - i]
        rows[i, :i] = negated[n - i:]
    return rows


def materialize_a(params, polys):
    """materializeAMatrix (:186-206): the transposed negacyclic matrices stacked, cut to database_columns rows."""
    blocks = [negacyclic_matrix(a, params["modulus"]).T for a in polys]
    return np.ascontiguousarray(np.concatenate(blocks, axis=0)[:params["database_columns"]])


def matmul_mod(lhs, rhs, p):
    """lhs [m][k] x rhs [k][n] mod p in exact integers: 16-bit limbs through float64 products (each below 2^32, a sum of k
    of them below 2^53), recombined in Python integers."""
    lhs, rhs = np.asarray(lhs, dtype=np.uint64), np.asarray(rhs, dtype=np.uint64)
    assert lhs.shape[1] == rhs.shape[0] and lhs.shape[1] < (1 << 21)
    def limbs(x):
        out, shift = [], 0
        top = int(x.max()) if x.size else 0
        while shift == 0 or (top >> shift):
            out.append(((x >> np.uint64(shift)) & np.uint64(0xFFFF)).astype(np.float64))
            shift += 16
        return out
    total = np.zeros((lhs.shape[0], rhs.shape[1]), dtype=object)
    for i, a in enumerate(limbs(lhs)):
        for j, b in enumerate(limbs(rhs)):
            part = (a @ b).astype(np.uint64) % np.uint64(p)
            total = total + part.astype(object) * (pow(2, 16 * (i + j), p))
    return (total % p).astype(np.uint64)


def hint(params, database, a_matrix, rows=None):
    """processedDatabase.multiply(matrixA, modulus:) (:279-281); `rows`: only those rows of the hint."""
    source = database if rows is None else database[np.asarray(rows)]
    return matmul_mod(source, a_matrix, params["modulus"])


def compute_response(params, database, requests, word_bits=64):
    """computeResponse (SimplePir+Server.swift:31-38): [query_count][column_size], wrapping products, then the mask."""
    dtype = np.uint64 if word_bits == 64 else np.uint32
    mask = dtype((1 << params["ciphertext_bits"]) - 1)
    with np.errstate(over="ignore"):
        return (np.asarray(requests).astype(dtype) @ np.asarray(database).astype(dtype).T) & mask


# ---- the minimum of the client ------------------------------------------------------------------------------------------
def ternary_secrets(params, rng):
    """generateSecretPolys (SimplePir+Client.swift:21-27): chunks_per_entry polynomials with coefficients in {-1, 0, 1}
    (returned centred, int64)."""
    return rng.integers(-1, 2, size=(params["chunks_per_entry"], params["lattice_dimension"]), dtype=np.int64)


def negacyclic_product(a, s, p):
    """a * s in Z_p[x] / (x^N + 1), schoolbook in Python integers."""
    n = len(a)
    out = [0] * n
    for i in range(n):
        si = int(s[i])
        if si == 0:
            continue
        for j in range(n):
            k = i + j
            if k < n:
                out[k] += si * int(a[j])
            else:
                out[k - n] -= si * int(a[j])
    return [v % p for v in out]


def noiseless_sample_polynomial(params, polys, secrets):
    """noiselessSample (SimplePir+Client.swift:29-50): per secret, the products a_k * s concatenated, cut to
    database_columns."""
    p = params["modulus"]
    rows = []
    for s in secrets:
        row = []
        for a in polys:
            row.extend(negacyclic_product(a, s, p))
        rows.append(row[:params["database_columns"]])
    return np.array(rows, dtype=np.uint64)


def secret_times_matrix(params, secrets, matrix):
    """secretMatrix.multiply(transposing: matrix, modulus: p): [chunks][rows of matrix]; the secrets are centred, so the sums
    stay in int64 (N * p < 2^63)."""
    p = params["modulus"]
    assert params["lattice_dimension"] * p < (1 << 62)
    return ((np.asarray(secrets, dtype=np.int64) @ np.asarray(matrix).astype(np.int64).T) % np.int64(p)).astype(np.uint64)


def mod_switch(params, matrix):
    """Array2d.divideAndRound(initialMod: p, newMod: 2^ciphertext_bits) (Array2d.swift:489-515)."""
    p, c = params["modulus"], params["ciphertext_bits"]
    flat = [(((int(v) << c) + (p >> 1)) // p) & ((1 << c) - 1) for v in np.asarray(matrix).ravel()]
    return np.array(flat, dtype=np.uint64).reshape(np.asarray(matrix).shape)


class Client:
    """PrecomputedQueries.WithoutIndices.init + add(index:) + integrate + decrypt for one set of secrets."""

    def __init__(self, oracle, params, hint_matrix, a_matrix, rng):
        self.oracle, self.params = oracle, params
        c = params["ciphertext_bits"]
        self.mask = (1 << c) - 1
        self.delta = 1 << (c - params["plaintext_bits"])
        secrets = ternary_secrets(params, rng)
        sample = mod_switch(params, secret_times_matrix(params, secrets, a_matrix))  # noiselessSample == secret x A
        # error of the centred binomial kind, variance 10.5 (standard deviation 3.24: ErrorStdDev.stdDev32)
        error = rng.binomial(42, 0.5, size=sample.shape).astype(np.int64) - 21
        self.queries = ((sample.astype(np.int64) + error) & self.mask).astype(np.uint64)
        self.results_without_response = secret_times_matrix(params, secrets, hint_matrix)

    def query(self, index):
        """add(index:) (SimplePir+Precompute.swift:232-248)."""
        queries = self.queries.copy()
        for q in range(self.params["chunks_per_entry"]):
            column = (q + index * self.params["chunks_per_entry"]) // self.params["entries_per_column"]
            queries[q, column] = (int(queries[q, column]) + self.delta) & self.mask
        return queries

    def _extract(self, data, index):
        """extractEntries (SimplePir+Client.swift:86-96)."""
        params, size = self.params, chunk_size(self.params)
        flat, out = np.asarray(data).ravel(), []
        for q in range(params["chunks_per_entry"]):
            entry = q + index * params["chunks_per_entry"]
            start = q * params["column_size"] + (entry % params["entries_per_column"]) * size
            out.extend(int(v) for v in flat[start:start + size])
        return out

    def decrypt(self, responses, index):
        """integrate (SimplePir+Precompute.swift:286-297) and decrypt (SimplePir+Client.swift:110-119)."""
        params = self.params
        shift = params["ciphertext_bits"] - params["plaintext_bits"]
        ours, theirs = self._extract(self.results_without_response, index), self._extract(responses, index)
        values = [(((t - o + (self.delta >> 1)) & self.mask) >> shift) for t, o in zip(theirs, ours)]
        data = self.oracle.coefficients_to_bytes(values, params["plaintext_bits"])
        return bytes(data[:params["entry_size_in_bytes"]])
