"""The SimplePIR client (reference Sources/PrivateInformationRetrieval/SimplePir/SimplePir+Client.swift:19-121,
SimplePir+Precompute.swift:116-311; HomomorphicEncryption/Array2d.swift:382-429, 489-514) restated in Python integers from
reading the Swift, for batches of independent precomputed queries.  It builds on simple_pir_reference.py (shape, the seeded
polynomials, the schoolbook product), encrypt_reference.py (ternary_values) and wire_format_reference.py (the DRBG), and shares no
shortcut with the device code: no NTT, no reciprocal, no 2-bit codes, no fold.

`stream(seed, count)` returns the first `count` bytes of NistAes128Ctr(seed:); python_stream is the pure-Python DRBG of
wire_format_reference.py behind BufferedRng's 4096-byte refills, and encrypt_reference.oracle_stream the oracle's (the same
bytes, faster)."""
import math

import numpy as np

import encrypt_reference as E
import simple_pir_reference as R
import wire_format_reference as WF

STD_DEVS = {"stdDev32": 3.2, "stdDev64": 6.4}  # ErrorStdDev


def python_stream(seed, count):
    drbg = WF.CtrDrbg(bytes(seed))
    return b"".join(bytes(drbg.generate(E.CHUNK)) for _ in range(-(-count // E.CHUNK)))[:count]


# ---- the plan (csrc/simple_pir_client_plan.hpp restated) --------------------------------------------------------------------------
SECRET_ROWS_PER_PASS, HINT_TILE_ROWS, CODE_SLAB_COLUMNS, STAGING_WORDS = 16, 64, 1024, 1 << 24
CHAIN_RECORD_BYTES, DEVICE_MODULUS_BYTES = 192, 144


def _round16(value):
    return (value + 15) // 16 * 16


def code_words_per_row(n):
    return max(n // 16, 1)


def plan(params, std_dev, batch, word_bits=64, forced_row_block=0):
    """Keys as heamd.simple_pir_client_plan."""
    n, chunks, columns = params["lattice_dimension"], params["chunks_per_entry"], params["database_columns"]
    word_bytes, rows, row_words = word_bits // 8, batch * chunks, params["a_poly_count"] * n
    stream_bytes = stream_bytes_per_coefficient(std_dev)
    chunk = R.chunk_size(params)
    block = max(STAGING_WORDS // row_words, 1)
    if forced_row_block:
        block = min(block, forced_row_block)
    if rows:
        block = min(block, rows)
    error_chunks = -(-chunks * columns * stream_bytes // E.CHUNK)
    encrypt_zero_bytes = _round16(batch * error_chunks * CHAIN_RECORD_BYTES) + _round16(block * n * 8) + _round16(block * row_words * 8)
    codes = _round16(rows * 4 * code_words_per_row(n))
    secrets = _round16(rows * -(-12 * n // E.CHUNK) * CHAIN_RECORD_BYTES) + _round16(rows * n * word_bytes)
    return {
        "chunk_size": chunk, "query_words": chunks * columns, "result_words": chunks * params["column_size"],
        "error_stream_bytes": stream_bytes, "secret_rows_per_pass": SECRET_ROWS_PER_PASS,
        "fold_terms": ((1 << 64) - 1) // params["modulus"], "row_block": block,
        "hint_product_lds_bytes": SECRET_ROWS_PER_PASS * (CODE_SLAB_COLUMNS // 16) * 4 + SECRET_ROWS_PER_PASS * HINT_TILE_ROWS * 8,
        "a_polynomials_workspace_bytes": (_round16(params["a_poly_count"] * DEVICE_MODULUS_BYTES)
                                          + _round16(-(-row_words // 256) * CHAIN_RECORD_BYTES)
                                          + (_round16(row_words * 8) if word_bits == 32 else 0)),
        "encrypt_zero_workspace_bytes": encrypt_zero_bytes, "secret_times_hint_workspace_bytes": codes,
        "precompute_workspace_bytes": secrets + encrypt_zero_bytes + codes,
        "decrypt_responses_workspace_bytes": _round16(batch * chunks * chunk * word_bytes),
    }


# ---- Array2d.randomCenteredBinomialDistribution (Array2d.swift:382-429) -------------------------------------------------------
def binomial_layout(std_dev):
    """-> (k, UInt64s per trial, mask of the last word of each half)"""
    variance = STD_DEVS[std_dev] * STD_DEVS[std_dev]
    k = math.ceil(2 * variance)
    words = 2 * -(-k // 64)
    mask = (1 << (k % 64)) - 1 if k % 64 else (1 << 64) - 1
    return k, words, mask


def stream_bytes_per_coefficient(std_dev):
    return 8 * binomial_layout(std_dev)[1]


def centered_binomial(stream_bytes, count, std_dev, modulus):
    """`count` columns of a 1 x count array over [modulus]: pos.subtractMod(neg, modulus:) of the bit counts of the two
    halves of the trial's UInt64s, each rng.next() eight little-endian stream bytes."""
    _, words, mask = binomial_layout(std_dev)
    half = words // 2
    out = []
    for column in range(count):
        trial = [int.from_bytes(stream_bytes[8 * (column * words + w):8 * (column * words + w) + 8], "little")
                 for w in range(words)]
        trial[half - 1] &= mask
        trial[words - 1] &= mask
        positive = sum(bin(t).count("1") for t in trial[:half])
        negative = sum(bin(t).count("1") for t in trial[half:])
        out.append((positive - negative) % modulus)
    return out


# ---- divideAndRound (Array2d.swift:489-514) --------------------------------------------------------------------------------------
def divide_and_round(x, p, c):
    return (((int(x) << c) + (p >> 1)) // p) % (1 << c)


# ---- noiselessSample, encryptZero (SimplePir+Client.swift:21-82) ------------------------------------------------------------------
def secret_polynomials(params, secret_seeds, stream):
    """generateSecretPolys: one randomizeTernary per seed -> centred int64 [len(seeds)][N]"""
    n = params["lattice_dimension"]
    return np.array([[v - 1 for v in E.ternary_values(stream(seed, 12 * n), n)] for seed in secret_seeds], dtype=np.int64)


def secret_words(params, secrets):
    """centred secrets as the Coeff words the device reads: 0, 1, p - 1"""
    return (np.asarray(secrets, dtype=np.int64) % np.int64(params["modulus"])).astype(np.uint64)


def negacyclic_product(a, s, p):
    """a * s in Z_p[x] / (x^N + 1) for a centred ternary s: the schoolbook sum of simple_pir_reference.negacyclic_product, a row
    of it at a time -- the words of `a` in two 31-bit halves so that N signed terms stay in int64, recombined in Python integers"""
    n = len(a)
    a = np.asarray(a, dtype=np.uint64)
    low, high = (a & np.uint64((1 << 31) - 1)).astype(np.int64), (a >> np.uint64(31)).astype(np.int64)
    sums = [np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)]
    for i in range(n):
        si = int(s[i])
        if si == 0:
            continue
        for part, total in zip((low, high), sums):
            total[i:] += si * part[:n - i]
            total[:i] -= si * part[n - i:]
    return [(int(lo) + (int(hi) << 31)) % p for lo, hi in zip(*sums)]


def noiseless_sample(params, polys, secrets):
    """noiselessSample (:29-50): per secret, the products a_k * s concatenated, cut to database_columns"""
    p = params["modulus"]
    rows = []
    for s in secrets:
        row = []
        for a in polys:
            row.extend(negacyclic_product(a, s, p))
        rows.append(row[:params["database_columns"]])
    return rows


def encrypt_zero(params, polys, secrets, error_seed, std_dev, stream, sample=None):
    """encryptZero (:59-82) for one query: secrets centred [chunks][N]; the error is ONE generator over database_columns x
    chunks coefficients, reshaped to [chunks][database_columns] -> uint64 [chunks][database_columns]"""
    p, c = params["modulus"], params["ciphertext_bits"]
    chunks, columns = params["chunks_per_entry"], params["database_columns"]
    mask = (1 << c) - 1
    sample = noiseless_sample(params, polys, secrets) if sample is None else sample
    count = columns * chunks
    error = centered_binomial(stream(error_seed, count * stream_bytes_per_coefficient(std_dev)), count, std_dev, 1 << c)
    return np.array([[(divide_and_round(sample[q][j], p, c) + (error[q * columns + j] & mask)) & mask for j in range(columns)]
                     for q in range(chunks)], dtype=np.uint64)


# ---- secretMatrix.multiply(transposing: hint, modulus: p) (SimplePir+Precompute.swift:122-188) ------------------------------------
def secret_times_matrix(secrets, matrix, p):
    """[rows of secrets][rows of matrix] in Python integers: secrets centred or as words mod p"""
    lhs = np.asarray(secrets).astype(object) % p
    rhs = np.asarray(matrix).astype(object)
    return (lhs.dot(rhs.T) % p).astype(np.uint64)


def precompute(params, polys, hint, secret_seeds, error_seed, std_dev, stream):
    """PrecomputedQueries.WithoutIndices.init (:199-227) for one query: secret_seeds [chunks][32] ->
    (queries [chunks][database_columns], results_without_response [chunks][column_size], secrets centred)"""
    secrets = secret_polynomials(params, secret_seeds, stream)
    queries = encrypt_zero(params, polys, secrets, error_seed, std_dev, stream)
    return queries, secret_times_matrix(secrets, hint, params["modulus"]), secrets


# ---- add(index:), extractEntries, integrate, decrypt (:241-311, SimplePir+Client.swift:85-121) ------------------------------------
def add(params, queries, index):
    queries = np.array(queries, dtype=np.uint64)
    c = params["ciphertext_bits"]
    delta, mask = 1 << (c - params["plaintext_bits"]), (1 << c) - 1
    for q in range(params["chunks_per_entry"]):
        column = (q + index * params["chunks_per_entry"]) // params["entries_per_column"]
        queries[q, column] = (int(queries[q, column]) + delta) & mask
    return queries


def extract_entries(params, data, index):
    size, flat, out = R.chunk_size(params), np.asarray(data).ravel(), []
    for q in range(params["chunks_per_entry"]):
        entry = q + index * params["chunks_per_entry"]
        start = q * params["column_size"] + (entry % params["entries_per_column"]) * size
        out.extend(int(v) for v in flat[start:start + size])
    return out


def integrate(params, responses, results, index, word_bits=64):
    c = params["ciphertext_bits"]
    delta, mask, word = 1 << (c - params["plaintext_bits"]), (1 << c) - 1, (1 << word_bits) - 1
    ours, theirs = extract_entries(params, results, index), extract_entries(params, responses, index)
    return [((((t - o) & word) + (delta >> 1)) & word & mask) >> (c - params["plaintext_bits"]) for t, o in zip(theirs, ours)]


def coefficients_to_bytes(values, bits):
    """CoefficientPacking.coefficientsToBytes (CoefficientPacking.swift:155-216) for values below 2^bits: the fields MSB first as
    one big-endian integer, zero-padded to a whole byte"""
    whole = 0
    for v in values:
        assert 0 <= v < (1 << bits)
        whole = (whole << bits) | v
    total = len(values) * bits
    pad = -total % 8
    return (whole << pad).to_bytes((total + pad) // 8, "big")


def decrypt(params, responses, results, index, word_bits=64):
    """SimplePirClient.decrypt (SimplePir+Client.swift:112-121)"""
    values = integrate(params, responses, results, index, word_bits)
    return coefficients_to_bytes(values, params["plaintext_bits"])[:params["entry_size_in_bytes"]]
