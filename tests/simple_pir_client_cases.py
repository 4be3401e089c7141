"""The shapes and inputs the SimplePIR client tests share (tests/test_simple_pir_client_reference.py on the host,
tests/test_gpu_simple_pir_client.py on the device).  SHAPES is copied from tests/test_gpu_simple_pir.py, not imported: that
module builds a device server per shape."""
import zlib

import numpy as np

import simple_pir_reference as R

# (entry_count, entry_size_in_bytes, plaintext_bits, ciphertext_bits, lattice_dimension, word_bits)
SHAPES = {
    "ref-small-u32": (600, 20, 7, 28, 1024, 32),
    "ref-small-u64": (600, 20, 14, 42, 1024, 64),
    "ref-large-u32": (20, 600, 7, 28, 1024, 32),   # chunks_per_entry 5, 686 scalars padded to 690
    "ref-large-u64": (20, 600, 14, 42, 1024, 64),  # chunks_per_entry 4, 343 scalars padded to 344
    "columns-equal-n-u32": (1024, 2, 7, 28, 1024, 32),
    "columns-equal-n-u64": (256, 3, 14, 42, 256, 64),
    "three-polys-u32": (700, 3, 7, 28, 256, 32),
    "three-polys-u64": (700, 3, 14, 42, 256, 64),
    "one-entry-u32": (1, 50, 7, 28, 64, 32),
    "one-entry-u64": (1, 50, 14, 42, 64, 64),
    "bytes2-u32": (90, 9, 14, 28, 64, 32),
    "bytes4-u32": (90, 9, 20, 29, 64, 32),
    "bytes1-u64": (90, 9, 7, 42, 64, 64),
    "bytes4-u64": (90, 9, 20, 42, 64, 64),
    "bytes8-u64": (90, 9, 40, 55, 64, 64),
}
# what the client tests run on: the cut and three polynomials, several chunks with a padded one, several entries per column at
# N = 1024, one entry, 55-bit words, database_columns = N
CLIENT_SHAPES = ["three-polys-u32", "three-polys-u64", "ref-large-u32", "ref-large-u64", "ref-small-u32", "ref-small-u64",
                 "one-entry-u32", "one-entry-u64", "bytes8-u64", "columns-equal-n-u32", "columns-equal-n-u64"]
# the reference's two parameter pairs, the only ones a client can decrypt with (tests/test_gpu_simple_pir.py END_TO_END)
END_TO_END = sorted(name for name, s in SHAPES.items() if s[2:4] in ((7, 28), (14, 42)))
STD_DEVS = ("stdDev32", "stdDev64")


def params_of(oracle, name):
    entry_count, entry_size, pbits, cbits, n, word_bits = SHAPES[name]
    return R.shape(oracle, pbits, cbits, n, entry_count, entry_size, word_bits)


def rng_of(name, salt=""):
    return np.random.default_rng(zlib.crc32((name + salt).encode()))


def inputs_of(name, params, batch, salt=""):
    """-> (entries, database seed, secret_seeds [batch][chunks][32], error_seeds [batch][32]) of a shape, the same wherever asked"""
    rng = rng_of(name, salt)
    entries = rng.integers(0, 256, size=(params["entry_count"], params["entry_size_in_bytes"]), dtype=np.uint8)
    seed = bytes(rng.integers(0, 256, size=32, dtype=np.uint8))
    secret_seeds = rng.integers(0, 256, size=(batch, params["chunks_per_entry"], 32), dtype=np.uint8)
    error_seeds = rng.integers(0, 256, size=(batch, 32), dtype=np.uint8)
    return entries, seed, secret_seeds, error_seeds


def end_to_end_indices(name, params):
    count = params["entry_count"]
    return sorted({0, count - 1, int(rng_of(name, "index").integers(0, count))})
