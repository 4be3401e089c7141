"""The cases tests/test_simple_pir_shard_reference.py and tests/test_gpu_simple_pir_shards.py share: databases of variable-length
values with an order of the shards per entry, drawn from a seed, and the worked example of the sharding section of
include/he_amd.h."""
import collections

import numpy as np

import simple_pir_shard_reference as R

Case = collections.namedtuple("Case", "name shard_count chunk_size count slab_residue seed")

SHARD_COUNTS = (1, 2, 3, 5, 64, 65, 256)
CHUNK_SIZES = (1, 7, 16, 33, 48)
TILE = R.MAP_TILE
COUNTS = (0, 1, TILE, TILE + 1, 3 * TILE + 37)  # nothing, one entry, one tile, one tile + 1, three tiles and a remainder


def grid():
    """every shard count with every chunk size; the entry counts rotate so that each meets every shard count and every chunk
    size.  The slab lies on a 16-byte boundary, and 8 bytes past one where the chunk size also allows the 8-byte form."""
    cases = []
    for i, shard_count in enumerate(SHARD_COUNTS):
        for j, chunk_size in enumerate(CHUNK_SIZES):
            count = COUNTS[(i + j) % len(COUNTS)]
            residues = (0, 8) if chunk_size % 8 == 0 and (i + j) % 2 == 0 else (0,)
            for residue in residues:
                cases.append(Case("S%d-C%d-n%d-at%d" % (shard_count, chunk_size, count, residue), shard_count, chunk_size, count,
                                  residue, 1000 * i + 10 * j + residue))
    return cases


GRID = grid()


def database(case):
    """-> (values: list of bytes, orders: list of lists).  The lengths start with 0, 1, C, C S and C S + 1 (one chunk more than
    a round of the order) and go on at random up to 300."""
    rng = np.random.default_rng(case.seed)
    S, C = case.shard_count, case.chunk_size
    fixed = [0, 1, C, C * S, C * S + 1]
    lengths = [fixed[e] if e < len(fixed) else int(rng.integers(0, 301)) for e in range(case.count)]
    if case.count == 1:
        lengths = [C * S + 1]
    values = [rng.integers(0, 256, size=length, dtype=np.uint8).tobytes() for length in lengths]
    orders = [[int(v) for v in rng.permutation(S)] for _ in range(case.count)]
    return values, orders


def flat(values):
    """-> (blob, offsets [count + 1])"""
    offsets = [0]
    for value in values:
        offsets.append(offsets[-1] + len(value))
    return b"".join(values), offsets


# the worked example: S = 2, C = 2
EXAMPLE_VALUES = [b"abcde", b"", b"fg"]
EXAMPLE_ORDERS = [[1, 0], [0, 1], [0, 1]]
EXAMPLE_CHUNKS = [[(1, 0), (0, 0), (1, 1)], [], [(0, 1)]]
EXAMPLE_SHARDS = [[b"cd", b"fg"], [b"ab", b"e\0"]]


def random_split(rng):
    """one case of the closed-form check: S 1..6, C 1..5, lengths that include 0, C, C S and C S + 1"""
    S, C = int(rng.integers(1, 7)), int(rng.integers(1, 6))
    count = int(rng.integers(0, 9))
    special = [0, C, C * S, C * S + 1]
    lengths = [special[int(rng.integers(0, 4))] if rng.integers(0, 2) else int(rng.integers(0, 4 * C * S + 2)) for _ in range(count)]
    values = [rng.integers(0, 256, size=length, dtype=np.uint8).tobytes() for length in lengths]
    orders = [[int(v) for v in rng.permutation(S)] for _ in range(count)]
    return S, C, values, orders
