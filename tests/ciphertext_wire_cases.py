"""The case table of tests/test_gpu_ciphertext_wire.py, kept apart from it so that tests/test_ciphertext_wire.py can hold the
kernel-form choice to its restatement over the same cases without a device.

Shapes: N in {8, 64, 128, 1024} (1024: eight 128-coefficient tiles per row, several workgroups per record), L in {1, 3}, poly_count in {2, 3}, count in
{1, 5} -- all 32 combinations, per word size.  Skips, strides, the record pointer's offset and the slab's offset rotate through
the combinations so that every value of each meets every degree:
  skips    "none" (NULL), "unequal" (a pair with unequal skips: a known-answer pair of tests/golden/skip_lsbs_kats.json where
           the moduli allow one -- UNEQUAL_SKIPS), "one-bit" (the second polynomial's narrowest row is left a single bit)
  strides  "exact", "plus1" (odd: a record's last chunk is shared with the next record's first), "mult16"
  offsets  the record pointer at +0 or +14 bytes of a 256-byte aligned buffer (+14: the payload, not the record, is 16-byte
           aligned); the slab at +0 or +1 word (off 16-byte alignment)."""
import collections
import itertools

Case = collections.namedtuple("Case", "word_bits degree bits poly_count count skip_kind stride_kind record_offset slab_offset")

# ceilLog2 of the moduli: 8-byte words 55 / 40 / 62 bits, 4-byte words 30, 27 and 2 bits
BITS = {64: {1: [55], 3: [55, 40, 62]}, 32: {1: [27], 3: [30, 27, 2]}}
# [22, 13] and [11, 3] are known answers of Bfv.skipLSBsForDecryption (n_8192_logq_3x55_logt_30, n_4096_logq_27_28_28_logt_13);
# next to a 2-bit modulus no skip above 1 is valid, so (32, 3) takes [1, 0], which is unequal and nobody's known answer
UNEQUAL_SKIPS = {(64, 1): [22, 13], (64, 3): [22, 13], (32, 1): [11, 3], (32, 3): [1, 0]}
DEGREES = (8, 64, 128, 1024)
SKIP_KINDS = ("none", "unequal", "one-bit")
RECORD_KINDS = ("packed", "random", "ones")  # what deserialize is fed: case i of ALL takes RECORD_KINDS[i % 3]
STRIDE_KINDS = ("exact", "plus1", "mult16")
BASE_ALIGNMENT = 256  # what the tests' device buffers are aligned to before the offsets below
RECORD_OFFSETS = (0, 14)
SLAB_OFFSETS = (0, 1)  # words


def skips_of(case):
    """the HOST skip array of a case (None: NULL), poly_count entries"""
    if case.skip_kind == "none":
        return None
    pair = list(UNEQUAL_SKIPS[(case.word_bits, len(case.bits))])
    if case.skip_kind == "one-bit":
        pair[1] = min(case.bits) - 1
    return (pair + [0])[:case.poly_count]


def stride_of(case, record_bytes):
    if case.stride_kind == "exact":
        return record_bytes
    if case.stride_kind == "plus1":
        return record_bytes + 1
    return (record_bytes + 16) // 16 * 16  # the next multiple of 16 above the byte count


def cases(word_bits):
    out = []
    shapes = itertools.product(DEGREES, (1, 3), (2, 3), (1, 5))
    for index, (degree, rows, poly_count, count) in enumerate(shapes):
        out.append(Case(word_bits, degree, tuple(BITS[word_bits][rows]), poly_count, count, SKIP_KINDS[index % 3],
                        STRIDE_KINDS[(index // 3 + index) % 3], RECORD_OFFSETS[(index // 2 + index // 8) % 2],
                        SLAB_OFFSETS[(index + index // 4) % 2]))
    return out


ALL = cases(64) + cases(32)


def case_id(case):
    return (f"u{case.word_bits}-n{case.degree}-l{len(case.bits)}-p{case.poly_count}-c{case.count}-{case.skip_kind}-"
            f"{case.stride_kind}-r{case.record_offset}-s{case.slab_offset}")


def moduli_of(bits, generate_primes, ntt_degree=1):
    """one modulus per entry with that ceilLog2: distinct primes, and 3 for the 2-bit one"""
    primes = iter(generate_primes([b for b in bits if b > 2], False, ntt_degree))
    moduli = [3 if b == 2 else next(primes) for b in bits]
    assert [(q - 1).bit_length() for q in moduli] == list(bits) and len(set(moduli)) == len(moduli)
    return moduli


# The polynomial-level entries on 4-byte slabs: degree, bits, skip, the byte buffer's offset, bytes a deserialized record is
# longer than the polynomial, and the form both directions take (serialize ignores the extra bytes: its records are tight)
Narrow = collections.namedtuple("Narrow", "degree bits skip bytes_offset extra serialize_form deserialize_form")
NARROW = [
    Narrow(8, (30, 27, 2), 0, 0, 0, "byte", "byte"),      # rows of 30, 27 and 2 bytes
    Narrow(64, (30, 27, 2), 1, 0, 0, "word", "word"),     # every row a multiple of 8 bytes
    Narrow(64, (30, 27, 2), 0, 1, 0, "byte", "byte"),     # ... but the buffer is not
    Narrow(128, (27,), 11, 0, 8, "word", "word"),
    Narrow(128, (27,), 11, 0, 1, "word", "byte"),         # the stride alone moves deserialize to the byte form
    Narrow(1024, (30, 27, 2), 1, 0, 16, "word", "word"),  # several trips under a capped grid
    Narrow(1024, (30, 27, 2), 0, 3, 5, "byte", "byte"),
]
