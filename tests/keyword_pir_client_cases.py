"""The hand-built bucket table of the keyword-PIR client, shared by tests/test_keyword_pir_client_reference.py (CPU) and
tests/test_gpu_keyword_pir_client.py: each case is (h, E, rows, target hash) -> (status, size, value), the rows written by
keyword_pir_reference.serialize_bucket or by hand where a bucket has to be one the library never writes.  The count cases are
byte strings -> the slots countEntriesInResponse finds.  Nothing here is random."""
import collections
import struct

import keyword_pir_client_reference as client
import keyword_pir_reference as kw

NIL, FOUND, CORRUPT = client.NIL, client.FOUND, client.CORRUPT
T = 0x8877665544332211                     # the target of most cases: every byte differs
A, B, C, D = 0x0101010101010101, 0xFFFFFFFFFFFFFFFF, 0x00000000000000FF, 0xFF00000000000000
BYTE0, BYTE7 = T ^ 0x01, T ^ (0x80 << 56)  # differ from T in byte 0 / byte 7 only
OFFSETS = (0, 1, 3, 15)                    # of the buckets pointer inside a 16-byte line: every head / tail path of the staging

Case = collections.namedtuple("Case", "name h entry_size rows target status size value")


def row(slots, entry_size, count=None):
    """serialize_bucket padded with zeros to entry_size; count: a count byte that differs from the slots written"""
    raw = bytearray(kw.serialize_bucket(slots))
    if count is not None:
        raw[0] = count
    assert len(raw) <= entry_size, (len(raw), entry_size)
    return bytes(raw) + bytes(entry_size - len(raw))


def slot(hash_, size, body):
    """a slot whose size field need not be its body's length"""
    return struct.pack("<QH", hash_, size) + body


def pattern(length, seed):
    return bytes((seed + 7 * i) % 251 for i in range(length))


def _cases():
    out = []

    def add(name, h, entry_size, rows, target, status, value=b""):
        assert len(rows) == h and all(len(r) == entry_size for r in rows), name
        out.append(Case(name, h, entry_size, [bytes(r) for r in rows], target, status, len(value), bytes(value)))

    other = lambda e, seed=0: row([(A + seed, b"other"), (B - seed, b"")], e)  # noqa: E731
    # where the match lies
    add("slot 0", 1, 64, [row([(T, b"abc"), (A, b"defg")], 64)], T, FOUND, b"abc")
    add("last slot of bucket 0", 2, 64, [row([(A, b"x"), (B, b"yy"), (T, b"last")], 64), other(64)], T, FOUND, b"last")
    add("bucket h - 1", 3, 77, [other(77), other(77, 1), row([(C, b"q"), (T, pattern(40, 3))], 77)], T, FOUND, pattern(40, 3))
    add("no match", 2, 64, [other(64), other(64, 1)], T, NIL)
    add("h = 8, bucket 7", 8, 45, [other(45, k) for k in range(7)] + [row([(T, pattern(34, 1))], 45)], T, FOUND, pattern(34, 1))
    add("h = 8, no match", 8, 45, [other(45, k) for k in range(8)], T, NIL)
    # a found value of no bytes next to a nil
    add("empty value found", 1, 33, [row([(A, b"a"), (T, b"")], 33)], T, FOUND, b"")
    add("empty value, other hash", 1, 33, [row([(A, b"a"), (T, b"")], 33)], D, NIL)
    # the first slot and the first bucket win
    add("same hash in two slots", 1, 64, [row([(T, b"first"), (T, b"second")], 64)], T, FOUND, b"first")
    add("same hash in two buckets", 2, 64, [row([(A, b"a"), (T, b"one")], 64), row([(T, b"two")], 64)], T, FOUND, b"one")
    # hashes one byte away, in slots at odd offsets 13 and 25 (slot 0 holds two bytes)
    near = [(A, b"xx"), (BYTE0, b"lo"), (BYTE7, b"hi")]
    add("byte 0 and byte 7 differ, then the hash", 1, 63, [row(near + [(T, b"yes")], 63)], T, FOUND, b"yes")
    add("byte 0 and byte 7 differ", 1, 63, [row(near, 63)], T, NIL)
    add("byte 7 differs, asked for", 1, 63, [row(near, 63)], BYTE7, FOUND, b"hi")
    # padding is no slot
    add("hash 0 against zeros", 1, 32, [bytes(32)], 0, NIL)
    add("hash 0 against padding behind a slot", 2, 40, [row([(A, b"a")], 40), bytes(40)], 0, NIL)
    # 255 slots of empty values
    full = [(1000 + k, b"") for k in range(255)]
    add("255 slots, the last", 1, 2551, [row(full, 2551)], 1254, FOUND, b"")
    add("255 slots, none", 1, 2551, [row(full, 2551)], 1255, NIL)
    # corrupt buckets
    three = [(T, b""), (A, b""), (B, b"")]
    add("three slots end at E", 1, 31, [row(three, 31)], B, FOUND, b"")
    add("a count byte one above the slots that fit", 1, 31, [row(three, 31, count=4)], T, CORRUPT)
    add("a value one byte past E", 1, 32, [bytes([1]) + slot(T, 22, pattern(21, 5))], T, CORRUPT)
    add("the same bucket ends at E", 1, 32, [bytes([1]) + slot(T, 21, pattern(21, 5))], T, FOUND, pattern(21, 5))
    broken = bytes([2]) + slot(A, 3, b"abc") + slot(B, 60000, b"") + bytes(64 - 24)
    add("a corrupt bucket behind the match", 2, 64, [row([(T, b"safe")], 64), broken], T, FOUND, b"safe")
    add("a corrupt bucket in front of the match", 2, 64, [broken, row([(T, b"late")], 64)], T, CORRUPT)
    add("a corrupt bucket and no match", 2, 64, [other(64), broken], T, CORRUPT)
    third = bytes([3]) + slot(T, 2, b"ok") + slot(A, 0, b"") + slot(B, 41, b"") + bytes(64 - 33)
    add("slot 0 matches, slot 2 is corrupt", 1, 64, [third], T, CORRUPT)
    add("the same with slot 2 ending at E", 1, 64, [bytes([3]) + slot(T, 2, b"ok") + slot(A, 0, b"") + slot(B, 31, bytes(31))], T,
        FOUND, b"ok")
    # the smallest rows
    add("E = 1, count 0", 1, 1, [b"\x00"], T, NIL)
    add("E = 1, count 1", 1, 1, [b"\x01"], T, CORRUPT)
    add("E = 10, count 1", 2, 10, [bytes(10), b"\x01" + bytes(9)], 0, CORRUPT)
    add("E = 11, an empty value", 1, 11, [row([(T, b"")], 11)], T, FOUND, b"")
    add("E = 12, one byte", 1, 12, [row([(T, b"\xa5")], 12)], T, FOUND, b"\xa5")
    # the ragged ends of the value copy: 15, 16, 17 and 33 bytes
    for length in (15, 16, 17, 33):
        add("a value of %d bytes" % length, 2, 61, [other(61), row([(A, b"z"), (T, pattern(length, length))], 61)], T, FOUND,
            pattern(length, length))
    # long rows: both sides of the one-wave instantiation, of the LDS budget, and the longest value there is
    for entry_size in (client.STAGED_SMALL_ROW_LIMIT, client.STAGED_SMALL_ROW_LIMIT + 1, client.STAGED_ROW_LIMIT,
                       client.STAGED_ROW_LIMIT + 1):
        filler = pattern(entry_size - 11 - 10 - 37, 9)
        add("E = %d, the value at its end" % entry_size, 2, entry_size,
            [row([(A, pattern(100, 2))], entry_size), row([(B, filler), (T, pattern(37, 4))], entry_size)], T, FOUND, pattern(37, 4))
    add("a value of 65535 bytes", 1, 65546, [row([(T, pattern(65535, 11))], 65546)], T, FOUND, pattern(65535, 11))
    return out


CASES = _cases()
assert len({case.name for case in CASES}) == len(CASES)

# which form the plan names on each side of its budget
FORMS = {client.STAGED_ROW_LIMIT: "staged", client.STAGED_ROW_LIMIT + 1: "direct", 65546: "direct", 1: "staged"}

# three queries over h = 2 with three outcomes and distinct rows: a transposed (query, bucket) index fails
BATCH_H, BATCH_E = 2, 77
BATCH = [
    ([row([(A, b"q0 b0")], 77), row([(T, b"found in bucket 1")], 77)], T, FOUND, b"found in bucket 1"),
    ([row([(T, b"another hash")], 77), row([(B, b"q1 b1")], 77)], C, NIL, b""),
    ([row([(C, b"q2 b0")], 77), bytes([1]) + slot(C, 70, bytes(66))], C, FOUND, b"q2 b0"),
    ([bytes([9]) + bytes(76), row([(D, b"too late")], 77)], D, CORRUPT, b""),
]

# ---- countEntriesInResponse: bytes -> slots found
_b2, _b1, _b3 = kw.serialize_bucket([(A, b"ab"), (B, b"")]), kw.serialize_bucket([(C, pattern(30, 1))]), \
    kw.serialize_bucket([(A, b"x"), (B, b"yy"), (T, b"zzz")])
COUNT_CASES = [
    ("all zero", bytes(40), 0),
    ("nothing", b"", 0),
    ("one zero byte", b"\x00", 0),
    ("back to back, the last ends at len", _b2 + _b1 + _b3, 6),
    ("a trailing partial bucket", _b2 + _b1 + _b3[:-1], 3),
    ("a trailing partial slot header", _b2 + _b3[:15], 2),
    ("count 255 over too few bytes behind two buckets", _b2 + _b1 + b"\xff" + pattern(100, 3), 3),
    ("zero runs of 13, 9 and 7 bytes", bytes(13) + _b2 + bytes(9) + _b3 + bytes(7), 5),
    ("a bucket inside the first eight bytes", bytes(3) + _b1 + bytes(70) + _b2 + bytes(1), 3),
    ("256 zero bytes and a bucket", bytes(256) + _b3, 3),
]
# replies of one length for a batched call: [queries][replies a query][length], zero padded (padding counts nothing)
COUNT_BATCH_LENGTH = 96
COUNT_BATCH = [[_b2 + _b1, bytes(5) + _b3, b""], [_b3 + bytes(8) + _b3, _b1 + b"\xff" + pattern(20, 1), bytes(17) + _b2]]
COUNT_BATCH_EXPECTED = [3 + 3 + 0, 6 + 1 + 2]

# ---- keywords for the query test: bucket counts 70 (dims [4, 3]) and 28 (dims [5]); the first two candidates of the named
# keywords collide (index_from_hash at counters 0 and 1), so hashIndices' retry runs past the candidate every keyword repeats
KEYWORDS = [b"", b"a", b"key-5", b"key-19", bytes(range(64)), b"k" * 119]
COLLIDING = {70: (b"key-5", [37, 27, 54]), 28: (b"key-19", [1, 26, 24])}
