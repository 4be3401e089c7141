"""KeywordPirClient restated in Python integers (reference Sources/PrivateInformationRetrieval/KeywordPir/
KeywordPirProtocol.swift:279-392) over tests/keyword_pir_reference.py (keyword_hash, hash_indices, deserialize_bucket, find)
and tests/pir_client_reference.py: the plan, the per-query outcome of decrypt(response:at:using:) over bucket rows and the scan
of countEntriesInResponse.  The constants restate csrc/keyword_pir_client_plan.hpp; tests/test_keyword_pir_client_reference.py
holds the two to each other through a compiled host program."""
import keyword_pir_reference as kw
import pir_client_reference as client

NIL, FOUND, CORRUPT = 0, 1, 2
SLOT_HEADER_BYTES = 10
STAGED_ROW_LIMIT = 32 * 1024       # rows up to this many bytes are walked in LDS
STAGED_SMALL_ROW_LIMIT = 4 * 1024  # ... by the one-wave instantiation
STAGE_PADDING = 16


def value_capacity(entry_size):
    """the longest value a row holds: the count byte and one slot header in front of it, a UInt16 size"""
    return 0 if entry_size < 11 else min(entry_size - 11, kw.MAX_VALUE_SIZE)


def find_form(entry_size):
    return "staged" if entry_size <= STAGED_ROW_LIMIT else "direct"


def staged_lds_bytes(entry_size):
    if entry_size > STAGED_ROW_LIMIT:
        return 0
    return (STAGED_SMALL_ROW_LIMIT if entry_size <= STAGED_SMALL_ROW_LIMIT else STAGED_ROW_LIMIT) + STAGE_PADDING


def plan(degree, t, dimensions, entry_count, entry_size, hash_function_count):
    """The keys of heamd's keyword_pir_client_plan: the index-PIR plan without a size prefix and with h indices a query
    (KeywordPirProtocol.swift:221-228), and what the bucket search adds"""
    p = client.plan(degree, t, dimensions, entry_count, entry_size, False, hash_function_count)
    p.update(value_capacity=value_capacity(entry_size), find_form=find_form(entry_size),
             staged_lds_bytes=staged_lds_bytes(entry_size),
             reply_bytes=p["reply_ciphertext_count"] * p["bytes_per_plaintext"])
    return p


def hash_and_indices(keyword, bucket_count, hash_function_count):
    """generateQuery(at:using:) in front of the index-PIR client (:329-332) -> (hash, [h] indices)"""
    hash_ = kw.keyword_hash(keyword)
    return hash_, kw.hash_indices_of_hash(hash_, bucket_count, hash_function_count)


def walk(raw, begin=0):
    """HashBucket.init(deserialize:) of raw[begin:] as the header states it -> ([(hash, value offset, value size)], end) or None
    for corruptedData"""
    length = len(raw)
    if begin >= length:
        return None
    count, offset, slots = raw[begin], begin + 1, []
    for _ in range(count):
        if length < offset + SLOT_HEADER_BYTES:
            return None
        hash_ = int.from_bytes(raw[offset:offset + 8], "little")
        size = int.from_bytes(raw[offset + 8:offset + 10], "little")
        offset += SLOT_HEADER_BYTES
        if offset + size > length:
            return None
        slots.append((hash_, offset, size))
        offset += size
    return slots, offset


def find_in_buckets(rows, hash_):
    """decrypt(response:at:using:) lines 352-358 over a query's h rows -> (status, size, value): the buckets in order, a
    bucket deserialized before it is searched"""
    for raw in rows:
        raw = bytes(raw)
        walked = walk(raw)
        if walked is None:
            return CORRUPT, 0, b""
        for slot_hash, offset, size in walked[0]:
            if slot_hash == hash_:
                return FOUND, size, raw[offset:offset + size]
    return NIL, 0, b""


def padded_value(status, value, entry_size):
    """out_values[q]: the value, then zeros up to value_capacity"""
    return bytes(value) + bytes(value_capacity(entry_size) - len(value))


def count_reply_entries(data):
    """countEntriesInResponse's scan of one reply (:384-388): a zero byte is an empty bucket of length one"""
    data, offset, found = bytes(data), 0, 0
    while offset < len(data):
        walked = walk(data, offset)
        if walked is None:
            break
        found += len(walked[0])
        offset = walked[1]
    return found


def count_entries(replies):
    return sum(count_reply_entries(data) for data in replies)
