"""The keyword-PIR database build on the device against keyword_pir_reference (hashlib): the hash, index and shard kernels, the
bucket serialization at every alignment, and the table object end to end -- its buckets, the index-PIR databases of its
sub-tables word for word, and every keyword found again in the bytes read back.  Whole output buffers are compared, with guard
bytes on both sides."""
import json
import os

import numpy as np
import pytest

import heamd
import keyword_pir_cases as cases
import keyword_pir_reference as ref
import pir_database_reference as refdb
from heamd.binding import vp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(ROOT, "tests", "golden", "keyword_pir_kats.json")) as f:
        return json.load(f)


class Guarded:
    """`nbytes` of device memory `offset` bytes past a 64-byte boundary, pre-filled with 0xA5 like the guard bytes around them"""

    def __init__(self, nbytes, offset=0):
        import torch

        self.nbytes, self.first = nbytes, GUARD + offset
        self.buffer = torch.full((self.first + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buffer.data_ptr() % 64 == 0
        self.ptr = vp(self.buffer.data_ptr() + self.first)

    def read(self, dtype=np.uint8):
        import torch

        torch.cuda.synchronize()
        host = self.buffer.cpu().numpy()
        assert (host[:self.first] == FILL).all() and (host[self.first + self.nbytes:] == FILL).all(), "guard bytes were written"
        return host[self.first:self.first + self.nbytes].copy().view(dtype)


def device(array, offset=0):
    """a host array on the device, `offset` bytes past a 64-byte boundary -> (tensor that owns it, pointer)"""
    import torch

    raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    buffer = torch.empty((raw.size + offset + 1,), dtype=torch.uint8, device="cuda")
    buffer[offset:offset + raw.size] = torch.from_numpy(raw.copy())
    return buffer, vp(buffer.data_ptr() + offset)


def check(status):
    heamd.binding._check(status)


def offsets_of(items):
    out = np.zeros(len(items) + 1, dtype=np.uint64)
    np.cumsum([len(item) for item in items], out=out[1:])
    return out


# ---- HashKeyword.hash ---------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 1000]  # a block exactly full, padding into a second block, multiples, many


def device_hashes(keywords, blob_offset):
    lib = heamd.load_library()
    blob = np.frombuffer(b"".join(keywords), dtype=np.uint8)
    blob_mem, blob_ptr = device(blob, blob_offset)
    offsets_mem, offsets_ptr = device(offsets_of(keywords))
    out = Guarded(8 * len(keywords))
    check(lib.he_keyword_pir_hash_keywords_device(blob_ptr, offsets_ptr, len(keywords), out.ptr, None))
    return out.read(np.uint64)


@pytest.mark.parametrize("order", ["rising", "falling"])
def test_keyword_hashes(order):
    rng = np.random.default_rng(len(order))
    lengths = LENGTHS if order == "rising" else LENGTHS[::-1]
    # 257 keywords (a second workgroup), back to back from an odd address: most start at odd addresses
    keywords = [rng.integers(0, 256, size=lengths[i % len(lengths)], dtype=np.uint8).tobytes() for i in range(257)]
    want = np.array([ref.keyword_hash(k) for k in keywords], dtype=np.uint64)
    assert np.array_equal(device_hashes(keywords, 1), want)
    for single in (keywords[0], keywords[2], keywords[10 if order == "rising" else 0]):  # count 1
        assert device_hashes([single], 3)[0] == ref.keyword_hash(single)


def test_keyword_hash_of_the_reference_bucket(kats):
    slots = kats["raw_bucket"]["slots"]
    got = device_hashes([b"Hello", b"Goodbye"], 0)
    assert [int(h) for h in got] == [slots[0]["hash"], slots[2]["hash"]]


# ---- HashKeyword.hashIndices and ShardingFunction.shardIndex --------------------------------------------------------------------
def device_indices(hashes, bucket_count, h):
    lib = heamd.load_library()
    hashes_mem, hashes_ptr = device(np.asarray(hashes, dtype=np.uint64))
    out = Guarded(4 * h * len(hashes))
    check(lib.he_keyword_pir_hash_indices_device(hashes_ptr, len(hashes), bucket_count, h, out.ptr, None))
    return out.read(np.uint32).reshape(len(hashes), h)


@pytest.mark.parametrize("bucket_count", [1, 2, 8, 1001, 2048, 2**32 - 1])
def test_hash_indices(bucket_count):
    """Bucket count 1: every index is 0 and the retries are used up; 2: keyword 780 (4 bytes little-endian) collides through the
    tenth retry at h = 2 and the repeated index is kept."""
    keywords = [v.to_bytes(4, "little") for v in list(range(700, 960)) + [0, 1, 2**32 - 1]]  # 263: a second workgroup
    hashes = [ref.keyword_hash(k) for k in keywords]
    for h in (1, 2, 3, 5, 8):
        want = np.array([ref.hash_indices_of_hash(x, bucket_count, h) for x in hashes], dtype=np.uint32)
        got = device_indices(hashes, bucket_count, h)
        assert np.array_equal(got, want), h
        if bucket_count == 1:
            assert not got.any()
        if bucket_count == 2 and h == 2:
            row = got[keywords.index((780).to_bytes(4, "little"))]
            assert row[0] == row[1]
    assert np.array_equal(device_indices(hashes[:1], bucket_count, 3)[0], ref.hash_indices_of_hash(hashes[0], bucket_count, 3))


def test_hash_indices_and_shards_of_the_reference(kats):
    import torch

    for kat in kats["hash_indices"]:
        hashes = heamd.keyword_pir_hash_keywords(torch.tensor(kat["keyword"], dtype=torch.uint8, device="cuda"),
                                                 torch.tensor([0, len(kat["keyword"])], dtype=torch.int64, device="cuda"))
        got = heamd.keyword_pir_hash_indices(hashes, kat["bucket_count"], kat["hash_function_count"])
        assert got.cpu().numpy().view(np.uint32).tolist() == [kat["expected"]]
    keywords = [bytes(kat["keyword"]) for kat in kats["sharding"]]
    hashes_mem, hashes_ptr = device(np.array([ref.keyword_hash(k) for k in keywords], dtype=np.uint64))
    lib = heamd.load_library()
    for i, kat in enumerate(kats["sharding"]):
        out = Guarded(4 * len(keywords))
        check(lib.he_keyword_pir_shard_indices_device(hashes_ptr, len(keywords), kat["shard_count"], kat["other_shard_count"],
                                                      out.ptr, None))
        got = out.read(np.uint32)
        assert got[i] == kat["expected"], kat
        assert got.tolist() == [ref.shard_index(k, kat["shard_count"], kat["other_shard_count"]) for k in keywords]
    # more than one workgroup, through the binding
    many = np.array([ref.keyword_hash(bytes([k & 255, k >> 8])) for k in range(300)], dtype=np.uint64)
    got = heamd.keyword_pir_shard_indices(heamd.to_device(many), 1001, 2000).cpu().numpy().view(np.uint32)
    assert got.tolist() == [int(x) % 2000 % 1001 for x in many]


# ---- HashBucket.serialize -------------------------------------------------------------------------------------------------------
def random_values(rng, sizes):
    return [rng.integers(0, 256, size=size, dtype=np.uint8).tobytes() for size in sizes]


def bucket_sets():
    """name -> (entry size, buckets as lists of value sizes)"""
    rng = np.random.default_rng(7)
    small = []
    for b in range(300):  # entry size 51: every third bucket empty, the others filled with 0 / 1 / 7 / 8 / 9 byte values
        sizes, used = [], 1
        while b % 3 != 1:
            size = int(rng.choice([0, 1, 7, 8, 9]))
            if used + 10 + size > 51:
                break
            sizes.append(size)
            used += 10 + size
        small.append(sizes)
    return {
        "300 buckets of 51 bytes": (51, small),
        "255 empty values fill 2551 bytes": (2551, [[2000, 7], [0] * 255, [], [1, 8, 9, 0, 7, 1200], [2540], [], [9] * 100]),
        "a value of 65 535 bytes": (65552, [[65535], [], [0, 1, 7, 8, 9]]),
        "empty buckets of one byte": (1, [[]] * 5),
        "rows of 64 bytes": (64, [[0, 1, 7, 8], [53], [], [], [9, 9, 9], [43, 0], [0] * 6, [8], [7, 7]]),
        "one bucket": (51, [[5, 6, 8]]),
    }


BUCKET_SETS = bucket_sets()


def serialize_on_device(entry_size, buckets, offset, rng, mismatch=False):
    """buckets: lists of value sizes -> (rows read back [buckets][entry_size], what HashBucket.serialize gives, mismatch word)"""
    lib = heamd.load_library()
    placed = sum(len(b) for b in buckets)
    order = rng.permutation(placed + 3)  # the entries lie in another order than the slots, three of them in no bucket
    sizes = np.zeros(placed + 3, dtype=np.int64)
    slot_entries, bucket_offsets = [], [0]
    for bucket in buckets:
        for size in bucket:
            entry = int(order[len(slot_entries)])
            sizes[entry] = size
            slot_entries.append(entry)
        bucket_offsets.append(len(slot_entries))
    sizes[order[placed:]] = [4, 0, 11]
    values = random_values(rng, sizes)
    hashes = rng.integers(0, 2**64, size=len(values), dtype=np.uint64)
    want = [ref.serialize_bucket([(int(hashes[e]), values[e]) for e in slot_entries[bucket_offsets[b]:bucket_offsets[b + 1]]])
            if bucket_offsets[b + 1] - bucket_offsets[b] <= 255 else None for b in range(len(buckets))]
    keep = [device(hashes), device(np.frombuffer(b"".join(values), dtype=np.uint8), 1), device(offsets_of(values)),
            device(np.array(bucket_offsets, dtype=np.uint32)), device(np.array(slot_entries + [0], dtype=np.uint32))]
    flag = Guarded(4)
    if mismatch:
        flag.buffer[flag.first:flag.first + 4] = 0
    out = Guarded(len(buckets) * entry_size, offset)
    check(lib.he_keyword_pir_serialize_buckets_device(keep[0][1], keep[1][1], keep[2][1], keep[3][1], keep[4][1], placed,
                                                      len(buckets), entry_size, out.ptr, flag.ptr if mismatch else None, None))
    rows = out.read().reshape(len(buckets), entry_size)
    return rows, want, int(flag.read(np.uint32)[0]) if mismatch else None


def assert_rows(rows, want, entry_size):
    for b, raw in enumerate(want):
        assert len(raw) <= entry_size
        assert rows[b].tobytes() == raw + bytes(entry_size - len(raw)), b  # the record, then zeros: no 0xA5 is left


@pytest.mark.parametrize("offset", [0, 1, 3, 8])
@pytest.mark.parametrize("name", list(BUCKET_SETS))
def test_serialized_buckets(name, offset):
    entry_size, buckets = BUCKET_SETS[name]
    rows, want, _ = serialize_on_device(entry_size, buckets, offset, np.random.default_rng(offset))
    assert_rows(rows, want, entry_size)


def test_serialized_reference_bucket(kats):
    import torch

    raw = bytes(kats["raw_bucket"]["bytes"])
    slots = kats["raw_bucket"]["slots"]
    values = [bytes(slot["value"]) for slot in slots]
    got = heamd.keyword_pir_serialize_buckets(
        heamd.to_device(np.array([slot["hash"] for slot in slots], dtype=np.uint64)),
        torch.from_numpy(np.frombuffer(b"".join(values), dtype=np.uint8).copy()).cuda(), heamd.to_device(offsets_of(values)),
        torch.tensor([0, 3], dtype=torch.int32, device="cuda"), torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda"),
        len(raw))
    assert got.cpu().numpy().tobytes() == raw


def test_serialize_reports_what_a_row_cannot_hold():
    """A bucket longer than its row is cut at the row's end (bit 0); more than 255 slots is bit 1.  Nothing else is written."""
    rng = np.random.default_rng(3)
    rows, want, flag = serialize_on_device(20, [[5], [9, 9], []], 1, rng, mismatch=True)
    assert flag == 1
    assert rows[0].tobytes() == want[0] + bytes(4) and rows[1].tobytes() == want[1][:20] and not rows[2].any()
    rows, want, flag = serialize_on_device(2561, [[0] * 256, [1]], 0, rng, mismatch=True)
    assert flag == 2 and rows[1].tobytes() == want[1] + bytes(2561 - len(want[1]))
    rows, want, flag = serialize_on_device(51, [[5, 6, 8], []], 0, rng, mismatch=True)
    assert flag == 0
    assert_rows(rows, want, 51)


# ---- the table object end to end --------------------------------------------------------------------------------------------
OK_CASES = [c for c in cases.CASES if c.expect == "ok"]


def c_config(config):
    return heamd.CuckooTableConfig(config.hash_function_count, config.max_eviction_count, config.max_serialized_bucket_size,
                                   config.bucket_count, config.expansion_factor, config.target_load_factor,
                                   config.multiple_tables, config.slot_count)


@pytest.fixture(scope="module")
def contexts(oracle):
    t = oracle.generate_primes([17], True, 64)[0]
    q = oracle.generate_primes([40, 40, 40, 41], False, 64)
    q32 = [(1 << 27) - 40959, (1 << 28) - 65535, (1 << 28) - 73727]  # n_4096_logq_27_28_28
    return {64: (heamd.BfvContext(64, t, q), oracle.BfvContext(64, t, q)),
            32: (heamd.BfvContext32(4096, (1 << 16) + 1, q32), oracle.BfvContext(4096, (1 << 16) + 1, q32, word_bits=32))}


@pytest.mark.parametrize("case", OK_CASES, ids=[c.name for c in OK_CASES])
def test_table_end_to_end(oracle, contexts, case):
    import torch

    want = ref.Table(case.config, case.keywords, case.values, case.seed)
    table = heamd.KeywordPirTable(c_config(case.config), case.keywords, case.values, case.seed)
    assert (table.bucket_count, table.buckets_per_table, table.table_count) == \
        (want.bucket_count, want.buckets_per_table, case.config.table_count)
    assert (table.entry_count, table.duplicates_dropped, table.expansion_count) == (want.placed, want.duplicates, want.expansions)
    assert table.largest_bucket_size == want.largest_bucket_size()
    assert np.float32(table.load_factor) == want.load_factor()
    if case.name in cases.EXPANSION_CASES:
        assert table.expansion_count >= 1
    # maxEntrySize (KeywordPirProtocol.swift:205-218)
    entry_size = case.config.max_serialized_bucket_size if case.config.fixed_size else want.largest_bucket_size()
    padded = want.padded(entry_size)
    image = np.frombuffer(b"".join(padded), dtype=np.uint8).reshape(want.bucket_count, entry_size)
    out = Guarded(image.size, 3)
    check(heamd.load_library().he_keyword_pir_table_entries_device(table.h, vp(table.values.data_ptr()), entry_size, out.ptr,
                                                                   None))
    rows = out.read().reshape(image.shape)
    assert np.array_equal(rows, image)
    assert np.array_equal(table.entries(entry_size).cpu().numpy(), image)
    if want.largest_bucket_size() > 1:
        with pytest.raises(heamd.HeError) as err:
            table.entries(want.largest_bucket_size() - 1)
        assert err.value.name == "invalidArgument"

    # every keyword is found in exactly one of its candidate buckets, in the bytes read back; a stranger in none
    per_table, h = want.buckets_per_table, case.config.hash_function_count
    first_value = {}
    for keyword, value in zip(case.keywords, case.values):
        first_value.setdefault(keyword, value)
    for keyword in list(first_value) + [b"no such keyword"]:
        candidates = ref.hash_indices(keyword, per_table, h)
        buckets = {t * per_table + i if case.config.multiple_tables else i for t, i in enumerate(candidates)}
        found = [value for value in (ref.find(rows[b].tobytes(), keyword=keyword) for b in sorted(buckets)) if value is not None]
        assert found == ([first_value[keyword]] if keyword in first_value else []), keyword

    # the index-PIR database of every sub-table, on both word sizes
    dims = [4, -(-per_table // 4)]
    for bits, (ours, oracle_ctx) in contexts.items():
        to_host = heamd.to_host32 if bits == 32 else heamd.to_host
        database, present = table.process_database(ours, dims, entry_size)
        torch.cuda.synchronize()
        got_db, got_present = to_host(database), present.cpu().numpy()
        assert got_db.shape[0] == got_present.shape[0] == case.config.table_count
        for t in range(case.config.table_count):
            sub = image[t * per_table:(t + 1) * per_table]
            direct_db, direct_present = ours.pir_process_database(torch.from_numpy(sub.copy()).cuda(), dims, entry_size, False)
            torch.cuda.synchronize()
            assert np.array_equal(got_db[t], to_host(direct_db)) and np.array_equal(got_present[t], direct_present.cpu().numpy())
            want_db, want_present = refdb.process(oracle, oracle_ctx, [bytes(row) for row in sub], dims, entry_size, False)
            assert np.array_equal(got_present[t], want_present)
            assert np.array_equal(got_db[t].reshape(want_db.shape), want_db)
    with pytest.raises(heamd.HeError) as err:
        table.process_database(contexts[64][0], dims, want.largest_bucket_size() - 1)
    assert err.value.name == "invalidArgument"


@pytest.mark.parametrize("case", [c for c in cases.CASES if c.expect != "ok"], ids=lambda c: c.name)
def test_table_errors(case):
    with pytest.raises(heamd.HeError) as err:
        heamd.KeywordPirTable(c_config(case.config), case.keywords, case.values, case.seed)
    assert err.value.name == case.expect
