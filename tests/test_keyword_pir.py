"""The keyword-PIR database build without a device: the restatement (keyword_pir_reference) against the reference's known
answers, he_keyword_pir_cuckoo_place against the restatement table for table over keyword_pir_cases, the invariants of every
resulting table, configuration and argument errors, and the ABI (header copy, exports, binding)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import heamd
import keyword_pir_cases as cases
import keyword_pir_reference as ref
from heamd.binding import STATUS_NAMES, U64P, c_size, c_u32, vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS_EXPANSION = "cuckooTableNeedsExpansion"
ENTRIES = (
    "he_keyword_pir_hash_keywords_device", "he_keyword_pir_hash_indices_device", "he_keyword_pir_shard_indices_device",
    "he_keyword_pir_config_validate", "he_keyword_pir_bucket_count", "he_keyword_pir_cuckoo_place",
    "he_keyword_pir_serialize_buckets_device", "he_keyword_pir_table_create_device", "he_keyword_pir_table_destroy",
    "he_keyword_pir_table_bucket_count", "he_keyword_pir_table_buckets_per_table", "he_keyword_pir_table_table_count",
    "he_keyword_pir_table_largest_bucket_size", "he_keyword_pir_table_entry_count",
    "he_keyword_pir_table_duplicates_dropped", "he_keyword_pir_table_expansion_count", "he_keyword_pir_table_load_factor",
    "he_keyword_pir_table_entries_device", "he_keyword_pir_process_database_device",
)


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(ROOT, "tests", "golden", "keyword_pir_kats.json")) as f:
        return json.load(f)


def c_config(config):
    return heamd.CuckooTableConfig(config.hash_function_count, config.max_eviction_count, config.max_serialized_bucket_size,
                                   config.bucket_count, config.expansion_factor, config.target_load_factor,
                                   config.multiple_tables, config.slot_count)


def status_of(code):
    return STATUS_NAMES[code]


# ---- the restatement against the reference's known answers ------------------------------------------------------------------
def test_restatement_reproduces_the_known_answers(kats):
    for kat in kats["hash_indices"]:
        assert ref.hash_indices(kat["keyword"], kat["bucket_count"], kat["hash_function_count"]) == kat["expected"]
    for kat in kats["sharding"]:
        assert ref.shard_index(kat["keyword"], kat["shard_count"], kat["other_shard_count"]) == kat["expected"], kat
    raw = bytes(kats["raw_bucket"]["bytes"])
    slots = [(slot["hash"], bytes(slot["value"])) for slot in kats["raw_bucket"]["slots"]]
    assert ref.deserialize_bucket(raw) == slots and ref.serialize_bucket(slots) == raw
    assert ref.serialized_size([len(v) for _, v in slots]) == len(raw)
    for found in kats["raw_bucket"]["finds"]:
        assert ref.find(raw, keyword=found["keyword"]) == bytes(found["value"])
    assert ref.find(raw, keyword=b"not there") is None
    assert ref.find(raw + bytes(13), keyword=b"Hello") == b"World"  # padding behind the last slot is ignored


def test_a_repeated_index_is_kept_after_the_tenth_retry():
    """The keyword the GPU test of bucket count 2 relies on: all eleven counters give one index."""
    keyword = (780).to_bytes(4, "little")
    hash_ = ref.keyword_hash(keyword)
    assert len({ref.index_from_hash(hash_, 2, counter) for counter in range(ref.MAX_RETRIES + 1)}) == 1
    first, second = ref.hash_indices(keyword, 2, 2)
    assert first == second
    assert ref.hash_indices(keyword, 1, 3) == [0, 0, 0]


# ---- placement ------------------------------------------------------------------------------------------------------------
def build_with_library(case):
    """The table object's loop over he_keyword_pir_cuckoo_place with the restatement's hashes and indices -> (buckets,
    duplicates, bucket count, expansions), or the error's name"""
    config = c_config(case.config)
    hashes = [ref.keyword_hash(k) for k in case.keywords]
    sizes = [len(v) for v in case.values]
    try:
        bucket_count = heamd.keyword_pir_bucket_count(config, sizes)
        expansions = 0
        while True:
            per_table = bucket_count // case.config.table_count
            indices = [ref.hash_indices_of_hash(h, per_table, case.config.hash_function_count) for h in hashes]
            got = heamd.keyword_pir_cuckoo_place(config, hashes, indices, sizes, bucket_count, case.seed)
            if got["status"] == "ok":
                break
            assert got["status"] == NEEDS_EXPANSION and got["next_bucket_count"] > bucket_count
            bucket_count = got["next_bucket_count"]
            expansions += 1
    except heamd.HeError as err:
        return err.name
    offsets = got["bucket_offsets"]
    assert offsets[0] == 0 and offsets[-1] == got["placed"] == len(got["slot_entries"])
    buckets = [[int(e) for e in got["slot_entries"][offsets[b]:offsets[b + 1]]] for b in range(bucket_count)]
    return buckets, got["duplicates_dropped"], bucket_count, expansions


def build_with_restatement(case):
    try:
        table = ref.Table(case.config, case.keywords, case.values, case.seed)
    except ref.PirError as err:
        return err.name
    return table


@pytest.mark.parametrize("case", cases.CASES, ids=[c.name for c in cases.CASES])
def test_placement_matches_the_restatement(case):
    want = build_with_restatement(case)
    got = build_with_library(case)
    if case.expect != "ok":
        assert want == case.expect and got == case.expect
        return
    assert not isinstance(want, str), want
    assert not isinstance(got, str), got
    buckets, duplicates, bucket_count, expansions = got
    assert bucket_count == want.bucket_count and expansions == want.expansions and duplicates == want.duplicates
    assert buckets == want.buckets
    if case.name in cases.EXPANSION_CASES:
        assert expansions >= 1
    assert duplicates == cases.DUPLICATES_DROPPED.get(case.name, 0)
    # the invariants
    config, hashes, sizes = case.config, want.hashes, [len(v) for v in case.values]
    per_table = bucket_count // config.table_count
    assert bucket_count % config.table_count == 0
    stored = [e for bucket in buckets for e in bucket]
    assert len(stored) == len(set(stored)) == len({hashes[e] for e in stored}) == len(case.keywords) - duplicates
    first_of_hash = {}
    for e, h in enumerate(hashes):
        first_of_hash.setdefault(h, e)
    assert sorted(stored) == sorted(first_of_hash.values())  # every keyword is there, in its first occurrence
    for b, bucket in enumerate(buckets):
        assert len(bucket) <= config.slot_count
        assert ref.serialized_size([sizes[e] for e in bucket]) <= config.max_serialized_bucket_size
        for e in bucket:
            candidates = ref.hash_indices_of_hash(hashes[e], per_table, config.hash_function_count)
            if config.multiple_tables:  # in the sub-table of the hash function that chose the bucket
                assert candidates[b // per_table] == b % per_table
            else:
                assert b in candidates


def test_the_large_newcomer_is_kept_where_nothing_can_be_swapped():
    """Where no resident value can be swapped out the reference expands and drops the pair it holds (CuckooTable.swift:449-457);
    here the pair is in the expanded table.  The case really takes that path: without the newcomer every entry fits the first
    table, with it the first pass asks for an expansion, and none of its swaps is possible by size."""
    case = next(c for c in cases.CASES if c.name == cases.LARGE_NEWCOMER)
    config = c_config(case.config)
    hashes = [ref.keyword_hash(k) for k in case.keywords]
    sizes = [len(v) for v in case.values]
    newcomer = len(sizes) - 1
    assert 1 + (10 + sizes[newcomer]) + 10 > case.config.max_serialized_bucket_size  # no bucket holds it beside a resident,
    assert all(size == 0 for size in sizes[:newcomer])                                # and swapping one out frees 10 bytes only
    first = heamd.keyword_pir_bucket_count(config, sizes)
    assert first == ref.initial_bucket_count(case.config, sizes)
    indices = [ref.hash_indices_of_hash(h, first, 1) for h in hashes]
    before = heamd.keyword_pir_cuckoo_place(config, hashes[:newcomer], indices[:newcomer], sizes[:newcomer], first, case.seed)
    assert before["status"] == "ok" and before["placed"] == newcomer
    with_it = heamd.keyword_pir_cuckoo_place(config, hashes, indices, sizes, first, case.seed)
    assert with_it["status"] == NEEDS_EXPANSION
    assert with_it["next_bucket_count"] == ref.expanded_bucket_count(case.config, first)
    buckets, _, _, expansions = build_with_library(case)
    assert expansions >= 1 and sum(bucket.count(newcomer) for bucket in buckets) == 1


def test_initial_and_expanded_bucket_counts():
    for h, multiple in ((1, True), (2, True), (3, True), (3, False)):
        for load, limit in ((0.9, 100), (0.5, 64), (0.99, 11)):
            config = ref.Config(h, 10, limit, target_load_factor=load, expansion_factor=1.1 + h, multiple_tables=multiple)
            for sizes in ([], [0], [5] * 50, [65535, 1, 2], list(range(300))):
                got = heamd.keyword_pir_bucket_count(c_config(config), sizes)
                assert got == ref.initial_bucket_count(config, sizes), (h, multiple, load, limit, len(sizes))
        fixed = ref.Config(h, 10, 100, bucket_count=7, multiple_tables=multiple)
        assert heamd.keyword_pir_bucket_count(c_config(fixed), [1, 2, 3]) == ref.initial_bucket_count(fixed, [1, 2, 3])
    # the next count of an expansion: ceil(count * factor) up to a multiple of the table count
    for h, factor, count in ((2, 1.1, 10), (3, 1.5, 3), (1, 1.0001, 1), (2, 2.0, 64), (3, 1.1, 9)):
        config = ref.Config(h, 0, 100, expansion_factor=factor)  # no eviction allowed: the first insertion asks for more
        got = heamd.keyword_pir_cuckoo_place(c_config(config), [5], [[0] * h], [1], count - count % h or h, 1)
        assert got["status"] == NEEDS_EXPANSION
        assert got["next_bucket_count"] == ref.expanded_bucket_count(config, count - count % h or h)


# ---- configuration and arguments --------------------------------------------------------------------------------------------
def test_config_validation():
    lib = heamd.load_library()
    good = dict(hash_function_count=2, max_eviction_count=10, max_serialized_bucket_size=11)
    heamd.CuckooTableConfig(**good).validate()
    heamd.CuckooTableConfig(**good, bucket_count=1).validate()
    heamd.CuckooTableConfig(**good, slot_count=1, expansion_factor=1.0001, target_load_factor=0.999).validate()
    bad = [dict(good, hash_function_count=0), dict(good, max_serialized_bucket_size=10), dict(good, slot_count=0),
           dict(good, slot_count=256), dict(good, expansion_factor=1.0), dict(good, target_load_factor=1.0),
           dict(good, target_load_factor=0.0), dict(good, bucket_count=0)]
    for kwargs in bad:
        config = heamd.CuckooTableConfig(**kwargs)
        if kwargs.get("bucket_count") == 0:
            config.fixed_size = 1
        with pytest.raises(heamd.HeError) as err:
            config.validate()
        assert err.value.name == "invalidCuckooConfig", kwargs
        want = ref.Config(**{k: v for k, v in kwargs.items()})
        with pytest.raises(ref.PirError):
            want.validate()
        # every entry that takes a configuration refuses it
        out = c_size(0)
        assert status_of(lib.he_keyword_pir_bucket_count(ctypes.byref(config), None, 0, ctypes.byref(out))) == \
            "invalidCuckooConfig"
        handle = vp()
        offsets = (ctypes.c_uint64 * 1)(0)
        assert status_of(lib.he_keyword_pir_table_create_device(ctypes.byref(config), None, offsets, None, offsets, 0, 0,
                                                                ctypes.byref(handle), None)) == "invalidCuckooConfig"
        with pytest.raises(heamd.HeError) as err:
            heamd.keyword_pir_cuckoo_place(config, [1], [[0] * config.hash_function_count], [1], 4, 0)
        assert err.value.name == "invalidCuckooConfig"
    assert status_of(lib.he_keyword_pir_config_validate(None)) == "invalidArgument"
    for code, name in ((25, "failedToConstructCuckooTable"), (26, "invalidCuckooConfig"),
                       (27, "invalidHashBucketEntryValueSize"), (28, "invalidHashBucketSlotCount"), (29, NEEDS_EXPANSION)):
        assert lib.he_status_string(code) == name.encode() and STATUS_NAMES[code] == name
    header = open(os.path.join(ROOT, "include", "he_amd.h")).read()
    for code, name in ((25, "FAILED_TO_CONSTRUCT_CUCKOO_TABLE"), (26, "INVALID_CUCKOO_CONFIG"),
                       (27, "INVALID_HASH_BUCKET_ENTRY_VALUE_SIZE"), (28, "INVALID_HASH_BUCKET_SLOT_COUNT"),
                       (29, "CUCKOO_TABLE_NEEDS_EXPANSION")):
        assert re.search(r"HE_ERR_%s = %d\b" % (name, code), header)


def test_placement_argument_errors():
    lib = heamd.load_library()
    config = heamd.CuckooTableConfig(2, 10, 100)

    def place(hashes, indices, sizes, bucket_count, cfg=config):
        return heamd.keyword_pir_cuckoo_place(cfg, hashes, indices, sizes, bucket_count, 0)

    assert place([1, 2], [[0, 1], [1, 0]], [3, 4], 4)["status"] == "ok"
    assert place([], np.zeros((0, 2)), [], 2)["placed"] == 0
    for bucket_count in (0, 3):  # zero, and no multiple of the two tables
        with pytest.raises(heamd.HeError) as err:
            place([1], [[0, 0]], [1], bucket_count)
        assert err.value.name == "invalidArgument"
    with pytest.raises(heamd.HeError) as err:  # an index that is not below the buckets per table
        place([1], [[0, 2]], [1], 4)
    assert err.value.name == "invalidArgument"
    assert place([1], [[0, 3]], [1], 4, heamd.CuckooTableConfig(2, 10, 100, multiple_tables=False))["status"] == "ok"
    with pytest.raises(heamd.HeError) as err:  # above UInt16.max
        place([1], [[0, 0]], [65536], 4, heamd.CuckooTableConfig(2, 10, 1 << 20))
    assert err.value.name == "invalidHashBucketEntryValueSize"
    assert place([1], [[0, 0]], [65535], 4, heamd.CuckooTableConfig(2, 10, 1 << 20))["status"] == "ok"
    with pytest.raises(heamd.HeError) as err:  # the size guard of insert: 1 + 10 + 90 > 100
        place([1], [[0, 0]], [90], 4)
    assert err.value.name == "failedToConstructCuckooTable"
    assert place([1], [[0, 0]], [89], 4)["status"] == "ok"
    # null pointers
    u32p = ctypes.POINTER(c_u32)
    one64, one32, offsets = (ctypes.c_uint64 * 1)(1), (c_u32 * 2)(0, 0), (c_u32 * 5)()
    args = [ctypes.cast(one64, U64P), ctypes.cast(one32, u32p), ctypes.cast(one64, U64P), 1, 4, 0, ctypes.cast(offsets, u32p),
            ctypes.cast(one32, u32p), None, None, None]
    assert status_of(lib.he_keyword_pir_cuckoo_place(ctypes.byref(config), *args)) == "ok"
    for null in (0, 1, 2, 6, 7):
        broken = list(args)
        broken[null] = None
        assert status_of(lib.he_keyword_pir_cuckoo_place(ctypes.byref(config), *broken)) == "invalidArgument", null
    assert status_of(lib.he_keyword_pir_cuckoo_place(None, *args)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_bucket_count(ctypes.byref(config), None, 1, ctypes.byref(c_size(0)))) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_bucket_count(ctypes.byref(config), ctypes.cast(one64, U64P), 1, None)) == "invalidArgument"


def test_device_entry_argument_errors():
    """Errors that are returned before anything touches a device: these hold on a machine without one."""
    lib = heamd.load_library()
    dummy = vp(0x10000)
    for bucket_count in (0, 1 << 32):
        assert status_of(lib.he_keyword_pir_hash_indices_device(dummy, 1, bucket_count, 2, dummy, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_hash_indices_device(dummy, 1, 8, 0, dummy, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_hash_indices_device(dummy, 1, 8, 9, dummy, None)) == "unsupportedHeOperation"
    assert status_of(lib.he_keyword_pir_hash_indices_device(None, 1, 8, 2, dummy, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_hash_indices_device(dummy, 1, 8, 2, None, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_hash_indices_device(dummy, 1 << 32, 8, 2, dummy, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_hash_indices_device(None, 0, 8, 2, None, None)) == "ok"
    for shard_count in (0, 1 << 32):
        assert status_of(lib.he_keyword_pir_shard_indices_device(dummy, 1, shard_count, 0, dummy, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_shard_indices_device(None, 1, 3, 0, dummy, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_shard_indices_device(dummy, 1, 3, 0, None, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_hash_keywords_device(dummy, None, 1, dummy, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_hash_keywords_device(dummy, dummy, 1, None, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_hash_keywords_device(dummy, dummy, 1 << 32, dummy, None)) == "invalidArgument"
    assert status_of(lib.he_keyword_pir_hash_keywords_device(None, None, 0, None, None)) == "ok"
    serialize = lib.he_keyword_pir_serialize_buckets_device
    assert status_of(serialize(dummy, dummy, dummy, None, dummy, 1, 1, 51, dummy, None, None)) == "invalidArgument"
    assert status_of(serialize(dummy, dummy, dummy, dummy, dummy, 1, 1, 51, None, None, None)) == "invalidArgument"
    assert status_of(serialize(None, dummy, dummy, dummy, dummy, 1, 1, 51, dummy, None, None)) == "invalidArgument"
    assert status_of(serialize(dummy, dummy, dummy, dummy, dummy, 1, 1 << 32, 51, dummy, None, None)) == "invalidArgument"
    assert status_of(serialize(None, None, None, None, None, 0, 0, 51, None, None, None)) == "ok"
    # the table object
    config = heamd.CuckooTableConfig(2, 10, 100)
    handle, offsets = vp(), (ctypes.c_uint64 * 2)(0, 1)
    create = lib.he_keyword_pir_table_create_device
    assert status_of(create(ctypes.byref(config), dummy, offsets, dummy, offsets, 1, 0, None, None)) == "invalidArgument"
    assert status_of(create(ctypes.byref(config), dummy, None, dummy, offsets, 1, 0, ctypes.byref(handle), None)) == \
        "invalidArgument"
    assert status_of(create(ctypes.byref(config), dummy, offsets, dummy, None, 1, 0, ctypes.byref(handle), None)) == \
        "invalidArgument"
    falling = (ctypes.c_uint64 * 2)(5, 4)
    assert status_of(create(ctypes.byref(config), dummy, falling, dummy, offsets, 1, 0, ctypes.byref(handle), None)) == \
        "invalidArgument"
    assert status_of(create(ctypes.byref(config), dummy, offsets, dummy, falling, 1, 0, ctypes.byref(handle), None)) == \
        "invalidArgument"
    large = (ctypes.c_uint64 * 2)(0, 65536)
    wide = heamd.CuckooTableConfig(2, 10, 1 << 20)
    assert status_of(create(ctypes.byref(wide), dummy, offsets, dummy, large, 1, 0, ctypes.byref(handle), None)) == \
        "invalidHashBucketEntryValueSize"
    nine = heamd.CuckooTableConfig(9, 10, 100)
    assert status_of(create(ctypes.byref(nine), dummy, offsets, dummy, offsets, 1, 0, ctypes.byref(handle), None)) == \
        "unsupportedHeOperation"
    assert handle.value is None
    lib.he_keyword_pir_table_destroy(None)
    assert lib.he_keyword_pir_table_bucket_count(None) == 0 and lib.he_keyword_pir_table_load_factor(None) == 0.0
    assert status_of(lib.he_keyword_pir_table_entries_device(None, dummy, 51, dummy, None)) == "invalidArgument"
    ctx = heamd.BfvContext(8, 17, [97, 193, 257], host_only=True)
    dims = (c_u32 * 1)(4)
    assert status_of(lib.he_keyword_pir_process_database_device(ctx.h, None, dummy, dims, 1, 51, dummy, dummy, None)) == \
        "invalidArgument"
    assert status_of(lib.he_keyword_pir_process_database_device(None, None, dummy, dims, 1, 51, dummy, dummy, None)) == \
        "invalidArgument"


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    lib = heamd.load_library()
    bound = {name for name, _, _ in heamd.binding.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "he_amd.h")).read()
    assert header == open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")).read()
    exports = open(os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*he_\*;", exports)  # the map exports the he_ prefix
    for name in ENTRIES:
        assert name.startswith("he_") and hasattr(lib, name) and name in bound and re.search(r"\b%s\(" % name, header), name
    declared = set(re.findall(r"\b(he_keyword_pir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(ENTRIES)
    assert "typedef struct he_cuckoo_table_config" in header
    # the structure the binding hands over has the header's fields in the header's order
    fields = re.search(r"typedef struct he_cuckoo_table_config \{(.*?)\} he_cuckoo_table_config;", header, flags=re.S).group(1)
    names = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [name for name, _ in heamd.CuckooTableConfig._fields_]
    for name in ("KeywordPirTable", "CuckooTableConfig", "keyword_pir_hash_keywords", "keyword_pir_hash_indices",
                 "keyword_pir_shard_indices", "keyword_pir_cuckoo_place", "keyword_pir_serialize_buckets",
                 "keyword_pir_bucket_count"):
        assert hasattr(heamd, name), name
