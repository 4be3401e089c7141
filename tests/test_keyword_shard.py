"""Database sharding without a device: he_keyword_sharding_shard_count against the restatement (keyword_shard_reference) over a
table of Sharding values, the partition's plan against the restated plan, the restated shard index against the reference's
known answers, the restated partition's own invariants, the argument errors the device entries return before any launch, and
the ABI (header copy, exports, binding)."""
import ctypes
import json
import os
import re

import pytest

import heamd
import keyword_pir_reference as ref
import keyword_shard_reference as shard_ref
from heamd.binding import STATUS_NAMES, c_size, c_u32, vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (
    "he_keyword_sharding_shard_count", "he_keyword_database_partition_device", "he_keyword_database_partition_plan",
    "he_keyword_database_create_device", "he_keyword_database_destroy", "he_keyword_database_shard_count",
    "he_keyword_database_shard_row_count", "he_keyword_database_shard_table", "he_keyword_database_shard_values",
    "he_keyword_database_order",
)


def status_of(code):
    return STATUS_NAMES[code]


# ---- Sharding -------------------------------------------------------------------------------------------------------------
def sharding_table():
    """(shard_count, entry_count_per_shard, max_shard_count, require_power_of_two, row counts)"""
    rows = []
    powers = [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2**31 - 1, 2**31, 2**31 + 1]
    for count in [0] + powers:  # .shardCount: the three checks of init
        for cap in (None, 0, 1, count - 1, count, count + 1):
            if cap is not None and cap < 0:
                continue
            for power in (False, True):
                rows.append((count, None, cap, power, (0, 1, 1000)))
    for per_shard in (0, 1, 2, 3, 10, 1000):  # .entryCountPerShard: divide, floor at 1, cap, previous power of two
        row_counts = sorted({0, 1, max(per_shard - 1, 0), per_shard, per_shard + 1, 2 * per_shard, 3 * per_shard, 7 * per_shard,
                             7 * per_shard + 1, 1000 * per_shard, 10**6, 2**32 - 2})
        for cap in (None, 0, 1, 2, 3, 5, 8, 2**20):
            for power in (False, True):
                rows.append((None, per_shard, cap, power, tuple(row_counts)))
    for value in powers:  # the resolved count at 1, 2, 3, 2^k +- 1 with the power of two on and off
        for power in (False, True):
            rows.append((None, 1, None, power, (value,)))
            rows.append((None, 1, value, power, (2**33,)))  # the cap below the value
    return rows


def test_shard_count_matches_the_restatement():
    lib = heamd.load_library()
    errors = resolved = 0
    for shard_count, per_shard, cap, power, row_counts in sharding_table():
        ours = heamd.binding.KeywordSharding(shard_count, per_shard, cap, power)
        try:
            want = shard_ref.Sharding(shard_count, per_shard, cap, power)
        except ref.PirError as err:
            assert err.name == "invalidSharding"
            want = None
        for row_count in row_counts:
            out = c_size(12345)
            status = status_of(lib.he_keyword_sharding_shard_count(ctypes.byref(ours), row_count, ctypes.byref(out)))
            case = (shard_count, per_shard, cap, power, row_count)
            if want is None:
                assert status == "invalidSharding" and out.value == 12345, case
                errors += 1
            else:
                assert status == "ok" and out.value == want.shard_count(row_count) >= 1, case
                resolved += 1
    assert errors > 50 and resolved > 500


def test_shard_count_cases_by_name():
    """every invalidSharding case of Sharding.init, and the declared zero cap, one by one through the binding"""
    def count(rows=100, **sharding):
        return heamd.keyword_pir_shard_count(heamd.KeywordSharding(**sharding), rows)

    for bad in (dict(shard_count=0), dict(shard_count=5, max_shard_count=4), dict(shard_count=6, require_power_of_two=True),
                dict(entry_count_per_shard=0), dict(entry_count_per_shard=10, max_shard_count=0)):
        with pytest.raises(heamd.HeError) as err:
            count(**bad)
        assert err.value.name == "invalidSharding", bad
    assert count(shard_count=5, max_shard_count=5) == 5 and count(shard_count=8, require_power_of_two=True) == 8
    assert count(shard_count=6) == 6  # nil and false behave alike
    assert count(rows=9, entry_count_per_shard=10) == 1 and count(rows=0, entry_count_per_shard=10) == 1
    assert count(rows=100, entry_count_per_shard=10) == 10 and count(rows=109, entry_count_per_shard=10) == 10
    assert count(rows=100, entry_count_per_shard=10, max_shard_count=7) == 7
    assert count(rows=100, entry_count_per_shard=10, max_shard_count=7, require_power_of_two=True) == 4
    assert count(rows=100, entry_count_per_shard=10, require_power_of_two=True) == 8
    lib = heamd.load_library()
    sharding, out = heamd.KeywordSharding(shard_count=2), c_size(0)
    assert status_of(lib.he_keyword_sharding_shard_count(None, 1, ctypes.byref(out))) == "invalidArgument"
    assert status_of(lib.he_keyword_sharding_shard_count(ctypes.byref(sharding), 1, None)) == "invalidArgument"


# ---- the plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shard_count", [1, 2, 256, 257, 65536, 65537, 2**24 + 1, 2**32 - 1])
def test_plan_matches_the_restatement(shard_count):
    passes = {1: 0, 2: 1, 256: 1, 257: 2, 65536: 2, 65537: 3, 2**24 + 1: 4, 2**32 - 1: 4}[shard_count]
    for count in (0, 1, 2047, 2048, 2049, 20011, 2**32 - 2):
        for keyword_bytes, value_bytes in ((0, 0), (5, 0), (0, 9), (160000, 2 * 10**8)):
            got = heamd.keyword_pir_partition_plan(count, shard_count, keyword_bytes, value_bytes)
            assert got == shard_ref.plan(count, shard_count, keyword_bytes, value_bytes), (count, keyword_bytes, value_bytes)
            assert got["digit_passes"] == (passes if count else 0)
    ragged = heamd.keyword_pir_partition_plan(20011, shard_count, 1, 1)
    assert ragged["workgroups_per_pass"] >= 3 and 0 < ragged["last_workgroup_rows"] < ragged["rows_per_workgroup"]


def test_plan_argument_errors():
    lib = heamd.load_library()
    for count, shard_count in ((1, 0), (1, 2**32), (2**32 - 1, 3)):
        assert status_of(lib.he_keyword_database_partition_plan(count, shard_count, 1, 1, None, None, None, None, None, None)) \
            == "invalidArgument"
    assert status_of(lib.he_keyword_database_partition_plan(5, 3, 1, 1, None, None, None, None, None, None)) == "ok"


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_restated_shard_index_reproduces_the_known_answers():
    with open(os.path.join(ROOT, "tests", "golden", "keyword_pir_kats.json")) as f:
        kats = json.load(f)
    assert len(kats["sharding"]) >= 2
    for kat in kats["sharding"]:
        assert shard_ref.shard_index(kat["keyword"], kat["shard_count"], kat["other_shard_count"]) == kat["expected"], kat
    assert shard_ref.shard_index is ref.shard_index  # imported, not copied


def test_restated_partition_is_a_stable_split():
    rows = [(bytes([k]) * (k % 4), bytes([255 - k]) * (k % 3)) for k in range(23)]
    indices = [(7 * k) % 5 for k in range(23)]
    indices[4] = 99  # at or above the shard count: the last shard
    order, starts, blobs, offsets = shard_ref.partition(rows, indices, 5)
    assert sorted(order) == list(range(23)) and starts[0] == 0 and starts[-1] == 23 and len(starts) == 6
    for shard in range(5):
        members = order[starts[shard]:starts[shard + 1]]
        assert members == sorted(members)  # input order
        assert all(min(indices[row], 4) == shard for row in members)
    assert 4 in order[starts[4]:starts[5]]
    for part in (0, 1):
        assert offsets[part][0] == 0 and offsets[part][-1] == len(blobs[part])
        for j, row in enumerate(order):
            assert blobs[part][offsets[part][j]:offsets[part][j + 1]] == rows[row][part]
    assert shard_ref.partition(rows, [0] * 23, 1)[0] == list(range(23))  # one shard: the identity
    assert shard_ref.partition([], [], 3) == ([], [0, 0, 0, 0], (b"", b""), ([0], [0]))


# ---- argument errors before any launch ---------------------------------------------------------------------------------------
def test_device_entry_argument_errors():
    """Errors that are returned before anything touches a device: these hold on a machine without one."""
    lib = heamd.load_library()
    d = vp(0x10000)
    partition = lib.he_keyword_database_partition_device

    def call(count=1, shard_count=3, keyword_bytes=4, value_bytes=4, null=()):
        args = [d, d, keyword_bytes, d, d, value_bytes, count, d, shard_count, d, d, d, d, d, d, None, None]
        for position in null:
            args[position] = None
        return status_of(partition(*args))

    assert call(shard_count=0) == "invalidArgument" and call(shard_count=2**32) == "invalidArgument"
    assert call(count=2**32 - 1) == "invalidArgument"
    for position in (1, 4, 7, 10, 12, 13, 14):  # offsets, indices, the four outputs every call writes
        assert call(null=(position,)) == "invalidArgument", position
    for position in (0, 3, 9, 11):  # a blob that holds bytes
        assert call(null=(position,)) == "invalidArgument", position
    for position in (10, 12, 14):  # written even without a row
        assert call(count=0, null=(position,)) == "invalidArgument", position

    config = heamd.CuckooTableConfig(2, 10, 100)
    handle, offsets = vp(), (ctypes.c_uint64 * 2)(0, 1)
    create = lib.he_keyword_database_create_device

    def created(config=config, keyword_offsets=offsets, value_offsets=offsets, count=1, shard_count=3, out=ctypes.byref(handle)):
        return status_of(create(ctypes.byref(config), d, keyword_offsets, d, value_offsets, count, shard_count, 0, 0, out, None))

    assert created(out=None) == "invalidArgument"
    assert created(shard_count=0) == "invalidArgument" and created(shard_count=2**32) == "invalidArgument"
    assert created(keyword_offsets=None) == "invalidArgument" and created(value_offsets=None) == "invalidArgument"
    falling = (ctypes.c_uint64 * 2)(5, 4)
    assert created(keyword_offsets=falling) == "invalidArgument" and created(value_offsets=falling) == "invalidArgument"
    assert created(config=heamd.CuckooTableConfig(0, 10, 100)) == "invalidCuckooConfig"
    assert created(config=heamd.CuckooTableConfig(9, 10, 100)) == "unsupportedHeOperation"
    large = (ctypes.c_uint64 * 2)(0, 65536)
    assert created(config=heamd.CuckooTableConfig(2, 10, 1 << 20), value_offsets=large) == "invalidHashBucketEntryValueSize"
    assert status_of(create(ctypes.byref(config), None, offsets, d, offsets, 1, 3, 0, 0, ctypes.byref(handle), None)) == \
        "invalidArgument"  # a keyword blob that holds a byte
    assert handle.value is None
    lib.he_keyword_database_destroy(None)
    assert lib.he_keyword_database_shard_count(None) == 0 and lib.he_keyword_database_shard_row_count(None, 0) == 0
    assert lib.he_keyword_database_shard_table(None, 0) is None and lib.he_keyword_database_shard_values(None, 0) is None
    assert status_of(lib.he_keyword_database_order(None, None)) == "invalidArgument"


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    lib = heamd.load_library()
    bound = {name for name, _, _ in heamd.binding.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "he_amd.h")).read()
    assert header == open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in bound and re.search(r"\b%s\(" % name, plain), name
    declared = set(re.findall(r"\b(he_keyword_(?:database|sharding)_[a-z0-9_]+)\s*\(", plain))
    assert declared == set(ENTRIES)
    assert STATUS_NAMES[30] == "invalidSharding" and "HE_ERR_INVALID_SHARDING = 30" in header
    lib.he_status_string.restype = ctypes.c_char_p
    assert lib.he_status_string(30) == b"invalidSharding"
    fields = re.search(r"typedef struct he_keyword_sharding \{(.*?)\} he_keyword_sharding;", header, flags=re.S).group(1)
    names = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [name for name, _ in heamd.KeywordSharding._fields_]
    for name in ("KeywordPirShardedDatabase", "KeywordSharding", "keyword_pir_shard_count", "keyword_pir_partition",
                 "keyword_pir_partition_plan"):
        assert hasattr(heamd, name), name
    assert not [name for name in bound if name.endswith("_u32") and "keyword" in name]
