"""Database sharding on the device against keyword_shard_reference: the partition of two byte blobs by shard index -- all six
outputs byte for byte, each between guard bytes, with the plan the call ran asserted -- over degenerate shapes, every source
and destination misalignment, one, two, three and four digit passes, and an index out of range; then the sharded-database
object, whose every shard must be, word for word, the table and Eval database the single-table path builds from that shard's
rows."""
import numpy as np
import pytest

import heamd
import keyword_pir_cases as cases
import keyword_pir_reference as ref
import keyword_shard_reference as shard_ref
from heamd.binding import vp

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
LENGTHS = (0, 1, 2, 7, 8, 9, 13, 30)  # as keyword_pir_cases.database


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
    assert buffer.data_ptr() % 64 == 0
    buffer[offset:offset + raw.size] = torch.from_numpy(raw.copy())
    return buffer, vp(buffer.data_ptr() + offset)


def offsets_of(items, first=0):
    out = np.full(len(items) + 1, first, dtype=np.uint64)
    out[1:] += np.cumsum([len(item) for item in items], dtype=np.uint64)
    return out


def random_rows(rng, count, key_lengths=LENGTHS, value_lengths=LENGTHS):
    def items(lengths):
        sizes = rng.choice(lengths, size=count)
        blob = rng.integers(0, 256, size=int(sizes.sum()), dtype=np.uint8).tobytes()
        ends = np.cumsum(sizes)
        return [blob[end - size:end] for size, end in zip(sizes.tolist(), ends.tolist())]

    return list(zip(items(key_lengths), items(value_lengths)))


def run_partition(rows, indices, shard_count, alignments=(0, 0, 0, 0), expect_mismatch=0, claimed_bytes=None):
    """The partition of `rows` on the device with the four blobs (keywords in, values in, keywords out, values out) at
    base + alignments[i]: asserts the plan, the guards and all six outputs against the restatement; -> the restatement."""
    lib = heamd.load_library()
    count = len(rows)
    keywords, values = b"".join(k for k, _ in rows), b"".join(v for _, v in rows)
    key_bytes, value_bytes = claimed_bytes if claimed_bytes is not None else (len(keywords), len(values))
    plan = heamd.keyword_pir_partition_plan(count, shard_count, key_bytes, value_bytes)
    assert plan == shard_ref.plan(count, shard_count, key_bytes, value_bytes)

    keep = [device(np.frombuffer(keywords, dtype=np.uint8), alignments[0]), device(offsets_of([k for k, _ in rows])),
            device(np.frombuffer(values, dtype=np.uint8), alignments[1]), device(offsets_of([v for _, v in rows])),
            device(np.asarray(indices, dtype=np.uint32))]
    out_keywords, out_values = Guarded(key_bytes, alignments[2]), Guarded(value_bytes, alignments[3])
    out_key_offsets, out_value_offsets = Guarded(8 * (count + 1)), Guarded(8 * (count + 1))
    out_order, out_starts = Guarded(4 * count), Guarded(4 * (shard_count + 1))
    flag = Guarded(4)
    flag.buffer[flag.first:flag.first + 4] = 0
    heamd.binding._check(lib.he_keyword_database_partition_device(
        keep[0][1], keep[1][1], key_bytes, keep[2][1], keep[3][1], value_bytes, count, keep[4][1], shard_count,
        out_keywords.ptr, out_key_offsets.ptr, out_values.ptr, out_value_offsets.ptr, out_order.ptr, out_starts.ptr, flag.ptr,
        None))
    want_order, want_starts, want_blobs, want_offsets = shard_ref.partition(rows, [int(i) for i in indices], shard_count)
    assert int(flag.read(np.uint32)[0]) == expect_mismatch
    assert np.array_equal(out_order.read(np.uint32), np.array(want_order, dtype=np.uint32))
    assert np.array_equal(out_starts.read(np.uint32), np.asarray(want_starts, dtype=np.uint32))
    assert np.array_equal(out_key_offsets.read(np.uint64), np.array(want_offsets[0], dtype=np.uint64))
    assert np.array_equal(out_value_offsets.read(np.uint64), np.array(want_offsets[1], dtype=np.uint64))
    got_keywords, got_values = out_keywords.read().tobytes(), out_values.read().tobytes()
    if claimed_bytes is None:
        assert got_keywords == want_blobs[0] and got_values == want_blobs[1]
    else:  # a claimed size below the offsets' span: the bytes both agree on, and the rest of the buffer untouched
        assert got_keywords == want_blobs[0][:key_bytes] and got_values == want_blobs[1][:value_bytes]
    return plan, want_order, want_starts


# ---- degenerate shapes -----------------------------------------------------------------------------------------------------
def test_no_row_and_one_row():
    for shard_count in (1, 3, 300):
        plan, _, starts = run_partition([], [], shard_count)
        assert plan["digit_passes"] == 0 and plan["workgroups_per_pass"] == 0 and not any(starts)
        assert plan["keyword_gather_form"] == plan["value_gather_form"] == "none"
        for row in ((b"key", b"value"), (b"", b""), (b"", b"v"), (b"k" * 30, b"")):
            plan, order, starts = run_partition([row], [shard_count - 1], shard_count)
            assert order == [0] and plan["workgroups_per_pass"] == 1 and plan["last_workgroup_rows"] == 1
            assert plan["keyword_gather_form"] == ("chunk" if row[0] else "none")


@pytest.mark.parametrize("name", ["one shard", "more shards than rows", "all in one shard", "all in the last shard",
                                  "sorted", "reverse sorted"])
def test_degenerate_index_patterns(name):
    rng = np.random.default_rng(len(name))
    rows = random_rows(rng, 300)
    shard_count, indices = {
        "one shard": (1, np.zeros(300, dtype=np.uint32)),
        "more shards than rows": (5000, rng.integers(0, 5000, size=300)),
        "all in one shard": (7, np.full(300, 2)),
        "all in the last shard": (300, np.full(300, 299)),
        "sorted": (40, np.sort(rng.integers(0, 40, size=300))),
        "reverse sorted": (40, np.sort(rng.integers(0, 40, size=300))[::-1]),
    }[name]
    plan, order, starts = run_partition(rows, indices, shard_count, (1, 2, 3, 5))
    assert plan["digit_passes"] == {1: 0, 7: 1, 40: 1, 300: 2, 5000: 2}[shard_count]
    if name in ("one shard", "all in one shard", "all in the last shard", "sorted"):
        assert order == list(range(300))  # already in shard order: the identity
    if name == "more shards than rows":
        assert sum(1 for s in range(shard_count) if starts[s] == starts[s + 1]) >= 4700


# ---- row lengths and alignments --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["empty keywords", "empty values", "both empty", "one long value"])
def test_row_lengths(name):
    rng = np.random.default_rng(len(name))
    if name == "one long value":  # 100 000 bytes among short ones: most chunks lie inside one row
        rows = random_rows(rng, 90)
        rows[41] = (rows[41][0], rng.integers(0, 256, size=100000, dtype=np.uint8).tobytes())
    else:
        rows = random_rows(rng, 700, (0,) if name != "empty values" else LENGTHS, (0,) if name != "empty keywords" else LENGTHS)
    plan, _, _ = run_partition(rows, rng.integers(0, 11, size=len(rows)), 11, (3, 1, 6, 7))
    assert plan["keyword_gather_form"] == ("none" if name in ("empty keywords", "both empty") else "chunk")
    assert plan["value_gather_form"] == ("none" if name in ("empty values", "both empty") else "chunk")


@pytest.mark.parametrize("source", range(8))
def test_every_misalignment_pair(source):
    """keywords (rows mostly shorter than a chunk) and values (one row of 41 bytes among the short ones) read from
    base + source and written to base + 0 .. 7; the other blob takes the mirrored pair"""
    rng = np.random.default_rng(source)
    rows = random_rows(rng, 61)
    rows[17] = (rows[17][0], bytes(range(41)))
    indices = rng.integers(0, 4, size=61)
    for destination in range(8):
        run_partition(rows, indices, 4, (source, destination, destination, source))


# ---- digit passes ------------------------------------------------------------------------------------------------------------
COUNT = 20011  # ten workgroups of 2048 rows in a pass, the last with 1579


@pytest.fixture(scope="module")
def many_rows():
    return random_rows(np.random.default_rng(20011), COUNT, tuple(range(10)), tuple(range(10)))


@pytest.mark.parametrize("shard_count", [3, 256, 257, 65537])
def test_one_two_and_three_digit_passes(many_rows, shard_count):
    rng = np.random.default_rng(shard_count)
    indices = rng.integers(0, shard_count, size=COUNT)
    indices[:3] = (shard_count - 1, 0, shard_count - 1)
    plan, _, _ = run_partition(many_rows, indices, shard_count, (1, 0, 2, 4))
    assert plan["digit_passes"] == {3: 1, 256: 1, 257: 2, 65537: 3}[shard_count]
    assert plan["workgroups_per_pass"] >= 3 and 0 < plan["last_workgroup_rows"] < plan["rows_per_workgroup"]


def test_low_digits_alone_would_misorder(many_rows):
    """Indices that differ only above the first digit, and indices that agree above it: a pass that lost the order of the one
    before it would show here"""
    rng = np.random.default_rng(5)
    indices = np.where(rng.integers(0, 2, size=COUNT) == 0, rng.integers(0, 4, size=COUNT) * 256,
                       rng.integers(0, 4, size=COUNT) * 65536 + 255)
    plan, _, _ = run_partition(many_rows, indices, 4 * 65536, (0, 0, 0, 0))
    assert plan["digit_passes"] == 3


def test_four_digit_passes():
    rng = np.random.default_rng(24)
    shard_count = 2**24 + 1
    indices = rng.integers(0, shard_count, size=1000)
    indices[:4] = (shard_count - 1, 0, 2**24 - 1, shard_count - 1)
    plan, _, starts = run_partition(random_rows(rng, 1000), indices, shard_count)  # out_shard_starts compared as a whole
    assert plan["digit_passes"] == 4 and len(starts) == shard_count + 1


# ---- what the mismatch word reports --------------------------------------------------------------------------------------------
def test_an_index_out_of_range_goes_to_the_last_shard():
    rng = np.random.default_rng(9)
    rows = random_rows(rng, 500)
    indices = rng.integers(0, 300, size=500).astype(np.uint32)
    indices[[7, 123, 499]] = (300, 2**32 - 1, 70000)
    _, order, starts = run_partition(rows, indices, 300, (1, 1, 1, 1), expect_mismatch=1)
    last = order[starts[299]:starts[300]]
    assert {7, 123, 499} <= set(last) and last == sorted(last)


def test_a_claimed_size_below_the_offsets_span_is_reported():
    rng = np.random.default_rng(10)
    rows = random_rows(rng, 100, (3,), (5,))
    run_partition(rows, rng.integers(0, 6, size=100), 6, (2, 0, 5, 0), expect_mismatch=2, claimed_bytes=(3 * 100 - 7, 5 * 100))


def test_partition_through_the_binding():
    import torch

    rng = np.random.default_rng(11)
    rows = random_rows(rng, 333)
    indices = rng.integers(0, 9, size=333)
    order, starts, blobs, offsets = shard_ref.partition(rows, indices.tolist(), 9)
    tensor = lambda raw: torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()  # noqa: E731
    got = heamd.keyword_pir_partition(
        tensor(b"".join(k for k, _ in rows)), heamd.to_device(offsets_of([k for k, _ in rows])),
        tensor(b"".join(v for _, v in rows)), heamd.to_device(offsets_of([v for _, v in rows])),
        torch.from_numpy(indices.astype(np.int32)).cuda(), 9)
    torch.cuda.synchronize()
    assert got["order"].cpu().tolist() == order and got["shard_starts"].cpu().tolist() == starts
    assert got["keywords"].cpu().numpy().tobytes() == blobs[0] and got["values"].cpu().numpy().tobytes() == blobs[1]
    assert got["keyword_offsets"].cpu().tolist() == offsets[0] and got["value_offsets"].cpu().tolist() == offsets[1]


# ---- the object ----------------------------------------------------------------------------------------------------------------
CONFIGS = {c.name: c.config for c in cases.CASES
           if c.name in ("two tables, expansion allowed", "one table of two functions, expansion allowed")}
DEGREE = 64  # the smallest degree test_gpu_keyword_pir.py builds an index-PIR database at


def c_config(config):
    return heamd.CuckooTableConfig(config.hash_function_count, config.max_eviction_count, config.max_serialized_bucket_size,
                                   config.bucket_count, config.expansion_factor, config.target_load_factor,
                                   config.multiple_tables, config.slot_count)


@pytest.fixture(scope="module")
def context():
    t = heamd.generate_primes([17], True, DEGREE)[0]
    return heamd.BfvContext(DEGREE, t, heamd.generate_primes([40, 40, 40, 41], False, DEGREE))


@pytest.fixture(scope="module")
def database():
    keywords, values = cases.database(200, count=194)
    # six keywords come again with other values: equal keywords share a shard, and the first value wins there
    return keywords + keywords[10:16], values + [b"later" + bytes([k]) for k in range(6)]


TABLE_FIELDS = ("bucket_count", "buckets_per_table", "table_count", "largest_bucket_size", "entry_count", "duplicates_dropped",
                "expansion_count", "load_factor")


@pytest.mark.parametrize("other_shard_count", [0, 8], ids=["sha256", "doubleMod"])
@pytest.mark.parametrize("config_name", list(CONFIGS))
def test_sharded_database_end_to_end(context, database, config_name, other_shard_count):
    import torch

    keywords, values = database
    config, shard_count, seed = CONFIGS[config_name], 3, 2**64 - 2  # seed + 2 wraps to 0
    want_shard = [shard_ref.shard_index(k, shard_count, other_shard_count) for k in keywords]
    order, starts, _, _ = shard_ref.partition(list(zip(keywords, values)), want_shard, shard_count)
    sharded = heamd.KeywordPirShardedDatabase(c_config(config), keywords, values, shard_count, other_shard_count, seed)
    assert sharded.shard_count == shard_count and sharded.order().tolist() == order
    assert [sharded.shard_row_count(s) for s in range(shard_count)] == [starts[s + 1] - starts[s] for s in range(shard_count)]
    assert sum(sharded.shard_row_count(s) for s in range(shard_count)) == len(keywords) == 200
    dropped, images = 0, []
    for s, (table, shard_values) in enumerate(sharded.shards()):
        members = order[starts[s]:starts[s + 1]]
        assert members, "three shards of 200 rows: none is empty"
        shard_keywords, own_values = [keywords[row] for row in members], [values[row] for row in members]
        assert shard_values.cpu().numpy().tobytes() == b"".join(own_values)
        single = heamd.KeywordPirTable(c_config(config), shard_keywords, own_values, (seed + s) % 2**64)
        for field in TABLE_FIELDS:
            assert getattr(table, field) == getattr(single, field), (s, field)
        dropped += table.duplicates_dropped
        entry_size = single.largest_bucket_size
        want_rows = single.entries(entry_size).cpu().numpy()
        assert np.array_equal(table.entries(entry_size).cpu().numpy(), want_rows)
        images.append((want_rows, single.buckets_per_table))
        dims = [4, -(-single.buckets_per_table // 4)]
        got_db, got_present = table.process_database(context, dims, entry_size)
        want_db, want_present = single.process_database(context, dims, entry_size)
        torch.cuda.synchronize()
        assert np.array_equal(heamd.to_host(got_db), heamd.to_host(want_db))
        assert np.array_equal(got_present.cpu().numpy(), want_present.cpu().numpy())
    assert dropped == 6

    # every keyword is found in exactly the shard the restatement names, with its first value; a stranger in none
    first_value = {}
    for keyword, value in zip(keywords, values):
        first_value.setdefault(keyword, value)
    h = config.hash_function_count
    for keyword in list(first_value) + [b"no such keyword"]:
        home = shard_ref.shard_index(keyword, shard_count, other_shard_count)
        for s, (rows, per_table) in enumerate(images):
            candidates = ref.hash_indices(keyword, per_table, h)
            buckets = {t * per_table + i if config.multiple_tables else i for t, i in enumerate(candidates)}
            found = [v for v in (ref.find(rows[b].tobytes(), keyword=keyword) for b in sorted(buckets)) if v is not None]
            assert found == ([first_value[keyword]] if keyword in first_value and s == home else []), (keyword, s)


def test_shards_without_a_row_have_no_table():
    keywords, values = cases.database(5, count=5)
    config = CONFIGS["two tables, expansion allowed"]
    want_shard = [shard_ref.shard_index(k, 64) for k in keywords]
    sharded = heamd.KeywordPirShardedDatabase(c_config(config), keywords, values, 64, seed=3)
    lib = heamd.load_library()
    assert sharded.shard_count == 64 and sum(sharded.shard_row_count(s) for s in range(64)) == 5
    for s, (table, shard_values) in enumerate(sharded.shards()):
        rows = want_shard.count(s)
        assert sharded.shard_row_count(s) == rows
        assert (table is None) == (rows == 0) and bool(lib.he_keyword_database_shard_table(sharded.h, s)) == (rows != 0)
        if rows:
            single = heamd.KeywordPirTable(c_config(config), [k for k, w in zip(keywords, want_shard) if w == s],
                                           [v for v, w in zip(values, want_shard) if w == s], 3 + s)
            assert np.array_equal(table.entries().cpu().numpy(), single.entries().cpu().numpy())
        else:
            assert shard_values.numel() == 0
    # a Sharding in place of a count, and no row at all
    by_entries = heamd.KeywordPirShardedDatabase(c_config(config), keywords, values, heamd.KeywordSharding(entry_count_per_shard=2))
    assert by_entries.shard_count == 2
    empty = heamd.KeywordPirShardedDatabase(c_config(config), [], [], 4)
    assert empty.shard_count == 4 and all(table is None for table, _ in empty.shards()) and empty.order().size == 0
