"""SimplePIR over sharded databases without a device: the restatement of DatabaseMap.shardDatabase and SimplePirClientForAllShards
(tests/simple_pir_shard_reference.py) on the worked example of include/he_amd.h, the closed forms the kernels use against the
line-for-line split on random cases, he_simple_pir_shard_plan against the restatement with every error it returns, the form choice
of csrc/simple_pir_shard_plan.hpp through a host program, the argument errors of the device entries, and the ABI."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import heamd
import simple_pir_shard_cases as cases
import simple_pir_shard_reference as R
from test_aliasing_contract import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc")
DEVICE_ENTRIES = ["he_simple_pir_shard_map_device", "he_simple_pir_shard_scatter_device",
                  "he_simple_pir_shard_query_indices_device", "he_simple_pir_shard_assemble_device"]
ENTRIES = ["he_simple_pir_shard_plan"] + DEVICE_ENTRIES
vp = ctypes.c_void_p


def name_of(status):
    return heamd.binding.STATUS_NAMES[status]


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_worked_example():
    raw = list(enumerate(cases.EXAMPLE_VALUES))
    database_map, shards = R.shard_database(raw, cases.EXAMPLE_ORDERS, 2, 2)
    assert [entry.size for entry in database_map.entries] == [5, 0, 2]
    assert [[tuple(chunk) for chunk in entry.chunks] for entry in database_map.entries] == cases.EXAMPLE_CHUNKS
    assert shards == cases.EXAMPLE_SHARDS
    shard_map = R.ShardMap(database_map)
    assert (shard_map.maximum_chunk_count, shard_map.shard_count, shard_map.chunks_per_shard) == (3, 2, 2)
    # query(for:): the real indices first, then fake queries at index 0
    assert R.query_indices(shard_map, 2, 0) == [[0, 0], [0, 1]]
    assert R.query_indices(shard_map, 2, 1) == [[0, 0], [0, 0]]
    assert R.query_indices(shard_map, 2, 2) == [[1, 0], [0, 0]]
    assert R.query_indices(shard_map, 2, 7) == [[0, 0], [0, 0]]
    for index, value in raw:
        lists = R.query_indices(shard_map, 2, index)
        decrypted = [[shards[s][j] for j in lists[s]] for s in range(2)]
        assert R.assemble(shard_map, decrypted, lists, index) == value
    assert R.assemble(shard_map, [[b"zz", b"zz"]] * 2, [[0, 0], [0, 0]], 7) is None
    arrays = R.device_map([5, 0, 2], cases.EXAMPLE_ORDERS, 2, 2)
    assert arrays["chunk_starts"] == [0, 3, 3, 4] and arrays["chunk_shard"] == [1, 0, 1, 0] and arrays["chunk_index"] == [0, 0, 1, 1]
    assert arrays["shard_row_starts"] == [0, 2, 4] and arrays["row_chunk"] == [1, 3, 0, 2] and arrays["mismatch"] == 0


def test_reference_quirks():
    """what only the reference decides: the shard count is the shards USED, a real chunk at index 0 is read from the LAST slot
    that asks for index 0 (a trailing fake query), and of duplicate original indices the last stays"""
    database_map, shards = R.shard_database([(4, b"ab"), (9, b"cdef")], [[2, 0, 1], [2, 1, 0]], 3, 2)
    shard_map = R.ShardMap(database_map)
    assert shard_map.shard_count == 2 and shard_map.maximum_chunk_count == 2 and shard_map.chunks_per_shard == 1  # not 3 shards
    database_map, shards = R.shard_database([(0, b"abcd"), (1, b"ef")], [[0, 1], [1, 0]], 2, 1)
    shard_map = R.ShardMap(database_map)
    lists = R.query_indices(shard_map, 2, 0)
    assert lists == [[0, 1], [0, 1]]
    lists = R.query_indices(shard_map, 2, 1)  # chunks (1, 2), (0, 2): one real query and one fake per shard
    assert lists == [[2, 0], [2, 0]]
    database_map, shards = R.shard_database([(0, b"a"), (1, b"bcd")], [[0, 1], [0, 1]], 2, 1)
    shard_map = R.ShardMap(database_map)
    lists = R.query_indices(shard_map, 2, 0)  # its one chunk is (0, 0): slot 0 is real, slot 1 is the fake query at index 0
    assert lists == [[0, 0], [0, 0]] and shard_map.chunks_per_shard == 2
    decrypted = [[b"1", b"2"], [b"3", b"4"]]  # different bytes per slot: the LAST match is taken
    assert R.assemble(shard_map, decrypted, lists, 0) == b"2"
    database_map, _ = R.shard_database([(5, b"ab"), (5, b"c")], [[0], [0]], 1, 1)
    assert R.ShardMap(database_map).get(5).size == 1


def test_closed_forms_match_the_line_for_line_split():
    rng = np.random.default_rng(20)
    seen = set()
    for _ in range(2000):
        S, C, values, orders = cases.random_split(rng)
        database_map, shards = R.shard_database(list(enumerate(values)), orders, S, C)
        lengths = [len(value) for value in values]
        wanted = [[tuple(chunk) for chunk in entry.chunks] for entry in database_map.entries]
        assert [[tuple(chunk) for chunk in entry] for entry in R.closed_form_locations(lengths, orders, S, C)] == wanted
        for shard in range(S):
            rows = sum(R.rows_given(R.chunk_count(length, C), order, shard, S) for length, order in zip(lengths, orders))
            assert rows == len(shards[shard]), (S, C, lengths, orders, shard)
        arrays = R.device_map(lengths, orders, S, C)
        blob = b"".join(values)
        offsets = cases.flat(values)[1]
        for shard in range(S):  # the slab rows of a shard, filled through row_chunk, are the shard
            for row in range(arrays["shard_row_starts"][shard], arrays["shard_row_starts"][shard + 1]):
                chunk = arrays["row_chunk"][row]
                entry = max(e for e in range(len(values)) if arrays["chunk_starts"][e] <= chunk)
                begin = offsets[entry] + (chunk - arrays["chunk_starts"][entry]) * C
                piece = blob[begin:min(begin + C, offsets[entry + 1])]
                assert piece + bytes(C - len(piece)) == shards[shard][row - arrays["shard_row_starts"][shard]]
        seen |= {(S, C)} | {("length", name) for length in lengths for name, special in
                            (("0", 0), ("C", C), ("CS", C * S), ("CS+1", C * S + 1)) if length == special}
    assert {("length", name) for name in ("0", "C", "CS", "CS+1")} <= seen
    assert {(S, C) for S in range(1, 7) for C in range(1, 6)} <= seen


def test_invalid_orders_fall_back_to_the_identity():
    arrays = R.device_map([3, 3], [[1, 1], [1, 0]], 2, 1)
    assert arrays["mismatch"] == 1 and arrays["orders"] == [[0, 1], [1, 0]]
    assert R.device_map([3], [[0, 2]], 2, 1)["mismatch"] == 1 and R.device_map([3], [[1, 0]], 2, 1)["mismatch"] == 0


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def test_plan_matches_the_restatement():
    for case in cases.GRID:
        values, _ = cases.database(case)
        lengths = [len(value) for value in values]
        offsets = cases.flat(values)[1]
        for address in (0, 8, 16, 4096 + 1):
            got = heamd.simple_pir_shard_plan(offsets, case.shard_count, case.chunk_size, address)
            assert got == R.plan(lengths, case.shard_count, case.chunk_size, address), (case.name, address)
    got = heamd.simple_pir_shard_plan(cases.flat(cases.EXAMPLE_VALUES)[1], 2, 2)
    assert (got["total_chunks"], got["maximum_chunk_count"], got["chunks_per_shard"], got["scatter_form"]) == (4, 3, 2, "byte")
    big = heamd.simple_pir_shard_plan(np.arange(0, 4096 * (2**20 + 1), 4096, dtype=np.uint64), 5, 820)
    assert big == R.plan([4096] * 2**20, 5, 820) and big["map_tiles"] == 8192 and big["scratch_bytes"] < 2**20


def test_plan_errors():
    lib = heamd.load_library()
    offsets = (ctypes.c_uint64 * 3)(0, 5, 9)

    def plan(offsets=offsets, count=2, shard_count=3, chunk_size=4):
        return name_of(lib.he_simple_pir_shard_plan(offsets, count, shard_count, chunk_size, 0, *[None] * 8))

    assert plan() == "ok"  # every out pointer may be NULL, and no device is needed
    assert plan(shard_count=0) == "invalidArgument" and plan(shard_count=257) == "invalidArgument" and plan(shard_count=256) == "ok"
    assert plan(chunk_size=0) == "invalidArgument"
    assert plan(offsets=(ctypes.c_uint64 * 3)(0, 5, 4)) == "invalidArgument"
    assert b"decrease" in lib.he_last_error_message()
    assert plan(offsets=None, count=2**32 - 1) == "invalidArgument"  # before anything is read
    assert plan(offsets=None, count=2) == "invalidArgument" and plan(offsets=None, count=0) == "ok"
    assert plan(offsets=(ctypes.c_uint64 * 3)(0, 2**32 - 2, 2**32), chunk_size=1) == "invalidArgument"  # 2^32 chunks
    assert b"chunks" in lib.he_last_error_message()
    assert plan(offsets=(ctypes.c_uint64 * 3)(0, 2**32 - 2, 2**32 - 1), chunk_size=1) == "ok"


# ---- the plan header, on the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    binary = tmp_path_factory.mktemp("simple_pir_shard") / "simple_pir_shard_form"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "simple_pir_shard_form.cpp"), "-o", str(binary)], check=True)

    def ask(*queries):
        args = []
        for query in queries:
            args += [str(a) for a in query] + ["--"]
        result = subprocess.run([str(binary), *args], capture_output=True, text=True, check=True)
        lines = result.stdout.splitlines()
        assert len(lines) == len(queries)
        return [[int(word) for word in line.split()] for line in lines]

    return ask


def test_plan_header_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "simple_pir_shard_plan.hpp")).read()
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', text)
    assert includes and all(name in ("cstddef", "cstdint") for name in includes), includes


def test_form_over_address_residues_and_chunk_sizes(probe):
    queries = [(written, other, chunk_size, nbytes)
               for written in (0, 1, 4, 8, 12, 16, 24, 4096, 4096 + 8, 2**40 + 16, 2**40 + 15)
               for other in (0, 8, 16, 17)
               for chunk_size in (0, 1, 7, 8, 16, 24, 33, 48, 820, 832)
               for nbytes in (0, chunk_size * 3)]
    widths = {"none": 0, "byte": 1, "word": 8, "wide": 16}
    for query, answer in zip(queries, probe(*[("form", *query) for query in queries])):
        wanted = R.form(*query)
        assert answer == [R.FORMS[wanted], widths[wanted]], query
    for written in range(32):  # the residues of the slab alone, as the scatter sees them
        for chunk_size in (16, 24, 33):
            wanted = ("wide" if written % 16 == 0 else "word" if written % 8 == 0 else "byte") if chunk_size == 16 else \
                ("word" if written % 8 == 0 else "byte") if chunk_size == 24 else "byte"
            assert R.form(written, 0, chunk_size, chunk_size) == wanted


def test_plan_header_matches_the_library(probe):
    picked = [case for case in cases.GRID if case.count in (0, 1, cases.TILE + 1)][:12]
    queries = []
    for case in picked:
        values, _ = cases.database(case)
        queries.append(("plan", case.shard_count, case.chunk_size, *[len(value) for value in values]))
    for case, query, answer in zip(picked, queries, probe(*queries)):
        wanted = R.plan(list(query[3:]), case.shard_count, case.chunk_size)
        assert answer == [0, wanted["total_chunks"], wanted["maximum_chunk_count"], wanted["chunks_per_shard"], wanted["map_tiles"],
                          wanted["count_workgroups"], wanted["scratch_bytes"]], case.name
    assert probe(("plan", 0, 1, 5), ("plan", 257, 1, 5), ("plan", 1, 0, 5)) == [[1], [1], [2]]


# ---- argument errors before any launch -------------------------------------------------------------------------------------------
def test_device_entry_argument_errors():
    lib = heamd.load_library()
    d = [vp(0x10000000 * (k + 1)) for k in range(16)]

    def mapped(count=1, shard_count=3, chunk_size=4, total=2, null=(), at=None):
        args = [d[0], d[1], count, shard_count, chunk_size, total, d[2], d[3], d[4], d[5], d[6], d[7], None]
        for position in null:
            args[position] = None
        for position, address in (at or {}).items():
            args[position] = vp(address)
        return name_of(lib.he_simple_pir_shard_map_device(*args))

    assert mapped(shard_count=0) == "invalidArgument" and mapped(shard_count=257) == "invalidArgument"
    assert mapped(chunk_size=0) == "invalidArgument" and mapped(count=2**32 - 1) == "invalidArgument"
    assert mapped(total=2**32) == "invalidArgument"
    for position in (0, 1, 6, 7, 8, 9, 10):
        assert mapped(null=(position,)) == "invalidArgument", position
    assert mapped(at={6: 0x10000004}) == "invalidArgument" and b"misaligned" in lib.he_last_error_message()
    assert mapped(at={7: 0x20000002}) == "invalidArgument"
    assert mapped(at={8: d[3].value}) == "invalidArgument" and b"overlaps" in lib.he_last_error_message()

    def scattered(count=1, chunk_size=4, total=2, values_bytes=5, null=()):
        args = [d[0], values_bytes, d[1], count, chunk_size, total, d[2], d[3], d[4], None]
        for position in null:
            args[position] = None
        return name_of(lib.he_simple_pir_shard_scatter_device(*args))

    assert scattered(chunk_size=0) == "invalidArgument" and scattered(total=2**32) == "invalidArgument"
    assert scattered(total=0, null=(0, 2, 6, 7, 8)) == "ok"  # nothing to write
    for position in (0, 2, 6, 7, 8):
        assert scattered(null=(position,)) == "invalidArgument", position

    def queried(batch=1, count=1, shard_count=3, total=2, largest=2, per_shard=1, null=()):
        args = [d[0], batch, count, shard_count, total, largest, per_shard, d[1], d[2], d[3], d[4], d[5], None]
        for position in null:
            args[position] = None
        return name_of(lib.he_simple_pir_shard_query_indices_device(*args))

    assert queried(shard_count=0) == "invalidArgument" and queried(largest=3) == "invalidArgument"
    assert queried(per_shard=0) == "invalidArgument" and queried(batch=0, null=(0, 7, 8, 9, 10, 11)) == "ok"
    for position in (0, 7, 8, 9, 10, 11):
        assert queried(null=(position,)) == "invalidArgument", position

    def assembled(batch=1, count=1, shard_count=3, chunk_size=4, total=2, largest=2, per_shard=1, null=()):
        args = [d[0], d[1], d[2], batch, d[3], count, shard_count, chunk_size, total, largest, per_shard, d[4], d[5], d[6], d[7],
                d[8], d[9], None]
        for position in null:
            args[position] = None
        return name_of(lib.he_simple_pir_shard_assemble_device(*args))

    assert assembled(shard_count=257) == "invalidArgument" and assembled(chunk_size=0) == "invalidArgument"
    assert assembled(largest=3) == "invalidArgument" and assembled(per_shard=0) == "invalidArgument"
    assert assembled(batch=0, null=tuple(range(3)) + (4,) + tuple(range(11, 17))) == "ok"
    for position in (0, 1, 2, 4, 11, 12, 13, 14, 15, 16):
        assert assembled(null=(position,)) == "invalidArgument", position


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    lib = heamd.load_library()
    header = open(os.path.join(ROOT, "include", "he_amd.h")).read()
    assert header == open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(he_simple_pir_shard_[a-z0-9_]+)\s*\(", plain)) == set(ENTRIES)
    out = subprocess.run(["nm", "-D", "--defined-only", heamd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    signatures = {name: argtypes for name, _, argtypes in heamd.binding.SIGNATURES}
    parameters = prototypes()
    for name in ENTRIES:
        assert name in exported and hasattr(lib, name) and name in signatures, name
        assert not hasattr(lib, name + "_u32"), name  # nothing here has a slab word
        assert len(parameters[name]) == len(signatures[name]), name
        for (text, _, _), argtype in zip(parameters[name], signatures[name]):
            is_pointer = argtype is vp or hasattr(argtype, "contents")
            assert is_pointer == ("*" in text or text.startswith("he_stream")), (name, text, argtype)
    for name in DEVICE_ENTRIES:
        assert parameters[name][-1][0] == "he_stream s", name
    for value, form in heamd.binding.SIMPLE_PIR_SHARD_FORMS.items():
        assert "#define HE_SIMPLE_PIR_SHARD_FORM_%s %d " % (form.upper(), value) in header and R.FORMS[form] == value
    assert callable(heamd.SimplePirDatabaseMap.shard_database) and callable(heamd.simple_pir_shard_plan)
    for method in ("query_indices", "assemble"):
        assert callable(getattr(heamd.SimplePirClientForAllShards, method))


class FakeMap:
    shard_count, requested_shard_count = 2, 3


def test_client_count_mismatch_raises_as_the_reference_does():
    with pytest.raises(ValueError, match="Mismatching shard count 2 and number of clients 3"):
        heamd.SimplePirClientForAllShards(FakeMap(), [None] * 3)
    with pytest.raises(ValueError, match="without a chunk"):
        heamd.SimplePirClientForAllShards(FakeMap(), [None] * 2)
